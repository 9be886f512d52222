// kiwi_linfit_candidates_floating.hpp -- misfits of many GIVEN coefficient vectors per group under floating_l2norm: every receiver
// slides its reference under the fixed taper by whole samples inside its own range (kiwi_hip_set_floating_shiftrange), and per
// candidate the shift with the smallest sum of squared component misfits wins (receiver.f90:439-510).  The taper stays with the
// synthetic, so G_r (synthetic x synthetic) does not depend on the shift: linfit_gram_kernel's sums serve unchanged, and only
// b_r[q] (synthetic x shifted reference) and R_r[q] are new.  For a given x the minimum over the shifts is exact and needs no
// iteration; nothing is FITTED here.  Included by kiwi_hip.hip behind the other linfit headers, under the same -ffp-contract=off:
// every fp64 operation below is rounded on its own, and tests/linfit_candidates_floating_restatement.py restates each in the same
// order (the GPU tests ask for bit identity).  Notation as in kiwi_linfit.hpp and kiwi_linfit_candidates.hpp.
//
//   xcorr       one workgroup of 256 threads per (group, receiver, pass of kFloatShiftsPerPass shifts).  Shift index q (shift
//               fl_lo + q, q ascending) compares the kept synthetics with a_q[t] = refx[t + (fl_ns - 1 - q)] tw[t], the fp32 product
//               floating_norm_kernel forms.  Per q, K + 1 fp64 accumulators: b[q][i] += s_i[t] a_q[t], R[q] += a_q[t] a_q[t], in
//               linfit_gram_kernel's order exactly -- slots ascending into the same accumulators, thread tid takes t = tid,
//               tid + 256, ..., the same wavefront and four-wave tree, then the product with (double) dt.  The K kept samples of t
//               are read once per pass; the reference comes straight from refx (the shifts of a pass read neighbouring words of the
//               same cache lines).  A shift's sums do not depend on the pass it falls into.  They are the bits linfit_gram_kernel
//               gives on a context whose references were moved by that shift (kiwi_hip_shift_ref_seismogram); at shift 0, the bits
//               of the unshifted context.
//   norms       one thread per (group, receiver): n_r = (sum_q sqrt(R_r[q])) / fl_ns, q ascending (the receiver-level form of
//               receiver.f90:501); 0 where w_r == 0 or the mean is not positive: such a receiver is skipped everywhere below.
//   candidates  one workgroup of kFloatCandThreads lanes per (group, tile of kFloatCandThreads candidates); a lane owns ONE
//               candidate with its x in registers.  Per receiver (ascending) the row N_r and, kFloatShiftStage shifts at a time,
//               the rows (b_r[q], R_r[q]) are staged in LDS and read as broadcasts.  xgx by `quad` on G_r, once; per q ascending
//               xb = 0; xb = xb + x_i b_r[q][i]; val_q = max((R_r[q] - 2 xb) + xgx, 0); the FIRST minimum of val_q is kept with its q.
//               m_r = sqrt(min val), shift_r = fl_lo + argmin, v_r = anarchy ? w_r / n_r : w_r, and
//                 outer l1norm   L = L + v_r m_r;            D = D + v_r n_r;              misfit = L / D
//                 outer l2norm   L = L + (v_r v_r) min val;  D = D + (v_r v_r) (n_r n_r);  misfit = sqrt(L / D)
//               (NaN where no receiver counts).  Under l2norm the minimum sits inside the sum: there is no fold-then-evaluate form.
//   fold        one wavefront per group: the tiles' bests folded in linfit_candidates_scan_fold_kernel's order; a lane per receiver
//               recomputes the winner's argmin with the same expressions (best_shift); status and receiver_norm = (float) n_r.
// The order of "best" is kiwi_linfit_candidates.hpp's total order.  No atomics.
// Status of a group: 0 evaluated; 1 no receiver counts: NaN, best_index -1; 2 a basis source failed to discretise (host).

namespace linfit_candidates_floating {

using linfit::kMaxBasis;
using linfit::nn_of;
using linfit::quad;
using linfit::take_better;
using linfit::wave_best;

constexpr int kFloatThreads = 256;
constexpr int kFloatShiftsPerPass = 4;             // J: 4 x (K + 1) = 36 fp64 accumulators at K = 8, no scratch
constexpr int kFloatCandThreads = 256;             // candidates per workgroup
constexpr int kFloatShiftStage = 32;               // shifts per LDS stage: 32 x (K + 1) x 8 bytes = 2.25 KiB at K = 8

// xc: [group of the chunk][receiver][max_ns][K + 1] = (b[q][0 .. K), R[q]); blockIdx.x = receiver, .y = group, .z = pass.  A
// disabled receiver, and the shifts past a receiver's range, are left at the zeros of the memset before the launch
template <int K>
__global__ __launch_bounds__(kFloatThreads) void linfit_float_xcorr_kernel(const float *__restrict__ proc, size_t syn_stride,
                                                                           const RecvDev *__restrict__ recv,
                                                                           const CompDev *__restrict__ comps,
                                                                           const float *__restrict__ refx, const float *__restrict__ tw,
                                                                           int nrec, int max_ns, float syn_factor, float dt,
                                                                           double *__restrict__ xc)
{
    constexpr int J = kFloatShiftsPerPass, M = K + 1;
    __shared__ double part[kFloatThreads / 64][J * M];
    const int r = (int)blockIdx.x, g = (int)blockIdx.y, q0 = (int)blockIdx.z * J, tid = (int)threadIdx.x;
    const RecvDev rd = recv[r];
    if (!rd.enabled) return;
    const int ns = comps[rd.slot0].fl_ns;
    if (q0 >= ns) return;
    const int nj = ns - q0 < J ? ns - q0 : J;
    const bool unit = (syn_factor == 1.f);
    const float *__restrict__ src0 = proc + (size_t)g * K * syn_stride;
    double acc[J][M];
#pragma unroll
    for (int j = 0; j < J; j++)
#pragma unroll
        for (int p = 0; p < M; p++) acc[j][p] = 0.0;
    for (int k = 0; k < rd.ncomp; k++) {
        const CompDev cd = comps[rd.slot0 + k];
        const float *__restrict__ sy = src0 + cd.synofs + cd.halo;
        // shift index q0 + j reads rq[i - j]: indices i + (fl_ns - 1 - q0 - j) in [0, wlen + fl_ns - 2] for j < nj
        const float *__restrict__ rq = refx + cd.refxofs + (cd.fl_ns - 1 - q0);
        const float *__restrict__ tp = tw + cd.refofs;
        for (int i = tid; i < cd.wlen; i += kFloatThreads) {
            double s[K];
#pragma unroll
            for (int a = 0; a < K; a++) {
                const float v = sy[(size_t)a * syn_stride + i];
                s[a] = (double)(unit ? v : syn_factor * v);
            }
            const float tv = tp[i];
#pragma unroll
            for (int j = 0; j < J; j++) {
                if (j < nj) {
                    const float av = rq[i - j] * tv;           // make_array_tapered on the moved data, as floating_norm_kernel
                    const double dv = (double)av;
#pragma unroll
                    for (int a = 0; a < K; a++) acc[j][a] = acc[j][a] + s[a] * dv;
                    acc[j][K] = acc[j][K] + dv * dv;
                }
            }
        }
    }
    const int lane = tid & 63, wave = tid >> 6;
#pragma unroll
    for (int j = 0; j < J; j++)
#pragma unroll
        for (int p = 0; p < M; p++) {
            double v = acc[j][p];
#pragma unroll
            for (int off = 32; off > 0; off >>= 1) v = v + __shfl_down(v, off, 64);
            if (lane == 0) part[wave][j * M + p] = v;
        }
    __syncthreads();
    if (tid < nj * M) {
        const double t = (part[0][tid] + part[1][tid]) + (part[2][tid] + part[3][tid]);
        xc[(((size_t)g * nrec + r) * max_ns + q0) * M + tid] = (double)dt * t;
    }
}

// nr: [group][receiver] n_r, 0 for a receiver that does not count.  One thread per (group, receiver)
__global__ __launch_bounds__(64) void linfit_float_norm_kernel(const double *__restrict__ xc, const double *__restrict__ w,
                                                               const RecvDev *__restrict__ recv, const CompDev *__restrict__ comps,
                                                               int nrec, int max_ns, int M, int ng, double *__restrict__ nr)
{
    const int idx = (int)(blockIdx.x * 64 + threadIdx.x);
    if (idx >= ng * nrec) return;
    const int r = idx % nrec;
    double n = 0.0;
    if (recv[r].enabled && w[r] != 0.0) {
        const int ns = comps[recv[r].slot0].fl_ns;
        const double *__restrict__ row = xc + (size_t)idx * max_ns * M;
        double sum = 0.0;
        for (int q = 0; q < ns; q++) sum = sum + sqrt(row[(size_t)q * M + M - 1]);
        n = sum / (double)ns;
        if (!(n > 0.0)) n = 0.0;
    }
    nr[idx] = n;
}

// the shifts [q0, q0 + nq) of one receiver, rows: [nq][K + 1]: the first minimum of val_q so far in (minv, arg); arg < 0: none yet
template <int K>
__device__ __forceinline__ void float_scan(const double *rows, int nq, int q0, const double (&x)[K], double xgx, double &minv, int &arg)
{
    for (int q = 0; q < nq; q++) {
        const double *row = rows + q * (K + 1);
        double xb = 0.0;
#pragma unroll
        for (int i = 0; i < K; i++) xb = xb + x[i] * row[i];
        double val = (row[K] - 2.0 * xb) + xgx;
        val = val > 0.0 ? val : 0.0;
        if (arg < 0 || val < minv) { minv = val; arg = q0 + q; }
    }
}

// nbr: [group][nrec][NN] (G_r of it), xc: [group][nrec][max_ns][K + 1], nr: [group][nrec], w: [nrec], x: [ncand][K].  misfit:
// [group][ncand] or null; cshift, rmis: [group][ncand][nrec] or null, zeroed before the launch.  tile_v, tile_i: [group][gridDim.x].
// blockIdx.x = tile of candidates, blockIdx.y = group
template <int K>
__global__ __launch_bounds__(kFloatCandThreads) void linfit_candidates_float_kernel(
    const double *__restrict__ nbr, const double *__restrict__ xc, const double *__restrict__ nr, const double *__restrict__ w,
    const RecvDev *__restrict__ recv, const CompDev *__restrict__ comps, int nrec, int max_ns, int anarchy, int outer,
    const double *__restrict__ x, int ncand, double *__restrict__ misfit, short *__restrict__ cshift, float *__restrict__ rmis,
    double *__restrict__ tile_v, int *__restrict__ tile_i)
{
    constexpr int NN = K * (K + 1) / 2 + K + 1, M = K + 1;
    __shared__ double sg[NN];
    __shared__ double sx[kFloatShiftStage * M];
    __shared__ double best_v[kFloatCandThreads / 64];
    __shared__ int best_i[kFloatCandThreads / 64];
    const int g = (int)blockIdx.y, tid = (int)threadIdx.x;
    const int cand = (int)blockIdx.x * kFloatCandThreads + tid;
    const bool live = cand < ncand;
    const size_t slot = (size_t)g * ncand + (live ? cand : 0);
    const double nan = __longlong_as_double(0x7ff8000000000000LL);
    double xv[K];
#pragma unroll
    for (int i = 0; i < K; i++) xv[i] = live ? x[(size_t)cand * K + i] : 0.0;
    double Ls = 0.0, Ds = 0.0;
    bool counted = false;
    for (int r = 0; r < nrec; r++) {                            // (everything that decides a branch here is the same for all lanes)
        const double n = nr[(size_t)g * nrec + r];
        if (!(n > 0.0)) continue;
        const double wr = w[r];
        const CompDev c0 = comps[recv[r].slot0];
        const int ns = c0.fl_ns;
        const double *__restrict__ grow = nbr + ((size_t)g * nrec + r) * NN;
        const double *__restrict__ xrow = xc + ((size_t)g * nrec + r) * max_ns * M;
        double xgx = 0.0, minv = 0.0;
        int arg = -1;
        for (int q0 = 0; q0 < ns; q0 += kFloatShiftStage) {
            const int nq = ns - q0 < kFloatShiftStage ? ns - q0 : kFloatShiftStage;
            __syncthreads();                                    // the stage before this one has been read by every wavefront
            if (q0 == 0 && tid < NN) sg[tid] = grow[tid];
            for (int p = tid; p < nq * M; p += kFloatCandThreads) sx[p] = xrow[(size_t)q0 * M + p];
            __syncthreads();
            if (q0 == 0) {
                double xb0;
                quad<K>(sg, xv, xb0, xgx);
            }
            float_scan<K>(sx, nq, q0, xv, xgx, minv, arg);
        }
        const double m = sqrt(minv);
        const double v = anarchy ? wr / n : wr;
        if (outer == 1) {
            Ls = Ls + v * m;
            Ds = Ds + v * n;
        } else {
            const double v2 = v * v;
            Ls = Ls + v2 * minv;
            Ds = Ds + v2 * (n * n);
        }
        counted = true;
        if (live) {
            if (rmis) rmis[slot * nrec + r] = (float)m;
            if (cshift) cshift[slot * nrec + r] = (short)(c0.fl_lo + arg);
        }
    }
    double mf = nan;
    if (counted) mf = outer == 1 ? Ls / Ds : sqrt(Ls / Ds);
    if (live && misfit) misfit[slot] = mf;
    double bv = mf;
    int bi = (live && mf == mf) ? cand : -1;
    wave_best(bv, bi);
    if ((tid & 63) == 0) { best_v[tid >> 6] = bv; best_i[tid >> 6] = bi; }
    __syncthreads();
    if (tid == 0) {
        for (int k = 1; k < kFloatCandThreads / 64; k++) take_better(bv, bi, best_v[k], best_i[k]);
        tile_v[(size_t)g * gridDim.x + blockIdx.x] = bv;
        tile_i[(size_t)g * gridDim.x + blockIdx.x] = bi;
    }
}

// best_shift: [group][nrec]; rnorm: [group][nrec] or null.  blockIdx.x = group
template <int K>
__global__ __launch_bounds__(64) void linfit_candidates_float_fold_kernel(
    const double *__restrict__ tile_v, const int *__restrict__ tile_i, int ntile, const double *__restrict__ nbr,
    const double *__restrict__ xc, const double *__restrict__ nr, const RecvDev *__restrict__ recv, const CompDev *__restrict__ comps,
    int nrec, int max_ns, const double *__restrict__ x, int *__restrict__ best_index, double *__restrict__ best_misfit,
    int *__restrict__ status, int *__restrict__ best_shift, float *__restrict__ rnorm)
{
    constexpr int NN = K * (K + 1) / 2 + K + 1, M = K + 1;
    const int g = (int)blockIdx.x, lane = (int)threadIdx.x;
    double bv = 0.0;
    int bi = -1;
    for (int t = lane; t < ntile; t += 64) take_better(bv, bi, tile_v[(size_t)g * ntile + t], tile_i[(size_t)g * ntile + t]);
    wave_best(bv, bi);
    bv = __shfl(bv, 0, 64);
    bi = __shfl(bi, 0, 64);
    double xv[K];
#pragma unroll
    for (int i = 0; i < K; i++) xv[i] = bi >= 0 ? x[(size_t)bi * K + i] : 0.0;
    int counts = 0;
    for (int r = lane; r < nrec; r += 64) {
        const double n = nr[(size_t)g * nrec + r];
        int sh = 0;
        if (n > 0.0) {
            counts = 1;
            if (bi >= 0) {
                const CompDev c0 = comps[recv[r].slot0];
                double xb0, xgx, minv = 0.0;
                int arg = -1;
                quad<K>(nbr + ((size_t)g * nrec + r) * NN, xv, xb0, xgx);
                float_scan<K>(xc + ((size_t)g * nrec + r) * max_ns * M, c0.fl_ns, 0, xv, xgx, minv, arg);
                sh = c0.fl_lo + arg;
            }
        }
        best_shift[(size_t)g * nrec + r] = sh;
        if (rnorm) rnorm[(size_t)g * nrec + r] = (float)n;
    }
    const int any = __any(counts);
    if (lane == 0) {
        best_index[g] = bi;
        best_misfit[g] = bi >= 0 ? bv : __longlong_as_double(0x7ff8000000000000LL);
        status[g] = any != 0 ? 0 : 1;
    }
}

// x [ncand][K] (host), shared by all groups; outer_norm 1 l1norm, 2 l2norm.  Host arrays for the groups of ONE call of run():
// best_index, best_misfit, status [group]; best_shift [group][nrec]; misfit [group][ncand], cand_shift, receiver_misfit
// [group][ncand][nrec], receiver_norm [group][nrec], each of the last four may be null
struct Floating {
    const double *x; int ncand, outer_norm;
    int *best_index; double *best_misfit; int *status; int *best_shift;
    double *misfit; short *cand_shift;
    float *receiver_misfit, *receiver_norm;
    Floating at(int g, int nrec) const
    {
        Floating f = *this;
        f.best_index += g; f.best_misfit += g; f.status += g; f.best_shift += (size_t)g * nrec;
        if (misfit) f.misfit += (size_t)g * ncand;
        if (cand_shift) f.cand_shift += (size_t)g * ncand * nrec;
        if (receiver_misfit) f.receiver_misfit += (size_t)g * ncand * nrec;
        if (receiver_norm) f.receiver_norm += (size_t)g * nrec;
        return f;
    }
};

// what this call cannot do is refused before anything runs, nothing approximated.  Leaves the context prepared
static void check_setup(kiwi_hip_ctx *c, int K, const Floating &fl)
{
    if (K < 1 || K > kMaxBasis)
        throw std::runtime_error("linear_fit_candidates_floating: K = " + std::to_string(K) + " basis sources per group; 1 to " +
                                 std::to_string(kMaxBasis) + " are supported");
    if (!fl.best_shift) throw std::runtime_error("linear_fit_candidates_floating: null best_shift array");
    refusing("linear_fit_candidates_floating", [&] {
        linfit::check_candidates(linfit::Candidates{ fl.x, fl.ncand, fl.outer_norm, 0, fl.best_index, fl.best_misfit, fl.status, nullptr,
                                                     nullptr, nullptr, nullptr }, K);
    });
    if (fl.cand_shift && !fl.misfit) throw std::runtime_error("linear_fit_candidates_floating: a cand_shift array without a misfit array");
    if (c->method == KIWI_FLOATING_L1NORM)
        throw std::runtime_error("linear_fit_candidates_floating: the misfit method is floating_l1norm, whose sums of absolute values are not "
                                 "quadratic in the coefficients; set floating_l2norm");
    if (c->method != KIWI_FLOATING_L2NORM)
        throw std::runtime_error("linear_fit_candidates_floating: the misfit method must be floating_l2norm (without shift ranges "
                                 "kiwi_hip_linear_fit_candidates answers under l2norm; floating_l1norm is not quadratic in the coefficients)");
    double d = 0.0;
    int s = 0;
    refusing("linear_fit_candidates_floating", [&] { linfit::check_setup(c, K, linfit::Out{ &d, &d, &s }, nullptr, nullptr, true); });
    if (fl.cand_shift)
        for (const auto &r : c->recv)
            if (r.enabled && r.ncomp > 0 && (r.float_lo < -32768 || r.float_hi > 32767))
                throw std::runtime_error("linear_fit_candidates_floating: a shift range beyond 16 bits does not fit the cand_shift array");
}

// device bytes of one group's outputs and sums beyond linfit_gram_kernel's (the chunk of run() is bounded by them too)
static size_t float_bytes(const Floating &fl, int K, int nrec, int max_ns)
{
    const size_t ntile = (size_t)(fl.ncand + kFloatCandThreads - 1) / kFloatCandThreads;
    return (size_t)nrec * ((size_t)max_ns * (K + 1) * sizeof(double) + sizeof(double) + sizeof(int) + sizeof(float)) +
           ntile * (sizeof(double) + sizeof(int)) +
           (size_t)fl.ncand * ((fl.misfit ? sizeof(double) : 0) + (fl.cand_shift ? (size_t)nrec * sizeof(short) : 0) +
                               (fl.receiver_misfit ? (size_t)nrec * sizeof(float) : 0));
}

struct Bufs {
    DevBuf<double> w, x, nbr, xc, nr, misfit, tile_v, best_misfit;
    DevBuf<float> rmis, rnorm;
    DevBuf<short> cshift;
    DevBuf<int> tile_i, best_index, status, best_shift;
};

template <int K>
static void launch_xcorr(kiwi_hip_ctx *c, int ng, Bufs &b)
{
    const int nrec = (int)c->recv.size(), npass = (c->max_ns + kFloatShiftsPerPass - 1) / kFloatShiftsPerPass;
    hipLaunchKernelGGL(linfit_float_xcorr_kernel<K>, dim3((unsigned)nrec, (unsigned)ng, (unsigned)npass), dim3(kFloatThreads), 0, c->stream,
                       c->proc_d.p, c->syn_stride, c->recv_d.p, c->comps_d.p, c->refx_d.p, c->tw_d.p, nrec, c->max_ns, c->syn_factor, c->gm.dt,
                       b.xc.p);
    HIPCHECK(hipGetLastError());
}

template <int K>
static void launch_cand(kiwi_hip_ctx *c, int ng, int anarchy, const Floating &fl, Bufs &b)
{
    const int nrec = (int)c->recv.size(), ntile = (fl.ncand + kFloatCandThreads - 1) / kFloatCandThreads;
    const size_t ncr = (size_t)ng * fl.ncand * nrec;
    hipLaunchKernelGGL(linfit_float_norm_kernel, dim3((unsigned)((ng * nrec + 63) / 64)), dim3(64), 0, c->stream, b.xc.p, b.w.p, c->recv_d.p,
                       c->comps_d.p, nrec, c->max_ns, K + 1, ng, b.nr.p);
    HIPCHECK(hipGetLastError());
    short *cs = fl.cand_shift ? b.cshift.p : nullptr;
    float *rm = fl.receiver_misfit ? b.rmis.p : nullptr;
    if (cs) HIPCHECK(hipMemsetAsync(cs, 0, ncr * sizeof(short), c->stream));
    if (rm) HIPCHECK(hipMemsetAsync(rm, 0, ncr * sizeof(float), c->stream));
    hipLaunchKernelGGL(linfit_candidates_float_kernel<K>, dim3((unsigned)ntile, (unsigned)ng), dim3(kFloatCandThreads), 0, c->stream, b.nbr.p,
                       b.xc.p, b.nr.p, b.w.p, c->recv_d.p, c->comps_d.p, nrec, c->max_ns, anarchy, fl.outer_norm, b.x.p, fl.ncand,
                       fl.misfit ? b.misfit.p : (double *)nullptr, cs, rm, b.tile_v.p, b.tile_i.p);
    HIPCHECK(hipGetLastError());
    hipLaunchKernelGGL(linfit_candidates_float_fold_kernel<K>, dim3((unsigned)ng), dim3(64), 0, c->stream, b.tile_v.p, b.tile_i.p, ntile,
                       b.nbr.p, b.xc.p, b.nr.p, c->recv_d.p, c->comps_d.p, nrec, c->max_ns, b.x.p, b.best_index.p, b.best_misfit.p, b.status.p,
                       b.best_shift.p, fl.receiver_norm ? b.rnorm.p : (float *)nullptr);
    HIPCHECK(hipGetLastError());
}

// groups that have no evaluation (a basis source failed to discretise): status 2, NaN, best_index -1, zeros per receiver
static void fill_failed(int ngroup, int nrec, const Floating &fl)
{
    const double nan = std::numeric_limits<double>::quiet_NaN();
    for (int g = 0; g < ngroup; g++) { fl.status[g] = 2; fl.best_index[g] = -1; fl.best_misfit[g] = nan; }
    std::fill(fl.best_shift, fl.best_shift + (size_t)ngroup * nrec, 0);
    const size_t nc = (size_t)ngroup * fl.ncand;
    if (fl.misfit) std::fill(fl.misfit, fl.misfit + nc, nan);
    if (fl.cand_shift) std::fill(fl.cand_shift, fl.cand_shift + nc * nrec, (short)0);
    if (fl.receiver_misfit) std::fill(fl.receiver_misfit, fl.receiver_misfit + nc * nrec, 0.f);
    if (fl.receiver_norm) std::fill(fl.receiver_norm, fl.receiver_norm + (size_t)ngroup * nrec, 0.f);
}

// the groups [isrc0, isrc0 + ngroup K) of the uploaded batch, on linfit::run's skeleton: per chunk of whole groups the floating
// evaluation with the tapered synthetics kept, the Gram and xcorr kernels, the candidate kernels, the downloads.  Adds its
// HIP-event times to c->linfit_cand_floating_ms
static void run(kiwi_hip_ctx *c, int isrc0, int ngroup, int K, const double *receiver_weight, int anarchy, const Floating &fl)
{
    check_setup(c, K, fl);
    check_group_range("linear_fit_candidates_floating", c, isrc0, ngroup, K);
    if (ngroup == 0) return;
    const int nrec = (int)c->recv.size(), NN = nn_of(K), M = K + 1, max_ns = c->max_ns;
    c->misfit_d.ensure((size_t)c->nsrc * c->nmis, &c->dev_bytes);
    c->global_d.ensure((size_t)c->nsrc, &c->dev_bytes);
    const int proc_which = 2;                                 // (the context refuses a misfit filter under a floating norm)
    c->fuse_now = can_fuse(c, proc_which, isrc0, ngroup * K);

    const std::vector<double> w = receiver_weights(c, receiver_weight);
    Bufs b;
    b.w.alloc((size_t)nrec, &c->dev_bytes);
    b.x.alloc((size_t)fl.ncand * K, &c->dev_bytes);
    HIPCHECK(hipMemcpyAsync(b.w.p, w.data(), (size_t)nrec * sizeof(double), hipMemcpyHostToDevice, c->stream));
    HIPCHECK(hipMemcpyAsync(b.x.p, fl.x, (size_t)fl.ncand * K * sizeof(double), hipMemcpyHostToDevice, c->stream));
    HIPCHECK(hipStreamSynchronize(c->stream));

    const PooledEvents<5> ev(c);
    const size_t ntile = (size_t)(fl.ncand + kFloatCandThreads - 1) / kFloatCandThreads;
    // per group: the sums by receiver, the sums per shift and the outputs
    const size_t per_group = (size_t)nrec * NN * sizeof(double) + float_bytes(fl, K, nrec, max_ns);
    int g0 = 0;
    while (g0 < ngroup) {
        const int ng = next_group_chunk(c, isrc0, g0, ngroup, K, 3, per_group, kNoSourceCap);
        const int s0 = isrc0 + g0 * K;
        const size_t ngr = (size_t)ng * nrec, nc = (size_t)ng * fl.ncand;
        HIPCHECK(hipEventRecord(ev[0], c->stream));
        run_chunk(c, s0, ng * K, proc_which);
        HIPCHECK(hipEventRecord(ev[1], c->stream));
        b.nbr.ensure(ngr * NN, &c->dev_bytes);
        b.xc.ensure(ngr * max_ns * M, &c->dev_bytes);
        b.nr.ensure(ngr, &c->dev_bytes);
        HIPCHECK(hipMemsetAsync(b.nbr.p, 0, ngr * NN * sizeof(double), c->stream));
        HIPCHECK(hipMemsetAsync(b.xc.p, 0, ngr * max_ns * M * sizeof(double), c->stream));
        linfit::launch_gram_any(c, K, ng, nullptr, b.nbr.p);
        by_basis(K, [&](auto k) { launch_xcorr<k.value>(c, ng, b); });
        HIPCHECK(hipEventRecord(ev[2], c->stream));
        b.tile_v.ensure((size_t)ng * ntile, &c->dev_bytes); b.tile_i.ensure((size_t)ng * ntile, &c->dev_bytes);
        b.best_index.ensure((size_t)ng, &c->dev_bytes); b.best_misfit.ensure((size_t)ng, &c->dev_bytes); b.status.ensure((size_t)ng, &c->dev_bytes);
        b.best_shift.ensure(ngr, &c->dev_bytes);
        if (fl.misfit) b.misfit.ensure(nc, &c->dev_bytes);
        if (fl.cand_shift) b.cshift.ensure(nc * nrec, &c->dev_bytes);
        if (fl.receiver_misfit) b.rmis.ensure(nc * nrec, &c->dev_bytes);
        if (fl.receiver_norm) b.rnorm.ensure(ngr, &c->dev_bytes);
        by_basis(K, [&](auto k) { launch_cand<k.value>(c, ng, anarchy ? 1 : 0, fl, b); });
        HIPCHECK(hipEventRecord(ev[3], c->stream));
        const Floating o = fl.at(g0, nrec);
        HIPCHECK(hipMemcpyAsync(o.best_index, b.best_index.p, (size_t)ng * sizeof(int), hipMemcpyDeviceToHost, c->stream));
        HIPCHECK(hipMemcpyAsync(o.best_misfit, b.best_misfit.p, (size_t)ng * sizeof(double), hipMemcpyDeviceToHost, c->stream));
        HIPCHECK(hipMemcpyAsync(o.status, b.status.p, (size_t)ng * sizeof(int), hipMemcpyDeviceToHost, c->stream));
        HIPCHECK(hipMemcpyAsync(o.best_shift, b.best_shift.p, ngr * sizeof(int), hipMemcpyDeviceToHost, c->stream));
        if (fl.misfit) HIPCHECK(hipMemcpyAsync(o.misfit, b.misfit.p, nc * sizeof(double), hipMemcpyDeviceToHost, c->stream));
        if (fl.cand_shift) HIPCHECK(hipMemcpyAsync(o.cand_shift, b.cshift.p, nc * nrec * sizeof(short), hipMemcpyDeviceToHost, c->stream));
        if (fl.receiver_misfit) HIPCHECK(hipMemcpyAsync(o.receiver_misfit, b.rmis.p, nc * nrec * sizeof(float), hipMemcpyDeviceToHost, c->stream));
        if (fl.receiver_norm) HIPCHECK(hipMemcpyAsync(o.receiver_norm, b.rnorm.p, ngr * sizeof(float), hipMemcpyDeviceToHost, c->stream));
        HIPCHECK(hipEventRecord(ev[4], c->stream));
        HIPCHECK(hipStreamSynchronize(c->stream));
        for (int i = 0; i < 4; i++) ev.add_elapsed(c->linfit_cand_floating_ms, i, i, i + 1);
        g0 += ng;
    }
    leave_evaluated(c, isrc0, ngroup * K, proc_which);
    for_each_failed_group(c, isrc0, ngroup, K, [&](int g) { fill_failed(1, nrec, fl.at(g, nrec)); });
}

// kiwi_hip_linear_fit_candidates_floating_params piece by piece (PieceCall, kiwi_group_run.hpp)
static PieceCall piece_call(int K, const double *receiver_weight, int anarchy, const Floating &fl)
{
    return PieceCall{ K,
        [=](kiwi_hip_ctx *c) { check_setup(c, K, fl); },
        [=](kiwi_hip_ctx *c, int s0, int n) { fill_failed(n / K, (int)c->recv.size(), fl.at(s0 / K, (int)c->recv.size())); },
        [=](kiwi_hip_ctx *c, int s0, int n) { run(c, 0, n / K, K, receiver_weight, anarchy, fl.at(s0 / K, (int)c->recv.size())); } };
}

} // namespace linfit_candidates_floating
