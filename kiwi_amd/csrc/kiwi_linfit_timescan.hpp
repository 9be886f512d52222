// kiwi_linfit_timescan.hpp -- the best coefficients of K basis sources per group at MANY origin times from ONE synthesis of the
// basis (kiwi_hip_linear_fit_time_scan): the linear fit of kiwi_linfit.hpp with the time scan of kiwi_timescan.hpp inside.  A source
// moved by a whole number k of samples has the same synthetic, moved, so the K basis synthetics of a group serve every offset; the
// receiver's taper and reference stay where they are.  For basis source i with row_i = the folded, moment-scaled, untapered
// synthetic (folded_scaled_sample) the scan's basis trace at offset k is, over the receiver's window,
//     s_{i,k}[t] = fp32(syn_factor x fp32(row_i[t - k] x taper[t]))
// -- kiwi_timescan.hpp's rk[i] * w, then the product linfit_gram_kernel forms --, d[t] is the tapered reference, and the sums
// G_r(k), b_r(k), R_r, their layout, the fold over the receivers and the solve are kiwi_linfit.hpp's.  Only the inner products
// depend on k; R_r does not.
// Per chunk of whole groups: the rows are made max |k| samples wider on either side (timescan::set_halo), run_chunk with the plain
// synthetics in memory, then
//   linfit_scan_gram_kernel<K, J>  one workgroup of 256 threads per (receiver, group, pass of J consecutive offsets).  Per slot of
//       the receiver the window is walked in tiles of kTile samples; per tile the K rows over kTile + (offsets of the pass - 1) x
//       kstep extended samples go into LDS once, folded and scaled.  Thread tid takes the samples tid, tid + 256, ... in ascending
//       order across tiles and slots (kTile is a multiple of 256, so the tiles do not change a thread's samples or their order)
//       into J x (NN - 1) fp64 accumulators plus one for R, in linfit_gram_kernel's order: G upper triangle by rows, then b, then R;
//       then its tree, (w0 + w1) + (w2 + w3), and the product with (double) dt.  Every element therefore has the bits
//       linfit_gram_kernel gives on the traces s_{i,k}.  No atomics.
//   linfit_solve_kernel<K>         unchanged, with ngroup x nk "groups" over nbr[(g nk + j)][receiver][NN]
//   linfit_scan_best_kernel        one thread per group: the first smallest misfit among the offsets with status 0, or -1
// Offset 0 is kiwi_hip_linear_fit bit for bit.  Included by kiwi_hip.hip, so compiled under its -ffp-contract=off.

namespace linfit_timescan {

constexpr int kThreads = 256;
constexpr int kTile = 512;                                              // window samples per LDS tile, a multiple of kThreads
// offsets per pass for K basis sources: 2 J (NN - 1) + 2 accumulator registers, at most 178 of the 512 a thread of a 256-thread
// workgroup may hold
constexpr int kPerPass[linfit::kMaxBasis + 1] = { 0, 8, 8, 8, 6, 4, 4, 2, 2 };
static_assert(kTile % kThreads == 0, "a thread's samples and their order must not depend on the tiling");

struct GramArgs {
    SynRows sr;                 // plain synthetics of the chunk, rows with the scan halo
    const RecvDev *recv;
    const float *reft;          // tapered references over the windows
    int isrc0;                  // first source of the chunk in the uploaded batch (moment, rise time)
    int nrec, k0, kstep, nk;
    int lds_row;                // floats per basis row in LDS: kTile + (min(J, nk) - 1) kstep
    float dt, syn_factor;
    double *nbr;                // [(group of the chunk) nk + offset][receiver][NN]
};

template <int K, int J>
__global__ __launch_bounds__(kThreads) void linfit_scan_gram_kernel(GramArgs a)
{
    constexpr int NG = K * (K + 1) / 2, NP = NG + K, NN = NP + 1, NACC = J * NP + 1;
    extern __shared__ __attribute__((aligned(16))) float rows[];            // [K][lds_row]
    __shared__ double part[kThreads / 64][NACC];
    __shared__ float fw[K][kMaxFold];
    __shared__ int fs[K][kMaxFold];
    __shared__ float fr[K][kMaxFold];
    __shared__ int nfold[K];
    const int r = (int)blockIdx.x, g = (int)blockIdx.y, j0 = (int)blockIdx.z * J, tid = (int)threadIdx.x;
    const RecvDev rd = a.recv[r];
    if (!rd.enabled) return;                                                // (its records stay at the zeros of the memset)
    const int nj = min(J, a.nk - j0);
    const int kf = a.k0 + j0 * a.kstep, kl = kf + (nj - 1) * a.kstep;       // first and last offset of the pass
    const int src0 = g * K;                                                 // first basis source of the group in the chunk
    if (tid < K) nfold[tid] = fold_setup(a.sr.risetime[a.isrc0 + src0 + tid], a.dt, fw[tid], fs[tid], fr[tid]);
    __syncthreads();
    const bool unit = (a.syn_factor == 1.f);
    int sh[J];                                                              // LDS index of sample t at offset j: (t - t0) + sh[j]
#pragma unroll
    for (int j = 0; j < J; j++) sh[j] = kl - (kf + (j < nj ? j : 0) * a.kstep);      // (past the last offset: the pass's first once more, dropped)
    double acc[J][NP], accR = 0.0;
#pragma unroll
    for (int j = 0; j < J; j++)
#pragma unroll
        for (int p = 0; p < NP; p++) acc[j][p] = 0.0;
    for (int k = 0; k < rd.ncomp; k++) {
        const CompDev cd = a.sr.comps[rd.slot0 + k];
        const float *__restrict__ tp = a.sr.taper + cd.refofs;
        const float *__restrict__ rt = a.reft + cd.refofs;
        for (int t0 = 0; t0 < cd.wlen; t0 += kTile) {
            const int tn = min(kTile, cd.wlen - t0), ext = tn + (kl - kf);  // <= lds_row
            // rows[i][e] = row_i[t0 - kl + e]: window samples -kl .. wlen - 1 - kf at most, inside the scan halo of max |k|
            for (int i = 0; i < K; i++) {
                const float *__restrict__ sy = a.sr.syn + (size_t)(src0 + i) * a.sr.syn_stride + cd.synofs + cd.halo;
                const float mom = a.sr.moment[a.isrc0 + src0 + i];
                const int nf = nfold[i];
                for (int e = tid; e < ext; e += kThreads)
                    rows[i * a.lds_row + e] = folded_scaled_sample(sy, t0 - kl + e, nf, fw[i], fs[i], fr[i], mom);
            }
            __syncthreads();
            for (int i = tid; i < tn; i += kThreads) {
                const float w = tp[t0 + i];
                const double dv = (double)rt[t0 + i];
#pragma unroll
                for (int j = 0; j < J; j++) {
                    double s[K];
#pragma unroll
                    for (int b = 0; b < K; b++) {
                        const float vt = rows[b * a.lds_row + i + sh[j]] * w;           // make_array_tapered, comparator.f90:1173-1184
                        s[b] = (double)(unit ? vt : a.syn_factor * vt);
                    }
                    int p = 0;
#pragma unroll
                    for (int b = 0; b < K; b++)
#pragma unroll
                        for (int q = b; q < K; q++, p++) acc[j][p] = acc[j][p] + s[b] * s[q];
#pragma unroll
                    for (int b = 0; b < K; b++) acc[j][NG + b] = acc[j][NG + b] + s[b] * dv;
                }
                accR = accR + dv * dv;
            }
            __syncthreads();                                                // (the rows are staged again)
        }
    }
    const int lane = tid & 63, wave = tid >> 6;
#pragma unroll
    for (int j = 0; j < J; j++)
#pragma unroll
        for (int p = 0; p < NP; p++) {
            double v = acc[j][p];
#pragma unroll
            for (int off = 32; off > 0; off >>= 1) v = v + __shfl_down(v, off, 64);
            if (lane == 0) part[wave][j * NP + p] = v;
        }
    {
        double v = accR;
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) v = v + __shfl_down(v, off, 64);
        if (lane == 0) part[wave][J * NP] = v;
    }
    __syncthreads();
    for (int q = tid; q < nj * NN; q += kThreads) {
        const int j = q / NN, p = q - j * NN;
        const int idx = p < NP ? j * NP + p : J * NP;                       // (R goes into every offset's record)
        const double t = (part[0][idx] + part[1][idx]) + (part[2][idx] + part[3][idx]);
        a.nbr[(((size_t)g * a.nk + (j0 + j)) * a.nrec + r) * NN + p] = (double)a.dt * t;
    }
}

// best[g]: the index of the smallest misfit among the offsets of group g with status 0, the lowest among equal values; -1 when no
// offset is solved
__global__ __launch_bounds__(64) void linfit_scan_best_kernel(const double *__restrict__ misfit, const int *__restrict__ status, int ng, int nk,
                                                              int *__restrict__ best)
{
    const int g = (int)(blockIdx.x * 64 + threadIdx.x);
    if (g >= ng) return;
    int b = -1;
    double v = 0.0;
    for (int j = 0; j < nk; j++) {
        if (status[(size_t)g * nk + j] != 0) continue;
        const double m = misfit[(size_t)g * nk + j];
        if (b < 0 || m < v) { b = j; v = m; }
    }
    best[g] = b;
}

template <int K>
static void launch(kiwi_hip_ctx *c, const GramArgs &a, int ng, const double *w_d, int anarchy, double *coef, double *misfit, int *status,
                   double *pivot, double *normal, int *best, hipEvent_t between)
{
    constexpr int J = kPerPass[K];
    const size_t dyn = (size_t)K * (size_t)a.lds_row * sizeof(float);      // at most 8 x (512 + 2048) floats = 80 KiB: timescan::check_setup
    if (!(c->linfit_timescan_attr & (1u << K))) {          // (the attribute belongs to the function on this context's device)
        HIPCHECK(hipFuncSetAttribute(reinterpret_cast<const void *>(&linfit_scan_gram_kernel<K, J>), hipFuncAttributeMaxDynamicSharedMemorySize,
                                     (int)((size_t)K * (size_t)(kTile + 2 * timescan::kMaxShift) * sizeof(float))));
        c->linfit_timescan_attr |= 1u << K;
    }
    hipLaunchKernelGGL((linfit_scan_gram_kernel<K, J>), dim3((unsigned)a.nrec, (unsigned)ng, (unsigned)((a.nk + J - 1) / J)), dim3(kThreads), dyn,
                       c->stream, a);
    HIPCHECK(hipGetLastError());
    HIPCHECK(hipEventRecord(between, c->stream));
    const int nsolve = ng * a.nk;
    hipLaunchKernelGGL(linfit::linfit_solve_kernel<K>, dim3((unsigned)((nsolve + 63) / 64)), dim3(64), 0, c->stream, a.nbr, w_d, a.nrec, anarchy,
                       nsolve, coef, misfit, status, pivot, normal);
    hipLaunchKernelGGL(linfit_scan_best_kernel, dim3((unsigned)((ng + 63) / 64)), dim3(64), 0, c->stream, misfit, status, ng, a.nk, best);
    HIPCHECK(hipGetLastError());
}

static void launch_any(kiwi_hip_ctx *c, int K, const GramArgs &a, int ng, const double *w_d, int anarchy, double *coef, double *misfit,
                       int *status, double *pivot, double *normal, int *best, hipEvent_t between)
{
    by_basis(K, [&](auto k) { launch<k.value>(c, a, ng, w_d, anarchy, coef, misfit, status, pivot, normal, best, between); });
}

// host arrays of the caller for the groups of ONE call of run(); pivot_min, best and normal may be null
struct Out {
    double *coef, *misfit;
    int *status;
    double *pivot_min;
    int *best;
    double *normal;
    Out at(size_t g, size_t K, size_t nk) const
    {
        const size_t nn = (size_t)linfit::nn_of((int)K);
        return Out{ coef + g * nk * K, misfit + g * nk, status + g * nk, pivot_min ? pivot_min + g * nk : nullptr, best ? best + g : nullptr,
                    normal ? normal + g * nk * nn : nullptr };
    }
};

// a group with a basis source that failed to discretise: status 2 and NaN at every offset, best = -1
static void mark_failed(size_t g, size_t K, size_t nk, const Out &out)
{
    const double nan = std::numeric_limits<double>::quiet_NaN();
    std::fill(out.status + g * nk, out.status + (g + 1) * nk, 2);
    std::fill(out.misfit + g * nk, out.misfit + (g + 1) * nk, nan);
    std::fill(out.coef + g * nk * K, out.coef + (g + 1) * nk * K, nan);
    if (out.best) out.best[g] = -1;
}

// groups whose basis sources could not be discretised at all (nothing was uploaded for them): the same, with zero pivots and sums
static void fill_failed(size_t ngroup, size_t K, size_t nk, const Out &out)
{
    for (size_t g = 0; g < ngroup; g++) mark_failed(g, K, nk, out);
    if (out.pivot_min) std::fill(out.pivot_min, out.pivot_min + ngroup * nk, 0.0);
    if (out.normal) std::memset(out.normal, 0, ngroup * nk * (size_t)linfit::nn_of((int)K) * sizeof(double));
}

// what the call cannot do is refused, nothing approximated: everything the linear fit and the time scan refuse, and a misfit filter
// (the taper sits in front of the filter, so a shifted basis trace would need a transform per basis source and offset).  Leaves the
// context prepared.
static void check_setup(kiwi_hip_ctx *c, int K, const timescan::Offsets &of, const Out &out)
{
    linfit::check_setup(c, K, linfit::Out{ out.coef, out.misfit, out.status });
    timescan::check_setup(c, of.k0, of.kstep, of.nk);
    if (c->any_filter)                                     // (prepare(): a filter on an enabled receiver with components)
        throw std::runtime_error("linear_fit_time_scan: an enabled receiver has a misfit filter; the taper sits in front of the filter, so every "
                                     "basis source and offset would need a transform of its own, which is not supported");
}

// the groups [isrc0, isrc0 + ngroup K) of the uploaded batch; adds its HIP-event times to c->linfit_timescan_ms
static void run(kiwi_hip_ctx *c, int isrc0, int ngroup, int K, const timescan::Offsets &of, const double *receiver_weight, int anarchy, const Out &out)
{
    check_setup(c, K, of, out);
    check_group_range("linear_fit_time_scan", c, isrc0, ngroup, K);
    if (ngroup == 0) return;
    const int nrec = (int)c->recv.size(), NN = linfit::nn_of(K), nk = of.nk;
    c->misfit_d.ensure((size_t)c->nsrc * c->nmis, &c->dev_bytes);
    c->global_d.ensure((size_t)c->nsrc, &c->dev_bytes);
    c->fuse_now = false;                                   // the plain synthetics go to memory
    // every source is synthesised (run_chunk shares no synthetics between sources then), as in timescan::run
    timescan::HaloScope halo(c);
    halo.widen(of.max_abs());

    const std::vector<double> w = receiver_weights(c, receiver_weight);
    DevBuf<double> w_d, nbr_d, coef_d, mis_d, piv_d, normal_d;
    DevBuf<int> st_d, best_d;
    w_d.alloc((size_t)nrec, &c->dev_bytes);
    HIPCHECK(hipMemcpyAsync(w_d.p, w.data(), (size_t)nrec * sizeof(double), hipMemcpyHostToDevice, c->stream));
    HIPCHECK(hipStreamSynchronize(c->stream));

    const PooledEvents<5> ev(c);
    std::vector<double> piv_h;
    std::vector<int> best_h;
    int g0 = 0;
    while (g0 < ngroup) {
        // per group: the sums by receiver, nk times those of a plain fit
        const int ng = next_group_chunk(c, isrc0, g0, ngroup, K, 1, (size_t)nk * nrec * NN * sizeof(double), kNoSourceCap);
        const int s0 = isrc0 + g0 * K;
        const size_t nsolve = (size_t)ng * nk;
        HIPCHECK(hipEventRecord(ev[0], c->stream));
        run_chunk(c, s0, ng * K, 0);
        HIPCHECK(hipEventRecord(ev[1], c->stream));
        nbr_d.ensure(nsolve * nrec * NN, &c->dev_bytes);
        coef_d.ensure(nsolve * K, &c->dev_bytes); mis_d.ensure(nsolve, &c->dev_bytes); piv_d.ensure(nsolve, &c->dev_bytes);
        st_d.ensure(nsolve, &c->dev_bytes); best_d.ensure((size_t)ng, &c->dev_bytes);
        if (out.normal) normal_d.ensure(nsolve * NN, &c->dev_bytes);
        HIPCHECK(hipMemsetAsync(nbr_d.p, 0, nsolve * nrec * NN * sizeof(double), c->stream));
        GramArgs a;
        a.sr = SynRows{ c->syn_d.p, c->syn_stride, c->comps_d.p, c->tw_d.p, c->moment_d.p, c->risetime_d.p, nullptr };
        a.recv = c->recv_d.p;
        a.reft = c->reft_d.p;
        a.isrc0 = s0; a.nrec = nrec; a.k0 = of.k0; a.kstep = of.kstep; a.nk = nk;
        a.lds_row = kTile + (std::min(kPerPass[K], nk) - 1) * of.kstep;          // (at most kTile + 2 kMaxShift: the offsets span no more)
        a.dt = c->gm.dt; a.syn_factor = c->syn_factor;
        a.nbr = nbr_d.p;
        launch_any(c, K, a, ng, w_d.p, anarchy ? 1 : 0, coef_d.p, mis_d.p, st_d.p, piv_d.p, out.normal ? normal_d.p : (double *)nullptr, best_d.p, ev[2]);
        HIPCHECK(hipEventRecord(ev[3], c->stream));
        piv_h.resize(nsolve); best_h.resize((size_t)ng);
        const size_t o = (size_t)g0 * nk;
        HIPCHECK(hipMemcpyAsync(out.coef + o * K, coef_d.p, nsolve * K * sizeof(double), hipMemcpyDeviceToHost, c->stream));
        HIPCHECK(hipMemcpyAsync(out.misfit + o, mis_d.p, nsolve * sizeof(double), hipMemcpyDeviceToHost, c->stream));
        HIPCHECK(hipMemcpyAsync(out.status + o, st_d.p, nsolve * sizeof(int), hipMemcpyDeviceToHost, c->stream));
        HIPCHECK(hipMemcpyAsync(out.pivot_min ? out.pivot_min + o : piv_h.data(), piv_d.p, nsolve * sizeof(double), hipMemcpyDeviceToHost, c->stream));
        HIPCHECK(hipMemcpyAsync(out.best ? out.best + g0 : best_h.data(), best_d.p, (size_t)ng * sizeof(int), hipMemcpyDeviceToHost, c->stream));
        if (out.normal) HIPCHECK(hipMemcpyAsync(out.normal + o * NN, normal_d.p, nsolve * NN * sizeof(double), hipMemcpyDeviceToHost, c->stream));
        HIPCHECK(hipEventRecord(ev[4], c->stream));
        HIPCHECK(hipStreamSynchronize(c->stream));
        for (int i = 0; i < 4; i++) ev.add_elapsed(c->linfit_timescan_ms, i, i, i + 1);
        g0 += ng;
    }
    leave_evaluated(c, isrc0, ngroup * K, 0);              // the plain evaluation of the basis sources was made on the way
    for_each_failed_group(c, isrc0, ngroup, K, [&](int g) { mark_failed((size_t)g, (size_t)K, (size_t)nk, out); });
}

// kiwi_hip_linear_fit_time_scan_params piece by piece (PieceCall, kiwi_group_run.hpp)
static PieceCall piece_call(int K, const timescan::Offsets &of, const double *receiver_weight, int anarchy, const Out &out)
{
    auto mine = [=](int s0) { return out.at((size_t)(s0 / K), (size_t)K, (size_t)of.nk); };
    return PieceCall{ K,
        [=](kiwi_hip_ctx *c) { check_setup(c, K, of, out); },
        [=](kiwi_hip_ctx *, int s0, int n) { fill_failed((size_t)(n / K), (size_t)K, (size_t)of.nk, mine(s0)); },
        [=](kiwi_hip_ctx *c, int s0, int n) { run(c, 0, n / K, K, of, receiver_weight, anarchy, mine(s0)); } };
}

} // namespace linfit_timescan
