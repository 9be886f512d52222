// kiwi_linfit.hpp -- least-squares coefficients of K basis sources per group under the time-domain l2norm: the inner products
// between SYNTHETICS (the comparator only ever pairs a synthetic with a reference), the normal equations of every group and
// their solution.  For `moment_tensor` and `mt_eikonal` the six tensor components enter the centroid table, and so the
// synthetics, linearly (kiwi_host.hpp discretize_moment_tensor, kiwi_host_eikonal.hpp): with six unit tensors as basis the
// coefficients ARE the best moment tensor of a trial location (kiwi_amd/mtfit.py).  Included by kiwi_hip.hip after the
// evaluation, so it is compiled with that object's -ffp-contract=off: every fp64 product, sum, quotient and root below is
// rounded on its own, and tests/linfit_restatement.py restates each step in the same order (the GPU tests ask for bit identity).
//
// Sources [isrc0, isrc0 + ngroup K) of the uploaded batch are ngroup groups of K consecutive basis sources.  Per chunk of whole
// groups (bounded like an evaluation's chunks, KIWI_HIP_CHUNK_MB):
//   evaluate  run_chunk with the processed synthetics kept (tapered; filtered where a receiver has a misfit filter): misfits,
//             norm factors and global misfits of the basis sources are left exactly as kiwi_hip_eval leaves them
//   gram      one workgroup of 256 threads per (group, receiver).  With s_i[t] = syn_factor x kept trace of basis source i (the
//             fp32 product the comparator forms) and d[t] the reference side of the same comparison, every thread keeps
//             NN = K (K + 1) / 2 + K + 1 fp64 accumulators, in this order: G[i][j] (i <= j, upper triangle by rows), b[i], R:
//                 G[i][j] += s_i[t] s_j[t]      b[i] += s_i[t] d[t]      R += d[t] d[t]
//             (a product of two fp32 values is exact in fp64; only the order of the additions matters).  A thread takes the
//             samples t = tid, tid + 256, ... of the receiver's first slot in ascending order, then those of the next slot, and
//             so on, into the SAME accumulators.  Tree: within a wavefront v[lane] = v[lane] + v[lane + off] for off = 32, 16,
//             8, 4, 2, 1; then (w0 + w1) + (w2 + w3) over the four wavefronts; the total times (double) dt.  The K traces of a
//             sample are read once and feed all pairs from registers: each sample of each kept trace is read from memory once.
//             The order is the same for every K, chunk size, isrc0 and group position.  No atomics.
//   solve     one thread per group.  Receivers r ascending: w = receiver_weight[r] (0 for a disabled receiver); a receiver with
//             w == 0 is skipped; anarchy: w = R_r > 0 ? w / sqrt(R_r) : 0; N[p] = N[p] + (w w) N_r[p].  D_i = G_ii; scaling
//             s_i = 1 / sqrt(D_i); A_ij = (G_ij s_i) s_j, A_ii = 1 (from here to coef_i: scaled_cholesky, which the reweighted
//             solves of kiwi_linfit_robust.hpp share).  Cholesky A = L L^T by columns j ascending:
//                 d = 1; d = d - L_jk L_jk (k < j ascending); pivot d; L_jj = sqrt(d);
//                 v = A_ij; v = v - L_ik L_jk (k < j ascending); L_ij = v / L_jj   (i > j)
//             y_i = (b_i s_i - sum_{k < i} L_ik y_k) / L_ii; z_i = (y_i - sum_{k > i} L_ki z_k) / L_ii (i descending, k
//             ascending); coef_i = z_i s_i.  misfit = sqrt(max((R - 2 x.b) + x.G.x, 0) / R) with x.b and the rows of G x summed
//             from zero in ascending index order and x.G.x = sum_i x_i (G x)_i.  pivot_min: the smallest pivot up to and
//             including the one that broke down; 0 for a diagonal that is not positive.
// Status of a group: 0 solved; 1 no solution (a diagonal element not positive, a pivot <= K 2^-52, or R not positive); 2 a
// basis source of the group failed to discretise (set on the host).  Groups with status != 0 answer NaN coefficients and misfit.

namespace linfit {

constexpr int kMaxBasis = 8;
constexpr int kThreads = 256;

__host__ __device__ constexpr int nn_of(int K) { return K * (K + 1) / 2 + K + 1; }
__host__ __device__ constexpr int tri(int K, int i, int j) { return i * K - i * (i - 1) / 2 + (j - i); }     // i <= j

// nbr: [group of the chunk][receiver][NN]; blockIdx.x = receiver (all of them: a disabled one is left at the zeros of the
// memset before the launch), blockIdx.y = group.  pairs: the chunk's (source, slot) records where transforms ran, else null
template <int K>
__global__ __launch_bounds__(kThreads) void linfit_gram_kernel(const float *__restrict__ proc, size_t syn_stride,
                                                               const RecvDev *__restrict__ recv, const CompDev *__restrict__ comps,
                                                               const float *__restrict__ reft, const float *__restrict__ reffilt,
                                                               const FftPair *__restrict__ pairs, int nmis, int nrec, float syn_factor,
                                                               float dt, double *__restrict__ nbr)
{
    constexpr int NG = K * (K + 1) / 2, NN = NG + K + 1;
    __shared__ double part[kThreads / 64][NN];
    const int r = (int)blockIdx.x, g = (int)blockIdx.y, tid = (int)threadIdx.x;
    const RecvDev rd = recv[r];
    if (!rd.enabled) return;
    const bool unit = (syn_factor == 1.f);
    const float *__restrict__ src0 = proc + (size_t)g * K * syn_stride;
    double acc[NN];
#pragma unroll
    for (int p = 0; p < NN; p++) acc[p] = 0.0;
    for (int k = 0; k < rd.ncomp; k++) {
        const int slot = rd.slot0 + k;
        const CompDev cd = comps[slot];
        const float *__restrict__ sy = src0 + cd.synofs + cd.halo;
        const float *__restrict__ dp = (cd.has_filter && pairs) ? reffilt + pairs[(size_t)g * K * nmis + slot].filtofs : reft + cd.refofs;
        for (int i = tid; i < cd.wlen; i += kThreads) {
            double s[K];
#pragma unroll
            for (int a = 0; a < K; a++) {
                const float v = sy[(size_t)a * syn_stride + i];
                s[a] = (double)(unit ? v : syn_factor * v);
            }
            const double dv = (double)dp[i];
            int p = 0;
#pragma unroll
            for (int a = 0; a < K; a++)
#pragma unroll
                for (int b = a; b < K; b++, p++) acc[p] = acc[p] + s[a] * s[b];
#pragma unroll
            for (int a = 0; a < K; a++) acc[NG + a] = acc[NG + a] + s[a] * dv;
            acc[NN - 1] = acc[NN - 1] + dv * dv;
        }
    }
    const int lane = tid & 63, wave = tid >> 6;
#pragma unroll
    for (int p = 0; p < NN; p++) {
        double v = acc[p];
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) v = v + __shfl_down(v, off, 64);
        if (lane == 0) part[wave][p] = v;
    }
    __syncthreads();
    if (tid < NN) {
        const double t = (part[0][tid] + part[1][tid]) + (part[2][tid] + part[3][tid]);
        nbr[((size_t)g * nrec + r) * NN + tid] = (double)dt * t;
    }
}

// The solve of linfit_solve_kernel (header comment) on sums laid out as G upper triangle by rows, then b: 0 and x, or 1 (a diagonal
// element not positive, or a pivot <= K 2^-52) and NaN in x.  pmin: the smallest pivot up to and including the one that broke down
template <int K, int M>
__device__ __forceinline__ int scaled_cholesky(const double (&N)[M], double (&x)[K], double &pmin)
{
    constexpr int NG = K * (K + 1) / 2;
    const double nan = __longlong_as_double(0x7ff8000000000000LL);
    int st = 0;
    pmin = 0.0;
#pragma unroll
    for (int i = 0; i < K; i++) x[i] = nan;
    bool diag_ok = true;
#pragma unroll
    for (int i = 0; i < K; i++) if (!(N[tri(K, i, i)] > 0.0)) diag_ok = false;
    if (!diag_ok) {
        st = 1;
    } else {
        double s[K], L[K][K];
#pragma unroll
        for (int i = 0; i < K; i++) s[i] = 1.0 / sqrt(N[tri(K, i, i)]);
        const double tol = (double)K * 2.220446049250313e-16;       // K 2^-52
        bool ok = true;
        pmin = 1.0;
#pragma unroll
        for (int j = 0; j < K; j++) {
            double d = 1.0;
#pragma unroll
            for (int k = 0; k < j; k++) d = d - L[j][k] * L[j][k];
            if (ok) {
                if (d < pmin) pmin = d;
                if (!(d > tol)) ok = false;
            }
            const double ljj = sqrt(d);
            L[j][j] = ljj;
#pragma unroll
            for (int i = j + 1; i < K; i++) {
                double v = (N[tri(K, j, i)] * s[i]) * s[j];
#pragma unroll
                for (int k = 0; k < j; k++) v = v - L[i][k] * L[j][k];
                L[i][j] = v / ljj;
            }
        }
        if (!ok) {
            st = 1;
        } else {
            double y[K];
#pragma unroll
            for (int i = 0; i < K; i++) {
                double v = N[NG + i] * s[i];
#pragma unroll
                for (int k = 0; k < i; k++) v = v - L[i][k] * y[k];
                y[i] = v / L[i][i];
            }
#pragma unroll
            for (int i = K - 1; i >= 0; i--) {
                double v = y[i];
#pragma unroll
                for (int k = i + 1; k < K; k++) v = v - L[k][i] * y[k];
                y[i] = v / L[i][i];                                   // (y becomes z in place: z_k, k > i, are final)
            }
#pragma unroll
            for (int i = 0; i < K; i++) x[i] = y[i] * s[i];
        }
    }
    return st;
}

// w: [nrec] receiver weights with zeros for disabled receivers.  normal: [ng][NN] or null
template <int K>
__global__ __launch_bounds__(64) void linfit_solve_kernel(const double *__restrict__ nbr, const double *__restrict__ w, int nrec,
                                                          int anarchy, int ng, double *__restrict__ coef, double *__restrict__ misfit,
                                                          int *__restrict__ status, double *__restrict__ pivot_min,
                                                          double *__restrict__ normal)
{
    constexpr int NG = K * (K + 1) / 2, NN = NG + K + 1;
    const int g = (int)(blockIdx.x * 64 + threadIdx.x);
    if (g >= ng) return;
    double N[NN];
#pragma unroll
    for (int p = 0; p < NN; p++) N[p] = 0.0;
    for (int r = 0; r < nrec; r++) {
        double wr = w[r];
        if (wr == 0.0) continue;
        const double *__restrict__ q = nbr + ((size_t)g * nrec + r) * NN;
        if (anarchy) {
            const double Rr = q[NN - 1];
            wr = Rr > 0.0 ? wr / sqrt(Rr) : 0.0;
            if (wr == 0.0) continue;
        }
        const double w2 = wr * wr;
#pragma unroll
        for (int p = 0; p < NN; p++) N[p] = N[p] + w2 * q[p];
    }
    if (normal)
#pragma unroll
        for (int p = 0; p < NN; p++) normal[(size_t)g * NN + p] = N[p];
    const double R = N[NN - 1];
    const double nan = __longlong_as_double(0x7ff8000000000000LL);
    double pmin;
    double x[K];
    int st = scaled_cholesky<K>(N, x, pmin);
    if (!(R > 0.0)) st = 1;
    double mf = nan;
    if (st == 0) {
        double xb = 0.0, xgx = 0.0;
#pragma unroll
        for (int i = 0; i < K; i++) xb = xb + x[i] * N[NG + i];
#pragma unroll
        for (int i = 0; i < K; i++) {
            double row = 0.0;
#pragma unroll
            for (int j = 0; j < K; j++) row = row + N[i <= j ? tri(K, i, j) : tri(K, j, i)] * x[j];
            xgx = xgx + x[i] * row;
        }
        double val = (R - 2.0 * xb) + xgx;
        val = val > 0.0 ? val : 0.0;
        mf = sqrt(val / R);
    }
#pragma unroll
    for (int i = 0; i < K; i++) coef[(size_t)g * K + i] = st == 0 ? x[i] : nan;
    misfit[g] = mf;
    status[g] = st;
    pivot_min[g] = pmin;
}

} // namespace linfit

// A host build of the kernels above (tests/host_kernels) stops here: what follows launches them from a kiwi_hip_ctx
#ifndef KIWI_LINFIT_KERNELS_ONLY
namespace linfit {

template <int K>
static void launch_gram(kiwi_hip_ctx *c, int ng, const FftPair *pairs, double *nbr)
{
    const int nrec = (int)c->recv.size();
    hipLaunchKernelGGL(linfit_gram_kernel<K>, dim3((unsigned)nrec, (unsigned)ng), dim3(kThreads), 0, c->stream, c->proc_d.p, c->syn_stride,
                       c->recv_d.p, c->comps_d.p, c->reft_d.p, c->reffilt_d.p, pairs, c->nmis, nrec, c->syn_factor, c->gm.dt, nbr);
    HIPCHECK(hipGetLastError());
}

// the Gram kernel alone (the wide fit's for K <= 8: kiwi_linfit_wide.hpp)
static void launch_gram_any(kiwi_hip_ctx *c, int K, int ng, const FftPair *pairs, double *nbr)
{
    by_basis(K, [&](auto k) { launch_gram<k.value>(c, ng, pairs, nbr); });
}

template <int K>
static void launch(kiwi_hip_ctx *c, int ng, const FftPair *pairs, const double *w_d, int anarchy, double *nbr, double *coef,
                   double *misfit, int *status, double *pivot, double *normal)
{
    const int nrec = (int)c->recv.size();
    launch_gram<K>(c, ng, pairs, nbr);
    hipLaunchKernelGGL(linfit_solve_kernel<K>, dim3((unsigned)((ng + 63) / 64)), dim3(64), 0, c->stream, nbr, w_d, nrec, anarchy, ng, coef,
                       misfit, status, pivot, normal);
    HIPCHECK(hipGetLastError());
}

static void launch_any(kiwi_hip_ctx *c, int K, int ng, const FftPair *pairs, const double *w_d, int anarchy, double *nbr, double *coef,
                       double *misfit, int *status, double *pivot, double *normal)
{
    by_basis(K, [&](auto k) { launch<k.value>(c, ng, pairs, w_d, anarchy, nbr, coef, misfit, status, pivot, normal); });
}

// host arrays of the caller, each for the groups of ONE call of run(); any of pivot_min, normal, by_receiver, trace may be null
// (trace: [group][trace_rows][2], the iterations of a robust fit)
struct Out {
    double *coef, *misfit;
    int *status;
    double *pivot_min, *normal, *by_receiver, *trace;
    int trace_rows;
    int *npositive, *nsolves;                       // the wide fit's (kiwi_linfit_wide.hpp), else null
    Out at(int g, int K, int nrec) const
    {
        const size_t nn = (size_t)nn_of(K);
        return Out{ coef + (size_t)g * K, misfit + g, status + g, pivot_min ? pivot_min + g : nullptr,
                    normal ? normal + (size_t)g * nn : nullptr, by_receiver ? by_receiver + (size_t)g * nrec * nn : nullptr,
                    trace ? trace + (size_t)g * trace_rows * 2 : nullptr, trace_rows, npositive ? npositive + g : nullptr,
                    nsolves ? nsolves + g : nullptr };
    }
};

// the reweighting passes behind the l2 solve (kiwi_linfit_robust.hpp); mode 1: A (inner l1norm), 2: B (inner l2norm)
struct Robust { int mode; int niter; double eps; };
static void robust_launch_any(kiwi_hip_ctx *c, int K, int ng, const FftPair *pairs, const double *w_d, int anarchy, const double *nbr,
                              const Robust &rb, double *wbr, double *x, double *misfit, int *status, double *trace);

// the wide fit (kiwi_linfit_wide.hpp) in place of the l2 kernels: up to 64 basis sources, a penalty [K (K + 1) / 2] (host
// pointer, or null), non-negative coefficients
struct Wide { int nonneg; const double *penalty; int relative; };
constexpr int kWideMaxBasis = 64;
static void wide_launch(kiwi_hip_ctx *c, int K, int ng, const FftPair *pairs, const double *w_d, int anarchy, const Wide &wd,
                        const double *penalty_d, double *nbr, double *coef, double *misfit, int *status, double *pivot, int *npos,
                        int *nsol, double *normal, hipEvent_t between);

// the misfits of given coefficient vectors behind the l2 kernels (kiwi_linfit_candidates.hpp): x [ncand][K] (host), shared by all
// groups; outer_norm 1 l1norm, 2 l2norm; free_scale: a candidate is a direction, its best scale is found (l2norm only).  Host
// arrays for the groups of ONE call of run(): best_index, best_misfit, status [group]; misfit, scale [group][ncand],
// receiver_misfit [group][ncand][nrec], receiver_norm [group][nrec], each of the four may be null
struct Candidates {
    const double *x; int ncand, outer_norm, free_scale;
    int *best_index; double *best_misfit; int *status;
    double *misfit, *scale;
    float *receiver_misfit, *receiver_norm;
    Candidates at(int g, int nrec) const
    {
        Candidates c = *this;
        c.best_index += g; c.best_misfit += g; c.status += g;
        if (misfit) c.misfit += (size_t)g * ncand;
        if (scale) c.scale += (size_t)g * ncand;
        if (receiver_misfit) c.receiver_misfit += (size_t)g * ncand * nrec;
        if (receiver_norm) c.receiver_norm += (size_t)g * nrec;
        return c;
    }
};
static void check_candidates(const Candidates &cd, int K);

} // namespace linfit

// The one implementation of the candidate evaluation (kiwi_linfit_candidates_timescan.hpp) evaluates the candidates at nk origin
// times per group; run() below hands it the plain call as nk = 1 without the arrays that only a scan has.
namespace linfit_candidates_timescan {

// host arrays of the caller for the groups of ONE call of run(): best_offset, status [group]; best_index, best_misfit, best_scale
// [group][nk]; cand_misfit, cand_offset, cand_scale [group][ncand]; misfit, scale [group][nk][ncand]; receiver_misfit
// [group][nk][ncand][nrec]; receiver_norm [group][nrec].  x [ncand][K] is shared by all groups and offsets.  best_scale and
// everything after it may be null; best_offset is null in the plain call and only there
struct Scan {
    const double *x; int ncand, outer_norm, free_scale;
    int *best_offset, *best_index; double *best_misfit, *best_scale; int *status;
    double *cand_misfit; int *cand_offset; double *cand_scale;
    double *misfit, *scale;
    float *receiver_misfit, *receiver_norm;
    Scan at(size_t g, size_t nk, size_t nrec) const
    {
        Scan s = *this;
        const size_t nc = (size_t)ncand;
        s.status += g; s.best_index += g * nk; s.best_misfit += g * nk;
        if (best_offset) s.best_offset += g;
        if (best_scale) s.best_scale += g * nk;
        if (cand_misfit) s.cand_misfit += g * nc;
        if (cand_offset) s.cand_offset += g * nc;
        if (cand_scale) s.cand_scale += g * nc;
        if (misfit) s.misfit += g * nk * nc;
        if (scale) s.scale += g * nk * nc;
        if (receiver_misfit) s.receiver_misfit += g * nk * nc * nrec;
        if (receiver_norm) s.receiver_norm += g * nrec;
        return s;
    }
    bool scaled() const { return free_scale && (scale || receiver_misfit); }        // the scales are kept on the device
};

// the plain call's arrays as those of a scan of one offset: the layouts coincide at nk = 1
static Scan plain(const linfit::Candidates &cd)
{
    return Scan{ cd.x, cd.ncand, cd.outer_norm, cd.free_scale, nullptr, cd.best_index, cd.best_misfit, nullptr, cd.status,
                 nullptr, nullptr, nullptr, cd.misfit, cd.scale, cd.receiver_misfit, cd.receiver_norm };
}

// device buffers of the candidate kernels, kept over the chunks of one run
struct Bufs {
    DevBuf<double> x, misfit, scale, tile_v, best_misfit, best_scale, cand_misfit, cand_scale;
    DevBuf<float> rmis, rnorm;
    DevBuf<int> tile_i, best_index, best_offset, status, cand_offset;
};

static size_t bytes_per_group(const Scan &sc, int nrec, int nk);
static void chunk(kiwi_hip_ctx *c, int K, int g0, int ng, int nk, const double *w_d, int anarchy, const double *nbr, const double *normal,
                  const Scan &sc, Bufs &b, hipEvent_t after_kernels);
static void fill_failed(size_t ngroup, size_t nk, size_t nrec, const Scan &sc);

} // namespace linfit_candidates_timescan

namespace linfit {

// what the fit cannot do is refused, nothing approximated.  Leaves the context prepared.  floating_l2: the caller evaluates GIVEN
// coefficient vectors under floating_l2norm (kiwi_linfit_candidates_floating.hpp) and fits nothing: that method, and only it, passes
static void check_setup(kiwi_hip_ctx *c, int K, const Out &out, const Robust *rb = nullptr, const Wide *wd = nullptr, bool floating_l2 = false)
{
    const int kmax = wd ? kWideMaxBasis : kMaxBasis;
    if (K < 1 || K > kmax)
        throw std::runtime_error("linear_fit: K = " + std::to_string(K) + " basis sources per group; 1 to " + std::to_string(kmax) + " are supported");
    if (wd) {
        if (wd->nonneg != 0 && wd->nonneg != 1) throw std::runtime_error("linear_fit_wide: nonneg = " + std::to_string(wd->nonneg) + " must be 0 or 1");
        if (wd->penalty)
            for (int p = 0; p < K * (K + 1) / 2; p++)
                if (!std::isfinite(wd->penalty[p])) throw std::runtime_error("linear_fit_wide: penalty entry " + std::to_string(p) + " is not finite");
    }
    if (!out.coef || !out.misfit || !out.status) throw std::runtime_error("linear_fit: null coef, misfit or status array");
    const bool floating_ok = floating_l2 && c->method == KIWI_FLOATING_L2NORM;
    if ((c->method == KIWI_FLOATING_L2NORM || c->method == KIWI_FLOATING_L1NORM) && !floating_ok)
        throw std::runtime_error("linear_fit: floating shift ranges make the misfit a minimum over shifts, which is not quadratic in the coefficients; set l2norm");
    if (c->method != KIWI_L2NORM && !(rb && rb->mode == 1 && c->method == KIWI_L1NORM) && !floating_ok)
        throw std::runtime_error("linear_fit: the misfit method must be l2norm (the only inner norm that is quadratic in the coefficients)");
    prepare(c);
    if (c->synth_only) throw std::runtime_error("linear_fit: every enabled receiver component needs a reference seismogram");
    if (c->any_untapered)
        throw std::runtime_error("linear_fit: an enabled receiver has no misfit taper (its comparison span follows the source, so the basis traces have no common span)");
}

// the groups [isrc0, isrc0 + ngroup K) of the uploaded batch; adds its HIP-event times to c->linfit_ms.  rb: the reweighting
// passes of a robust fit behind the l2 solve of every chunk, or null.  wd: the wide fit in place of the l2 kernels, or null.
// cd: candidate coefficient vectors evaluated behind the l2 kernels of every chunk, or null
static void run(kiwi_hip_ctx *c, int isrc0, int ngroup, int K, const double *receiver_weight, int anarchy, const Out &out,
                const Robust *rb = nullptr, const Wide *wd = nullptr, const Candidates *cd = nullptr)
{
    if (cd) check_candidates(*cd, K);
    check_setup(c, K, out, rb, wd);
    check_group_range("linear_fit", c, isrc0, ngroup, K);
    if (ngroup == 0) return;
    const int nrec = (int)c->recv.size(), NN = nn_of(K);
    const LibraryTransforms library_transforms(c);      // (a misfit filter: the kept traces through the library transforms)
    c->misfit_d.ensure((size_t)c->nsrc * c->nmis, &c->dev_bytes);
    c->global_d.ensure((size_t)c->nsrc, &c->dev_bytes);
    if (c->fft_needed && !c->fft_ready) prepare_fft(c, c->reft_h);
    const int proc_which = c->any_filter ? 3 : 2;
    c->fuse_now = can_fuse(c, proc_which, isrc0, ngroup * K);
    if (c->fft_needed && c->fft_cap < K) throw std::runtime_error("linear_fit: the transform workspace (KIWI_HIP_CHUNK_MB) does not hold one group");

    const std::vector<double> w = receiver_weights(c, receiver_weight);
    DevBuf<double> w_d, nbr_d, coef_d, mis_d, piv_d, normal_d, wbr_d, trace_d;
    const size_t trace_len = rb ? (size_t)(rb->niter + 1) * 2 : 0;
    DevBuf<int> st_d, npos_d, nsol_d;
    DevBuf<double> penalty_d;
    const linfit_candidates_timescan::Scan scan = cd ? linfit_candidates_timescan::plain(*cd) : linfit_candidates_timescan::Scan{};
    linfit_candidates_timescan::Bufs cand;
    w_d.alloc((size_t)nrec, &c->dev_bytes);
    HIPCHECK(hipMemcpyAsync(w_d.p, w.data(), (size_t)nrec * sizeof(double), hipMemcpyHostToDevice, c->stream));
    if (wd && wd->penalty) {
        penalty_d.alloc((size_t)(K * (K + 1) / 2), &c->dev_bytes);
        HIPCHECK(hipMemcpyAsync(penalty_d.p, wd->penalty, (size_t)(K * (K + 1) / 2) * sizeof(double), hipMemcpyHostToDevice, c->stream));
    }
    HIPCHECK(hipStreamSynchronize(c->stream));

    const PooledEvents<6> ev(c);                           // (ev[5]: between the Gram and the solve kernels of the wide fit)
    std::vector<double> piv_h;
    // per group: the sums by receiver, the reweighted sums of a robust fit of mode 1 beside them, the candidate outputs
    const size_t per_group = (size_t)nrec * (NN + (rb && rb->mode == 1 ? NN + 2 : 0)) * sizeof(double) + (cd ? linfit_candidates_timescan::bytes_per_group(scan, nrec, 1) : 0);
    int g0 = 0;
    while (g0 < ngroup) {
        const int ng = next_group_chunk(c, isrc0, g0, ngroup, K, 2, per_group, c->fft_needed ? c->fft_cap : kNoSourceCap);
        const int s0 = isrc0 + g0 * K;
        HIPCHECK(hipEventRecord(ev[0], c->stream));
        run_chunk(c, s0, ng * K, proc_which);
        HIPCHECK(hipEventRecord(ev[1], c->stream));
        nbr_d.ensure((size_t)ng * nrec * NN, &c->dev_bytes);
        coef_d.ensure((size_t)ng * K, &c->dev_bytes); mis_d.ensure((size_t)ng, &c->dev_bytes); piv_d.ensure((size_t)ng, &c->dev_bytes);
        st_d.ensure((size_t)ng, &c->dev_bytes);
        if (out.normal || cd) normal_d.ensure((size_t)ng * NN, &c->dev_bytes);
        HIPCHECK(hipMemsetAsync(nbr_d.p, 0, (size_t)ng * nrec * NN * sizeof(double), c->stream));
        if (wd) {
            npos_d.ensure((size_t)ng, &c->dev_bytes); nsol_d.ensure((size_t)ng, &c->dev_bytes);
            wide_launch(c, K, ng, c->fft_needed ? c->pairs_d.p : (const FftPair *)nullptr, w_d.p, anarchy ? 1 : 0, *wd, penalty_d.p, nbr_d.p,
                        coef_d.p, mis_d.p, st_d.p, piv_d.p, npos_d.p, nsol_d.p, out.normal ? normal_d.p : (double *)nullptr, ev[5]);
        } else
            launch_any(c, K, ng, c->fft_needed ? c->pairs_d.p : (const FftPair *)nullptr, w_d.p, anarchy ? 1 : 0, nbr_d.p, coef_d.p, mis_d.p,
                       st_d.p, piv_d.p, out.normal || cd ? normal_d.p : (double *)nullptr);
        HIPCHECK(hipEventRecord(ev[2], c->stream));
        if (rb) {
            if (rb->mode == 1) wbr_d.ensure((size_t)ng * nrec * (NN + 2), &c->dev_bytes);
            trace_d.ensure((size_t)ng * trace_len, &c->dev_bytes);
            robust_launch_any(c, K, ng, c->fft_needed ? c->pairs_d.p : (const FftPair *)nullptr, w_d.p, anarchy ? 1 : 0, nbr_d.p, *rb, wbr_d.p,
                              coef_d.p, mis_d.p, st_d.p, trace_d.p);
        }
        if (cd)                                                // (the downloads of the candidates' results are queued behind ev[3])
            linfit_candidates_timescan::chunk(c, K, g0, ng, 1, w_d.p, anarchy ? 1 : 0, nbr_d.p, normal_d.p, scan, cand, ev[3]);
        else HIPCHECK(hipEventRecord(ev[3], c->stream));
        piv_h.resize((size_t)ng);
        HIPCHECK(hipMemcpyAsync(out.coef + (size_t)g0 * K, coef_d.p, (size_t)ng * K * sizeof(double), hipMemcpyDeviceToHost, c->stream));
        HIPCHECK(hipMemcpyAsync(out.misfit + g0, mis_d.p, (size_t)ng * sizeof(double), hipMemcpyDeviceToHost, c->stream));
        HIPCHECK(hipMemcpyAsync(out.status + g0, st_d.p, (size_t)ng * sizeof(int), hipMemcpyDeviceToHost, c->stream));
        HIPCHECK(hipMemcpyAsync(out.pivot_min ? out.pivot_min + g0 : piv_h.data(), piv_d.p, (size_t)ng * sizeof(double), hipMemcpyDeviceToHost, c->stream));
        if (out.normal)
            HIPCHECK(hipMemcpyAsync(out.normal + (size_t)g0 * NN, normal_d.p, (size_t)ng * NN * sizeof(double), hipMemcpyDeviceToHost, c->stream));
        if (out.by_receiver)
            HIPCHECK(hipMemcpyAsync(out.by_receiver + (size_t)g0 * nrec * NN, nbr_d.p, (size_t)ng * nrec * NN * sizeof(double), hipMemcpyDeviceToHost, c->stream));
        if (wd && out.npositive)
            HIPCHECK(hipMemcpyAsync(out.npositive + g0, npos_d.p, (size_t)ng * sizeof(int), hipMemcpyDeviceToHost, c->stream));
        if (wd && out.nsolves)
            HIPCHECK(hipMemcpyAsync(out.nsolves + g0, nsol_d.p, (size_t)ng * sizeof(int), hipMemcpyDeviceToHost, c->stream));
        if (rb && out.trace)
            HIPCHECK(hipMemcpyAsync(out.trace + (size_t)g0 * trace_len, trace_d.p, (size_t)ng * trace_len * sizeof(double), hipMemcpyDeviceToHost, c->stream));
        HIPCHECK(hipEventRecord(ev[4], c->stream));
        HIPCHECK(hipStreamSynchronize(c->stream));
        for (int i = 0; i < 4; i++) ev.add_elapsed(c->linfit_ms, i, i, i + 1);
        if (wd) {
            ev.add_elapsed(c->linfit_wide_ms, 0, 1, 5);
            ev.add_elapsed(c->linfit_wide_ms, 1, 5, 2);
        }
        g0 += ng;
    }
    leave_evaluated(c, isrc0, ngroup * K, proc_which);
    // a basis source that failed to discretise: no fit for its group
    const double nan = std::numeric_limits<double>::quiet_NaN();
    for_each_failed_group(c, isrc0, ngroup, K, [&](int g) {
        out.status[g] = 2;
        out.misfit[g] = nan;
        for (int i = 0; i < K; i++) out.coef[(size_t)g * K + i] = nan;
        if (out.trace) std::fill(out.trace + (size_t)g * out.trace_rows * 2, out.trace + (size_t)(g + 1) * out.trace_rows * 2, nan);
        if (out.npositive) out.npositive[g] = 0;
        if (out.nsolves) out.nsolves[g] = 0;
        if (cd) linfit_candidates_timescan::fill_failed(1, 1, (size_t)nrec, scan.at((size_t)g, 1, (size_t)nrec));
    });
}

// groups whose basis sources could not be discretised at all (nothing was uploaded for them): status 2, NaN, zero sums
static void fill_failed(int ngroup, int K, int nrec, const Out &out)
{
    const double nan = std::numeric_limits<double>::quiet_NaN();
    const size_t nn = (size_t)nn_of(K);
    for (int g = 0; g < ngroup; g++) {
        out.status[g] = 2; out.misfit[g] = nan;
        for (int i = 0; i < K; i++) out.coef[(size_t)g * K + i] = nan;
        if (out.pivot_min) out.pivot_min[g] = 0.0;
        if (out.npositive) out.npositive[g] = 0;
        if (out.nsolves) out.nsolves[g] = 0;
    }
    if (out.trace) std::fill(out.trace, out.trace + (size_t)ngroup * out.trace_rows * 2, nan);
    if (out.normal) std::memset(out.normal, 0, (size_t)ngroup * nn * sizeof(double));
    if (out.by_receiver) std::memset(out.by_receiver, 0, (size_t)ngroup * nrec * nn * sizeof(double));
}

// kiwi_hip_linear_fit_params, _robust_params and _wide_params piece by piece (PieceCall, kiwi_group_run.hpp): rb and wd as in run()
static PieceCall piece_call(int K, const double *receiver_weight, int anarchy, const Out &out, const Robust *rb = nullptr, const Wide *wd = nullptr)
{
    return PieceCall{ K,
        [=](kiwi_hip_ctx *c) { check_setup(c, K, out, rb, wd); },
        [=](kiwi_hip_ctx *c, int s0, int n) { fill_failed(n / K, K, (int)c->recv.size(), out.at(s0 / K, K, (int)c->recv.size())); },
        [=](kiwi_hip_ctx *c, int s0, int n) { run(c, 0, n / K, K, receiver_weight, anarchy, out.at(s0 / K, K, (int)c->recv.size()), rb, wd); } };
}

} // namespace linfit
#endif // KIWI_LINFIT_KERNELS_ONLY
