// kiwi_linfit_candidates.hpp -- misfits of many GIVEN coefficient vectors per group from the normal equations kiwi_linfit.hpp keeps
// on the device: the synthetics are linear in the coefficients, so a candidate x (a trial double couple as a combination of the six
// elementary tensors, kiwi_amd/mtfit.py) needs no synthesis of its own.  Included by kiwi_hip.hip after the other linfit headers,
// under the same -ffp-contract=off: every fp64 operation below is rounded on its own, and tests/linfit_candidates_restatement.py
// restates each in the same order (the GPU tests ask for bit identity).  Notation as in kiwi_linfit.hpp and kiwi_linfit_robust.hpp:
// N_r = (G_r, b_r, R_r) the sums of receiver r from linfit_gram_kernel, N = (G, b, R) their fold by linfit_solve_kernel (weights,
// anarchy), w_r = receiver_weight[r] (0 for a disabled receiver).
//
//   candidates  one workgroup of kCandThreads lanes per (group, tile of kCandThreads candidates); a lane owns ONE candidate with
//               its x in registers.  The rows N_r are staged in LDS, kCandStage receivers at a time; every lane reads the same
//               address at the same time (a broadcast), receivers ascending, into the candidate's own accumulators: the result does
//               not depend on the tiling.  Per row q = (G, b, R) and vector x, `quad`:
//                   xb = 0; xb = xb + x_i b_i;  row_i = 0; row_i = row_i + G_ij x_j (j ascending);  xgx = 0; xgx = xgx + x_i row_i
//               -- the sums linfit_solve_kernel and robust_receiver_kernel form --, then val = (R - 2 xb) + xgx, clamped at 0.
//     pass 0    outer l1norm, rows N_r.  A receiver with w_r == 0 or not R_r > 0 is skipped.  m = sqrt(val); n = sqrt(R_r);
//               v = anarchy ? w_r / n : w_r;  L = L + v m;  D = D + v n;  misfit = L / D (NaN where no receiver counts);
//               receiver_misfit[g][c][r] = (float) m.  This is iterate 0 of robust_receiver_kernel at a fixed x.
//     pass 1    outer l2norm, the folded row N as the only "receiver": misfit = sqrt(val / R), NaN unless R > 0.
//               free_scale: the candidate is a direction u; quad(N, u) gives u.b and u.G.u; a = (u.b) / (u.G.u), NaN (and a NaN
//               misfit) unless u.G.u > 0; x_i = a u_i; then as above.  scale[g][c] = a.
//     pass 2    outer l2norm, receiver_misfit only: rows N_r, x (free_scale: x_i = scale[g][c] u_i, the product of pass 1) and
//               (float) m per counted receiver as in pass 0; NaN for a candidate whose scale is NaN.
//               Every lane keeps the best (misfit, index) it has; wavefront and workgroup fold it in the order below.
//   fold        one wavefront per group: the tiles' bests folded in the same order; status and receiver_norm[g][r] = (float)
//               sqrt(R_r) of the receivers that count (0 otherwise).
// The order of "best" is total -- a NaN misfit never wins, then the smaller value, then the LOWER candidate index --, so the
// answer does not depend on tile shape or chunking.  No atomics.
// Status of a group: 0 evaluated; 1 no data (l2norm: R not positive; l1norm: no receiver counts): NaN, best_index -1; 2 a basis
// source failed to discretise (set on the host).  A group whose candidates are all NaN has best_index -1.

namespace linfit {

constexpr int kCandThreads = 256;                   // candidates per workgroup
constexpr int kCandStage = 64;                      // receivers per LDS stage: 64 x NN x 8 bytes = 22.5 KiB at K = 8

// xb = x.b and xgx = x.G.x of the row q, summed as linfit_solve_kernel sums them for its misfit
template <int K>
__device__ __forceinline__ void quad(const double *q, const double (&x)[K], double &xb, double &xgx)
{
    constexpr int NG = K * (K + 1) / 2;
    xb = 0.0; xgx = 0.0;
#pragma unroll
    for (int i = 0; i < K; i++) xb = xb + x[i] * q[NG + i];
#pragma unroll
    for (int i = 0; i < K; i++) {
        double row = 0.0;
#pragma unroll
        for (int j = 0; j < K; j++) row = row + q[i <= j ? tri(K, i, j) : tri(K, j, i)] * x[j];
        xgx = xgx + x[i] * row;
    }
}

// (v, i) becomes (v2, i2) where that is the better one; i < 0: none
__device__ __forceinline__ void take_better(double &v, int &i, double v2, int i2)
{
    if (i2 >= 0 && (i < 0 || v2 < v || (v2 == v && i2 < i))) { v = v2; i = i2; }
}

__device__ __forceinline__ void wave_best(double &v, int &i)
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const double v2 = __shfl_down(v, off, 64);
        const int i2 = __shfl_down(i, off, 64);
        take_better(v, i, v2, i2);
    }
}

// rows: [group][nrows][NN] (pass 0, 2: nbr with nrows = nrec; pass 1: normal with nrows = 1).  w: [nrows] (pass 1: null).
// x: [ncand][K].  misfit, scale: [group][ncand] or null.  rmis: [group][ncand][nrows] or null, zeroed before the launch.
// tile_v, tile_i: [group][gridDim.x] (pass 2: not written).  blockIdx.x = tile of candidates, blockIdx.y = group
template <int K>
__global__ __launch_bounds__(kCandThreads) void linfit_candidates_kernel(const double *__restrict__ rows, int nrows,
                                                                         const double *__restrict__ w, int anarchy, int pass,
                                                                         int free_scale, const double *__restrict__ x, int ncand,
                                                                         double *__restrict__ misfit, double *__restrict__ scale,
                                                                         float *__restrict__ rmis, double *__restrict__ tile_v,
                                                                         int *__restrict__ tile_i)
{
    constexpr int NN = K * (K + 1) / 2 + K + 1;
    __shared__ double sq[kCandStage * NN];
    __shared__ double sw[kCandStage];
    __shared__ double best_v[kCandThreads / 64];
    __shared__ int best_i[kCandThreads / 64];
    const int g = (int)blockIdx.y, tid = (int)threadIdx.x;
    const int cand = (int)blockIdx.x * kCandThreads + tid;
    const bool live = cand < ncand;
    const size_t slot = (size_t)g * ncand + (live ? cand : 0);
    const double nan = __longlong_as_double(0x7ff8000000000000LL);
    double xc[K];
#pragma unroll
    for (int i = 0; i < K; i++) xc[i] = live ? x[(size_t)cand * K + i] : 0.0;
    double a = pass == 1 && free_scale ? nan : 1.0;
    if (pass == 2 && free_scale) {
        a = scale[slot];
#pragma unroll
        for (int i = 0; i < K; i++) xc[i] = a * xc[i];
    }
    double Ls = 0.0, Ds = 0.0, mf = nan;
    bool counted = false;
    for (int r0 = 0; r0 < nrows; r0 += kCandStage) {
        const int nr = nrows - r0 < kCandStage ? nrows - r0 : kCandStage;
        if (r0 > 0) __syncthreads();
        const double *__restrict__ src = rows + ((size_t)g * nrows + r0) * NN;
        for (int p = tid; p < nr * NN; p += kCandThreads) sq[p] = src[p];
        if (tid < nr) sw[tid] = w ? w[r0 + tid] : 1.0;
        __syncthreads();
        for (int r = 0; r < nr; r++) {
            const double wr = sw[r];
            if (wr == 0.0) continue;
            const double *q = sq + r * NN;
            const double Rr = q[NN - 1];
            if (!(Rr > 0.0)) continue;
            double xb, xgx;
            quad<K>(q, xc, xb, xgx);
            bool ok = true;
            if (pass == 1 && free_scale) {
                ok = xgx > 0.0;
                a = ok ? xb / xgx : nan;
                double xs[K];
#pragma unroll
                for (int i = 0; i < K; i++) xs[i] = a * xc[i];
                quad<K>(q, xs, xb, xgx);
            }
            double val = (Rr - 2.0 * xb) + xgx;
            val = val > 0.0 ? val : 0.0;
            if (pass == 1) {
                mf = ok ? sqrt(val / Rr) : nan;
            } else {
                const double m = sqrt(val), n = sqrt(Rr);
                const double v = anarchy ? wr / n : wr;
                Ls = Ls + v * m;
                Ds = Ds + v * n;
                counted = true;
                if (rmis && live) rmis[slot * nrows + r0 + r] = a == a ? (float)m : __int_as_float(0x7fc00000);
            }
        }
    }
    if (pass == 2) return;
    if (pass == 0) mf = counted ? Ls / Ds : nan;
    if (live) {
        if (misfit) misfit[slot] = mf;
        if (scale) scale[slot] = a;
    }
    double bv = mf;
    int bi = (live && mf == mf) ? cand : -1;
    wave_best(bv, bi);
    if ((tid & 63) == 0) { best_v[tid >> 6] = bv; best_i[tid >> 6] = bi; }
    __syncthreads();
    if (tid == 0) {
        for (int k = 1; k < kCandThreads / 64; k++) take_better(bv, bi, best_v[k], best_i[k]);
        tile_v[(size_t)g * gridDim.x + blockIdx.x] = bv;
        tile_i[(size_t)g * gridDim.x + blockIdx.x] = bi;
    }
}

// nbr: [group][nrec][NN], normal: [group][NN], w: [nrec].  rnorm: [group][nrec] or null.  blockIdx.x = group
__global__ __launch_bounds__(64) void linfit_candidates_fold_kernel(const double *__restrict__ tile_v, const int *__restrict__ tile_i,
                                                                    int ntile, const double *__restrict__ nbr,
                                                                    const double *__restrict__ normal, const double *__restrict__ w,
                                                                    int nrec, int NN, int outer, int *__restrict__ best_index,
                                                                    double *__restrict__ best_misfit, int *__restrict__ status,
                                                                    float *__restrict__ rnorm)
{
    const int g = (int)blockIdx.x, lane = (int)threadIdx.x;
    double bv = 0.0;
    int bi = -1;
    for (int t = lane; t < ntile; t += 64) take_better(bv, bi, tile_v[(size_t)g * ntile + t], tile_i[(size_t)g * ntile + t]);
    wave_best(bv, bi);
    int counts = 0;
    for (int r = lane; r < nrec; r += 64) {
        const double Rr = nbr[((size_t)g * nrec + r) * NN + NN - 1];
        const bool in = w[r] != 0.0 && Rr > 0.0;
        if (in) counts = 1;
        if (rnorm) rnorm[(size_t)g * nrec + r] = in ? (float)sqrt(Rr) : 0.f;
    }
    const int any = __any(counts);
    if (lane == 0) {
        best_index[g] = bi;
        best_misfit[g] = bi >= 0 ? bv : __longlong_as_double(0x7ff8000000000000LL);
        status[g] = (outer == 2 ? normal[(size_t)g * NN + NN - 1] > 0.0 : any != 0) ? 0 : 1;
    }
}

// what the candidate evaluation cannot do is refused before anything runs
static void check_candidates(const Candidates &cd, int K)
{
    if (cd.ncand < 1) throw std::runtime_error("linear_fit_candidates: ncand = " + std::to_string(cd.ncand) + "; at least one candidate is needed");
    if (!cd.x || !cd.best_index || !cd.best_misfit || !cd.status)
        throw std::runtime_error("linear_fit_candidates: null candidates, best_index, best_misfit or status array");
    if (cd.outer_norm != 1 && cd.outer_norm != 2) throw std::runtime_error("linear_fit_candidates: outer_norm must be 1 (l1norm) or 2 (l2norm)");
    if (cd.free_scale != 0 && cd.free_scale != 1)
        throw std::runtime_error("linear_fit_candidates: free_scale = " + std::to_string(cd.free_scale) + " must be 0 or 1");
    if (cd.free_scale && cd.outer_norm == 1)
        throw std::runtime_error("linear_fit_candidates: free_scale needs the outer l2norm (under l1norm the best scale of a direction has no closed form)");
    if (cd.scale && !cd.free_scale) throw std::runtime_error("linear_fit_candidates: a scale array without free_scale");
    if (K >= 1 && K <= kMaxBasis)
        for (size_t p = 0; p < (size_t)cd.ncand * K; p++)
            if (!std::isfinite(cd.x[p]))
                throw std::runtime_error("linear_fit_candidates: entry " + std::to_string(p % K) + " of candidate " + std::to_string(p / K) + " is not finite");
}

// device bytes of one group's candidate outputs (the chunk of linfit::run is bounded by them too)
static size_t cand_bytes(const Candidates &cd, int nrec)
{
    const size_t ntile = (size_t)(cd.ncand + kCandThreads - 1) / kCandThreads;
    const bool scaled = cd.free_scale && (cd.scale || cd.receiver_misfit);
    return ntile * (sizeof(double) + sizeof(int)) + (size_t)cd.ncand * ((cd.misfit ? sizeof(double) : 0) + (scaled ? sizeof(double) : 0) +
                                                                         (cd.receiver_misfit ? (size_t)nrec * sizeof(float) : 0));
}

// behind the l2 kernels of one chunk: nbr and normal as they left them on the stream
template <int K>
static void cand_launch(kiwi_hip_ctx *c, int ng, const double *w_d, int anarchy, const double *nbr, const double *normal,
                        const Candidates &cd, CandBufs &b)
{
    const int nrec = (int)c->recv.size(), NN = nn_of(K), ntile = (cd.ncand + kCandThreads - 1) / kCandThreads;
    const dim3 grid((unsigned)ntile, (unsigned)ng);
    double *mis = cd.misfit ? b.misfit.p : nullptr, *sc = cd.free_scale && (cd.scale || cd.receiver_misfit) ? b.scale.p : nullptr;
    float *rm = cd.receiver_misfit ? b.rmis.p : nullptr;
    if (rm) HIPCHECK(hipMemsetAsync(rm, 0, (size_t)ng * cd.ncand * nrec * sizeof(float), c->stream));
    if (cd.outer_norm == 1) {
        hipLaunchKernelGGL(linfit_candidates_kernel<K>, grid, dim3(kCandThreads), 0, c->stream, nbr, nrec, w_d, anarchy, 0, 0, b.x.p,
                           cd.ncand, mis, (double *)nullptr, rm, b.tile_v.p, b.tile_i.p);
        HIPCHECK(hipGetLastError());
    } else {
        hipLaunchKernelGGL(linfit_candidates_kernel<K>, grid, dim3(kCandThreads), 0, c->stream, normal, 1, (const double *)nullptr, 0, 1,
                           cd.free_scale, b.x.p, cd.ncand, mis, sc, (float *)nullptr, b.tile_v.p, b.tile_i.p);
        HIPCHECK(hipGetLastError());
        if (rm) {
            hipLaunchKernelGGL(linfit_candidates_kernel<K>, grid, dim3(kCandThreads), 0, c->stream, nbr, nrec, w_d, anarchy, 2,
                               cd.free_scale, b.x.p, cd.ncand, (double *)nullptr, sc, rm, (double *)nullptr, (int *)nullptr);
            HIPCHECK(hipGetLastError());
        }
    }
    hipLaunchKernelGGL(linfit_candidates_fold_kernel, dim3((unsigned)ng), dim3(64), 0, c->stream, b.tile_v.p, b.tile_i.p, ntile, nbr, normal,
                       w_d, nrec, NN, cd.outer_norm, b.best_index.p, b.best_misfit.p, b.status.p, cd.receiver_norm ? b.rnorm.p : (float *)nullptr);
    HIPCHECK(hipGetLastError());
}

// the candidate kernels of one chunk and the downloads of their results for the groups [g0, g0 + ng) of the call
static void cand_chunk(kiwi_hip_ctx *c, int K, int g0, int ng, const double *w_d, int anarchy, const double *nbr, const double *normal,
                       const Candidates &cd, CandBufs &b, hipEvent_t after_kernels)
{
    const int nrec = (int)c->recv.size();
    const size_t ntile = (size_t)(cd.ncand + kCandThreads - 1) / kCandThreads, nc = (size_t)ng * cd.ncand;
    if (!b.x.p) {
        b.x.alloc((size_t)cd.ncand * K, &c->dev_bytes);
        HIPCHECK(hipMemcpyAsync(b.x.p, cd.x, (size_t)cd.ncand * K * sizeof(double), hipMemcpyHostToDevice, c->stream));
    }
    b.tile_v.ensure((size_t)ng * ntile, &c->dev_bytes); b.tile_i.ensure((size_t)ng * ntile, &c->dev_bytes);
    b.best_index.ensure((size_t)ng, &c->dev_bytes); b.best_misfit.ensure((size_t)ng, &c->dev_bytes); b.status.ensure((size_t)ng, &c->dev_bytes);
    if (cd.misfit) b.misfit.ensure(nc, &c->dev_bytes);
    if (cd.free_scale && (cd.scale || cd.receiver_misfit)) b.scale.ensure(nc, &c->dev_bytes);
    if (cd.receiver_misfit) b.rmis.ensure(nc * nrec, &c->dev_bytes);
    if (cd.receiver_norm) b.rnorm.ensure((size_t)ng * nrec, &c->dev_bytes);
    switch (K) {
    case 1: cand_launch<1>(c, ng, w_d, anarchy, nbr, normal, cd, b); break;
    case 2: cand_launch<2>(c, ng, w_d, anarchy, nbr, normal, cd, b); break;
    case 3: cand_launch<3>(c, ng, w_d, anarchy, nbr, normal, cd, b); break;
    case 4: cand_launch<4>(c, ng, w_d, anarchy, nbr, normal, cd, b); break;
    case 5: cand_launch<5>(c, ng, w_d, anarchy, nbr, normal, cd, b); break;
    case 6: cand_launch<6>(c, ng, w_d, anarchy, nbr, normal, cd, b); break;
    case 7: cand_launch<7>(c, ng, w_d, anarchy, nbr, normal, cd, b); break;
    default: cand_launch<8>(c, ng, w_d, anarchy, nbr, normal, cd, b); break;
    }
    HIPCHECK(hipEventRecord(after_kernels, c->stream));
    const Candidates o = cd.at(g0, nrec);
    HIPCHECK(hipMemcpyAsync(o.best_index, b.best_index.p, (size_t)ng * sizeof(int), hipMemcpyDeviceToHost, c->stream));
    HIPCHECK(hipMemcpyAsync(o.best_misfit, b.best_misfit.p, (size_t)ng * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIPCHECK(hipMemcpyAsync(o.status, b.status.p, (size_t)ng * sizeof(int), hipMemcpyDeviceToHost, c->stream));
    if (cd.misfit) HIPCHECK(hipMemcpyAsync(o.misfit, b.misfit.p, nc * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    if (cd.scale) HIPCHECK(hipMemcpyAsync(o.scale, b.scale.p, nc * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    if (cd.receiver_misfit) HIPCHECK(hipMemcpyAsync(o.receiver_misfit, b.rmis.p, nc * nrec * sizeof(float), hipMemcpyDeviceToHost, c->stream));
    if (cd.receiver_norm) HIPCHECK(hipMemcpyAsync(o.receiver_norm, b.rnorm.p, (size_t)ng * nrec * sizeof(float), hipMemcpyDeviceToHost, c->stream));
}

// groups that have no fit (a basis source failed to discretise): status 2, NaN, best_index -1, zeros per receiver
static void cand_fill_failed(int ngroup, int nrec, const Candidates &cd)
{
    const double nan = std::numeric_limits<double>::quiet_NaN();
    for (int g = 0; g < ngroup; g++) { cd.status[g] = 2; cd.best_index[g] = -1; cd.best_misfit[g] = nan; }
    const size_t nc = (size_t)ngroup * cd.ncand;
    if (cd.misfit) std::fill(cd.misfit, cd.misfit + nc, nan);
    if (cd.scale) std::fill(cd.scale, cd.scale + nc, nan);
    if (cd.receiver_misfit) std::fill(cd.receiver_misfit, cd.receiver_misfit + nc * nrec, 0.f);
    if (cd.receiver_norm) std::fill(cd.receiver_norm, cd.receiver_norm + (size_t)ngroup * nrec, 0.f);
}

} // namespace linfit
