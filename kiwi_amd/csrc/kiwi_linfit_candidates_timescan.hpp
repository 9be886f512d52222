// kiwi_linfit_candidates_timescan.hpp -- misfits of many GIVEN coefficient vectors per group from the normal equations the linear
// fit keeps on the device: the synthetics are linear in the coefficients, so a candidate x (a trial double couple as a combination
// of the six elementary tensors, kiwi_amd/mtfit.py) needs no synthesis of its own.  One implementation serves two calls:
// kiwi_hip_linear_fit_candidates_time_scan evaluates the candidates at MANY origin times from ONE synthesis of the basis
// (kiwi_linfit_timescan.hpp's sums per offset), kiwi_hip_linear_fit_candidates is the case of one offset, nk = 1, on the sums of
// kiwi_linfit.hpp (linfit::run hands it over; the layouts below coincide there).  Included by kiwi_hip.hip after the other linfit
// headers, under the same -ffp-contract=off: every fp64 operation below is rounded on its own, and
// tests/linfit_candidates_restatement.py and tests/linfit_candidates_timescan_restatement.py restate each in the same order (the GPU
// tests ask for bit identity).  Notation as in kiwi_linfit.hpp and kiwi_linfit_robust.hpp: N_r = (G_r, b_r, R_r) the sums of
// receiver r from the Gram kernel, N = (G, b, R) their fold by linfit_solve_kernel (weights, anarchy), w_r = receiver_weight[r] (0
// for a disabled receiver).  Per chunk of whole groups
//   linfit_gram_kernel<K> or linfit_scan_gram_kernel<K, J>, linfit_solve_kernel<K>   unchanged: nbr[(g nk + j)][receiver][NN] and
//       normal[(g nk + j)][NN]
//   linfit_candidates_scan_kernel<K>, linfit_candidates_kernel<K>   two entries of ONE body (`candidates_body`), the second with
//       nk = 1 known to the compiler for the plain call.  One workgroup of kCandThreads lanes per (group, tile of kCandThreads
//       candidates); a lane owns
//       ONE candidate with its x in registers, loaded once, and walks the nk offsets itself.  Per offset the rows of (g, j) are
//       staged in LDS (passes 0 and 2: kCandStage receivers at a time from nbr; pass 1: the one folded row from normal); every lane
//       reads the same address at the same time (a broadcast), receivers ascending, into the candidate's own accumulators: the
//       result does not depend on the tiling.  Per row q = (G, b, R) and vector x, `quad`:
//           xb = 0; xb = xb + x_i b_i;  row_i = 0; row_i = row_i + G_ij x_j (j ascending);  xgx = 0; xgx = xgx + x_i row_i
//       -- the sums linfit_solve_kernel and robust_receiver_kernel form --, then val = (R - 2 xb) + xgx, clamped at 0.
//         pass 0    outer l1norm, rows N_r.  A receiver with w_r == 0 or not R_r > 0 is skipped.  m = sqrt(val); n = sqrt(R_r);
//                   v = anarchy ? w_r / n : w_r;  L = L + v m;  D = D + v n;  misfit = L / D (NaN where no receiver counts);
//                   receiver_misfit[g][j][c][r] = (float) m.  This is iterate 0 of robust_receiver_kernel at a fixed x.
//         pass 1    outer l2norm, the folded row N as the only "receiver": misfit = sqrt(val / R), NaN unless R > 0.
//                   free_scale: the candidate is a direction u; quad(N, u) gives u.b and u.G.u; a = (u.b) / (u.G.u), NaN (and a
//                   NaN misfit) unless u.G.u > 0; x_i = a u_i; then as above.  scale[g][j][c] = a.
//         pass 2    outer l2norm, receiver_misfit only: rows N_r, x (free_scale: x_i = scale[g][j][c] u_i, the product of pass 1)
//                   and (float) m per counted receiver as in pass 0; NaN for a candidate whose scale is NaN.
//       The lane keeps its running (minimum over j, argmin j, scale there) -- NaN passed over, the smaller value, the first j among
//       equal values -- and writes cand_misfit, cand_offset, cand_scale once at the end.  Per offset every lane has its (misfit,
//       index); wavefront and workgroup fold them in the order below into tile_v, tile_i[g][j][tile].
//   linfit_candidates_scan_fold_kernel<K>   one wavefront per group: per offset the tiles' bests folded in the same order,
//       best_scale = (u.b) / (u.G.u) of the winner by `quad` on the folded row of (g, j) -- the bits scale[g][j][best_index] has --,
//       then the offsets walked for best_offset (the smaller best_misfit, then the lowest j); status and receiver_norm[g][r] =
//       (float) sqrt(R_r) of the receivers that count (0 otherwise) from the rows of offset 0 (R_r does not depend on the offset).
// The order of "best" is total -- a NaN misfit never wins, then the smaller value, then the LOWER candidate index --, so no answer
// depends on tile shape, chunking or pieces.  No atomics.
// Status of a group: 0 evaluated; 1 no data (l2norm: R not positive; l1norm: no receiver counts): NaN, best_index -1; 2 a basis
// source failed to discretise (set on the host).  A group and offset whose candidates are all NaN has best_index -1.

namespace linfit_candidates_timescan {

using linfit::kCandStage;
using linfit::kCandThreads;

// (Scan, the caller's host arrays, and Bufs, the device buffers kept over the chunks of one run: kiwi_linfit.hpp, whose run() needs them)

// nbr: [group][nk][nrec][NN], normal: [group][nk][NN], w: [nrec] (pass 1: not read).  x: [ncand][K].  misfit, scale:
// [group][nk][ncand] or null.  rmis: [group][nk][ncand][nrec] or null, zeroed before the launch.  cand_misfit, cand_offset,
// cand_scale: [group][ncand] or null.  tile_v, tile_i: [group][nk][gridDim.x] (pass 2: not written).  blockIdx.x = tile of
// candidates, blockIdx.y = group.  kScan = false: the one offset of the plain call -- nk = 1, no cand_* array -- known to the
// compiler: without the walk over the offsets a lane needs fewer registers (K = 6: 114 against 140, 4 waves per SIMD against 3)
template <int K, bool kScan>
__device__ __forceinline__ void candidates_body(const double *__restrict__ nbr, const double *__restrict__ normal, int nrec, int nk,
                                                const double *__restrict__ w, int anarchy, int pass, int free_scale,
                                                const double *__restrict__ x, int ncand, double *__restrict__ misfit,
                                                double *__restrict__ scale, float *__restrict__ rmis, double *__restrict__ cand_misfit,
                                                int *__restrict__ cand_offset, double *__restrict__ cand_scale, double *__restrict__ tile_v,
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
    const int nrows = pass == 1 ? 1 : nrec;
    const double nan = __longlong_as_double(0x7ff8000000000000LL);
    double xu[K];
#pragma unroll
    for (int i = 0; i < K; i++) xu[i] = live ? x[(size_t)cand * K + i] : 0.0;
    double cm = nan, cs = nan;                              // the candidate's smallest misfit over the offsets, the scale there
    int co = -1;                                            // and its offset
    for (int j = 0; j < (kScan ? nk : 1); j++) {
        const size_t gj = kScan ? (size_t)g * nk + j : (size_t)g;
        const size_t slot = gj * ncand + (live ? cand : 0);
        const double *__restrict__ rows = pass == 1 ? normal + gj * NN : nbr + gj * nrec * NN;
        double xc[K];
#pragma unroll
        for (int i = 0; i < K; i++) xc[i] = xu[i];
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
            if (kScan || r0 > 0) __syncthreads();           // (the rows of the stage before, the bests of the offset before)
            const double *__restrict__ src = rows + (size_t)r0 * NN;
            for (int p = tid; p < nr * NN; p += kCandThreads) sq[p] = src[p];
            if (tid < nr) sw[tid] = pass == 1 ? 1.0 : w[r0 + tid];
            __syncthreads();
            for (int r = 0; r < nr; r++) {
                const double wr = sw[r];
                if (wr == 0.0) continue;
                const double *q = sq + r * NN;
                const double Rr = q[NN - 1];
                if (!(Rr > 0.0)) continue;
                double xb, xgx;
                linfit::quad<K>(q, xc, xb, xgx);
                bool ok = true;
                if (pass == 1 && free_scale) {
                    ok = xgx > 0.0;
                    a = ok ? xb / xgx : nan;
                    double xs[K];
#pragma unroll
                    for (int i = 0; i < K; i++) xs[i] = a * xc[i];
                    linfit::quad<K>(q, xs, xb, xgx);
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
        if (pass == 2) continue;
        if (pass == 0) mf = counted ? Ls / Ds : nan;
        if (live) {
            if (misfit) misfit[slot] = mf;
            if (scale) scale[slot] = a;
        }
        if (kScan && mf == mf && (co < 0 || mf < cm)) { cm = mf; co = j; cs = a; }
        double bv = mf;
        int bi = (live && mf == mf) ? cand : -1;
        linfit::wave_best(bv, bi);
        if ((tid & 63) == 0) { best_v[tid >> 6] = bv; best_i[tid >> 6] = bi; }
        __syncthreads();
        if (tid == 0) {
            for (int k = 1; k < kCandThreads / 64; k++) linfit::take_better(bv, bi, best_v[k], best_i[k]);
            tile_v[gj * gridDim.x + blockIdx.x] = bv;
            tile_i[gj * gridDim.x + blockIdx.x] = bi;
        }
    }
    if (!kScan || pass == 2 || !live) return;
    const size_t at = (size_t)g * ncand + cand;
    if (cand_misfit) cand_misfit[at] = cm;
    if (cand_offset) cand_offset[at] = co;
    if (cand_scale) cand_scale[at] = cs;
}

template <int K>
__global__ __launch_bounds__(kCandThreads) void linfit_candidates_scan_kernel(const double *__restrict__ nbr, const double *__restrict__ normal,
                                                                              int nrec, int nk, const double *__restrict__ w, int anarchy,
                                                                              int pass, int free_scale, const double *__restrict__ x, int ncand,
                                                                              double *__restrict__ misfit, double *__restrict__ scale,
                                                                              float *__restrict__ rmis, double *__restrict__ cand_misfit,
                                                                              int *__restrict__ cand_offset, double *__restrict__ cand_scale,
                                                                              double *__restrict__ tile_v, int *__restrict__ tile_i)
{
    candidates_body<K, true>(nbr, normal, nrec, nk, w, anarchy, pass, free_scale, x, ncand, misfit, scale, rmis, cand_misfit, cand_offset,
                             cand_scale, tile_v, tile_i);
}

template <int K>
__global__ __launch_bounds__(kCandThreads) void linfit_candidates_kernel(const double *__restrict__ nbr, const double *__restrict__ normal,
                                                                         int nrec, const double *__restrict__ w, int anarchy, int pass,
                                                                         int free_scale, const double *__restrict__ x, int ncand,
                                                                         double *__restrict__ misfit, double *__restrict__ scale,
                                                                         float *__restrict__ rmis, double *__restrict__ tile_v,
                                                                         int *__restrict__ tile_i)
{
    candidates_body<K, false>(nbr, normal, nrec, 1, w, anarchy, pass, free_scale, x, ncand, misfit, scale, rmis, nullptr, nullptr, nullptr,
                              tile_v, tile_i);
}

// tile_v, tile_i: [group][nk][ntile].  nbr, normal, w as above.  best_index, best_misfit, best_scale (or null): [group][nk];
// best_offset (or null), status: [group]; rnorm: [group][nrec] or null.  blockIdx.x = group
template <int K>
__global__ __launch_bounds__(64) void linfit_candidates_scan_fold_kernel(const double *__restrict__ tile_v, const int *__restrict__ tile_i,
                                                                         int ntile, const double *__restrict__ nbr,
                                                                         const double *__restrict__ normal, const double *__restrict__ w,
                                                                         int nrec, int nk, int outer, const double *__restrict__ x,
                                                                         int *__restrict__ best_offset, int *__restrict__ best_index,
                                                                         double *__restrict__ best_misfit, double *__restrict__ best_scale,
                                                                         int *__restrict__ status, float *__restrict__ rnorm)
{
    constexpr int NN = K * (K + 1) / 2 + K + 1;
    const int g = (int)blockIdx.x, lane = (int)threadIdx.x;
    const double nan = __longlong_as_double(0x7ff8000000000000LL);
    double ov = 0.0;                                        // (lane 0's: the smallest best_misfit so far and its offset)
    int oj = -1;
    for (int j = 0; j < nk; j++) {
        const size_t gj = (size_t)g * nk + j;
        double bv = 0.0;
        int bi = -1;
        for (int t = lane; t < ntile; t += 64) linfit::take_better(bv, bi, tile_v[gj * ntile + t], tile_i[gj * ntile + t]);
        linfit::wave_best(bv, bi);
        if (lane != 0) continue;
        best_index[gj] = bi;
        best_misfit[gj] = bi >= 0 ? bv : nan;
        if (best_scale) {
            double a = nan;
            if (bi >= 0) {
                double u[K], xb, xgx;
#pragma unroll
                for (int i = 0; i < K; i++) u[i] = x[(size_t)bi * K + i];
                linfit::quad<K>(normal + gj * NN, u, xb, xgx);
                a = xgx > 0.0 ? xb / xgx : nan;
            }
            best_scale[gj] = a;
        }
        if (bi >= 0 && (oj < 0 || bv < ov)) { ov = bv; oj = j; }
    }
    int counts = 0;
    for (int r = lane; r < nrec; r += 64) {
        const double Rr = nbr[((size_t)g * nk * nrec + r) * NN + NN - 1];
        const bool in = w[r] != 0.0 && Rr > 0.0;
        if (in) counts = 1;
        if (rnorm) rnorm[(size_t)g * nrec + r] = in ? (float)sqrt(Rr) : 0.f;
    }
    const int any = __any(counts);
    if (lane == 0) {
        if (best_offset) best_offset[g] = oj;
        status[g] = (outer == 2 ? normal[(size_t)g * nk * NN + NN - 1] > 0.0 : any != 0) ? 0 : 1;
    }
}

// what the call cannot do is refused before anything runs: everything the linear fit's time scan and the candidate evaluation refuse
static void check_setup(kiwi_hip_ctx *c, int K, const timescan::Offsets &of, const linfit_timescan::Out &fit, const Scan &sc)
{
    refusing("linear_fit_candidates_time_scan", [&] {
        if (!sc.best_offset) throw std::runtime_error("null best_offset array");
        linfit::check_candidates(linfit::Candidates{ sc.x, sc.ncand, sc.outer_norm, sc.free_scale, sc.best_index, sc.best_misfit, sc.status,
                                                     nullptr, sc.scale, nullptr, nullptr }, K);
        if ((sc.best_scale || sc.cand_scale) && !sc.free_scale) throw std::runtime_error("a best_scale or cand_scale array without free_scale");
        if (sc.cand_offset && !sc.cand_misfit) throw std::runtime_error("a cand_offset array without cand_misfit");
        linfit_timescan::check_setup(c, K, of, fit);
    });
}

// device bytes of one group's candidate outputs as the chunks count them (they are bounded by them too): per offset the tiles' bests
// and the per-candidate arrays that were asked for; a scan counts its bests per offset, its per-candidate minima and receiver_norm
// on top, asked for or not, the plain call (no best_offset) none of them.  Chunk boundaries follow from these figures
static size_t bytes_per_group(const Scan &sc, int nrec, int nk)
{
    const size_t ntile = (size_t)(sc.ncand + kCandThreads - 1) / kCandThreads, nc = (size_t)sc.ncand;
    const size_t per_offset = ntile * (sizeof(double) + sizeof(int)) +
                              nc * ((sc.misfit ? sizeof(double) : 0) + (sc.scaled() ? sizeof(double) : 0) +
                                    (sc.receiver_misfit ? (size_t)nrec * sizeof(float) : 0));
    if (!sc.best_offset) return (size_t)nk * per_offset;
    return (size_t)nk * (per_offset + 2 * sizeof(double) + sizeof(int)) + nc * (2 * sizeof(double) + sizeof(int)) + (size_t)nrec * sizeof(float);
}

// behind the Gram-scan and solve kernels of one chunk: nbr and normal as they left them on the stream
template <int K>
static void launch(kiwi_hip_ctx *c, int ng, int nk, const double *w_d, int anarchy, const double *nbr, const double *normal, const Scan &sc, Bufs &b)
{
    const int nrec = (int)c->recv.size(), ntile = (sc.ncand + kCandThreads - 1) / kCandThreads;
    const dim3 grid((unsigned)ntile, (unsigned)ng);
    double *mis = sc.misfit ? b.misfit.p : nullptr, *scl = sc.scaled() ? b.scale.p : nullptr;
    float *rm = sc.receiver_misfit ? b.rmis.p : nullptr;
    double *cm = sc.cand_misfit ? b.cand_misfit.p : nullptr, *cs = sc.cand_scale ? b.cand_scale.p : nullptr;
    int *co = sc.cand_offset ? b.cand_offset.p : nullptr;
    if (rm) HIPCHECK(hipMemsetAsync(rm, 0, (size_t)ng * nk * sc.ncand * nrec * sizeof(float), c->stream));
    // one pass of the candidate kernel; the plain call (no best_offset, nk = 1) through the entry without the walk over the offsets
    auto pass = [&](int which, int free_scale, double *misfit, double *scale, float *rmis, double *cand_misfit, int *cand_offset,
                    double *cand_scale, double *tile_v, int *tile_i) {
        if (sc.best_offset)
            hipLaunchKernelGGL(linfit_candidates_scan_kernel<K>, grid, dim3(kCandThreads), 0, c->stream, nbr, normal, nrec, nk, w_d, anarchy,
                               which, free_scale, b.x.p, sc.ncand, misfit, scale, rmis, cand_misfit, cand_offset, cand_scale, tile_v, tile_i);
        else
            hipLaunchKernelGGL(linfit_candidates_kernel<K>, grid, dim3(kCandThreads), 0, c->stream, nbr, normal, nrec, w_d, anarchy, which,
                               free_scale, b.x.p, sc.ncand, misfit, scale, rmis, tile_v, tile_i);
        HIPCHECK(hipGetLastError());
    };
    if (sc.outer_norm == 1) {
        pass(0, 0, mis, nullptr, rm, cm, co, nullptr, b.tile_v.p, b.tile_i.p);
    } else {
        pass(1, sc.free_scale, mis, scl, nullptr, cm, co, cs, b.tile_v.p, b.tile_i.p);
        if (rm) pass(2, sc.free_scale, nullptr, scl, rm, nullptr, nullptr, nullptr, nullptr, nullptr);
    }
    hipLaunchKernelGGL(linfit_candidates_scan_fold_kernel<K>, dim3((unsigned)ng), dim3(64), 0, c->stream, b.tile_v.p, b.tile_i.p, ntile, nbr,
                       normal, w_d, nrec, nk, sc.outer_norm, b.x.p, sc.best_offset ? b.best_offset.p : (int *)nullptr, b.best_index.p, b.best_misfit.p,
                       sc.best_scale ? b.best_scale.p : (double *)nullptr, b.status.p, sc.receiver_norm ? b.rnorm.p : (float *)nullptr);
    HIPCHECK(hipGetLastError());
}

// the candidate kernels of one chunk and the downloads of their results for the groups [g0, g0 + ng) of the call
static void chunk(kiwi_hip_ctx *c, int K, int g0, int ng, int nk, const double *w_d, int anarchy, const double *nbr, const double *normal,
                  const Scan &sc, Bufs &b, hipEvent_t after_kernels)
{
    const size_t nrec = c->recv.size(), ntile = (size_t)(sc.ncand + kCandThreads - 1) / kCandThreads;
    const size_t nj = (size_t)ng * nk, nc = (size_t)ng * sc.ncand, njc = nj * sc.ncand;
    if (!b.x.p) {
        b.x.alloc((size_t)sc.ncand * K, &c->dev_bytes);
        HIPCHECK(hipMemcpyAsync(b.x.p, sc.x, (size_t)sc.ncand * K * sizeof(double), hipMemcpyHostToDevice, c->stream));
    }
    b.tile_v.ensure(nj * ntile, &c->dev_bytes); b.tile_i.ensure(nj * ntile, &c->dev_bytes);
    b.best_index.ensure(nj, &c->dev_bytes); b.best_misfit.ensure(nj, &c->dev_bytes);
    b.status.ensure((size_t)ng, &c->dev_bytes);
    if (sc.best_offset) b.best_offset.ensure((size_t)ng, &c->dev_bytes);
    if (sc.best_scale) b.best_scale.ensure(nj, &c->dev_bytes);
    if (sc.cand_misfit) b.cand_misfit.ensure(nc, &c->dev_bytes);
    if (sc.cand_offset) b.cand_offset.ensure(nc, &c->dev_bytes);
    if (sc.cand_scale) b.cand_scale.ensure(nc, &c->dev_bytes);
    if (sc.misfit) b.misfit.ensure(njc, &c->dev_bytes);
    if (sc.scaled()) b.scale.ensure(njc, &c->dev_bytes);
    if (sc.receiver_misfit) b.rmis.ensure(njc * nrec, &c->dev_bytes);
    if (sc.receiver_norm) b.rnorm.ensure((size_t)ng * nrec, &c->dev_bytes);
    by_basis(K, [&](auto k) { launch<k.value>(c, ng, nk, w_d, anarchy, nbr, normal, sc, b); });
    HIPCHECK(hipEventRecord(after_kernels, c->stream));
    const Scan o = sc.at((size_t)g0, (size_t)nk, nrec);
    auto down = [&](void *dst, const void *src, size_t bytes) { if (dst) HIPCHECK(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, c->stream)); };
    down(o.best_offset, b.best_offset.p, (size_t)ng * sizeof(int));
    down(o.status, b.status.p, (size_t)ng * sizeof(int));
    down(o.best_index, b.best_index.p, nj * sizeof(int));
    down(o.best_misfit, b.best_misfit.p, nj * sizeof(double));
    down(o.best_scale, b.best_scale.p, nj * sizeof(double));
    down(o.cand_misfit, b.cand_misfit.p, nc * sizeof(double));
    down(o.cand_offset, b.cand_offset.p, nc * sizeof(int));
    down(o.cand_scale, b.cand_scale.p, nc * sizeof(double));
    down(o.misfit, b.misfit.p, njc * sizeof(double));
    down(o.scale, b.scale.p, njc * sizeof(double));
    down(o.receiver_misfit, b.rmis.p, njc * nrec * sizeof(float));
    down(o.receiver_norm, b.rnorm.p, (size_t)ng * nrec * sizeof(float));
}

// groups that have no fit (a basis source failed to discretise): status 2, NaN, -1 indices, zeros per receiver
static void fill_failed(size_t ngroup, size_t nk, size_t nrec, const Scan &sc)
{
    const double nan = std::numeric_limits<double>::quiet_NaN();
    const size_t nj = ngroup * nk, nc = ngroup * (size_t)sc.ncand, njc = nj * (size_t)sc.ncand;
    std::fill(sc.status, sc.status + ngroup, 2);
    if (sc.best_offset) std::fill(sc.best_offset, sc.best_offset + ngroup, -1);
    std::fill(sc.best_index, sc.best_index + nj, -1);
    std::fill(sc.best_misfit, sc.best_misfit + nj, nan);
    if (sc.best_scale) std::fill(sc.best_scale, sc.best_scale + nj, nan);
    if (sc.cand_misfit) std::fill(sc.cand_misfit, sc.cand_misfit + nc, nan);
    if (sc.cand_offset) std::fill(sc.cand_offset, sc.cand_offset + nc, -1);
    if (sc.cand_scale) std::fill(sc.cand_scale, sc.cand_scale + nc, nan);
    if (sc.misfit) std::fill(sc.misfit, sc.misfit + njc, nan);
    if (sc.scale) std::fill(sc.scale, sc.scale + njc, nan);
    if (sc.receiver_misfit) std::fill(sc.receiver_misfit, sc.receiver_misfit + njc * nrec, 0.f);
    if (sc.receiver_norm) std::fill(sc.receiver_norm, sc.receiver_norm + ngroup * nrec, 0.f);
}

// the groups [isrc0, isrc0 + ngroup K) of the uploaded batch; adds its HIP-event times to c->linfit_cand_timescan_ms.  The skeleton
// is linfit_timescan::run's: the halo put back on the way out, every source synthesised, chunks of whole groups
static void run(kiwi_hip_ctx *c, int isrc0, int ngroup, int K, const timescan::Offsets &of, const double *receiver_weight, int anarchy,
                const linfit_timescan::Out &fit, const Scan &sc)
{
    check_setup(c, K, of, fit, sc);
    check_group_range("linear_fit_candidates_time_scan", c, isrc0, ngroup, K);
    if (ngroup == 0) return;
    const int nrec = (int)c->recv.size(), NN = linfit::nn_of(K), nk = of.nk;
    c->misfit_d.ensure((size_t)c->nsrc * c->nmis, &c->dev_bytes);
    c->global_d.ensure((size_t)c->nsrc, &c->dev_bytes);
    c->fuse_now = false;                                   // the plain synthetics go to memory
    timescan::HaloScope halo(c);
    halo.widen(of.max_abs());

    const std::vector<double> w = receiver_weights(c, receiver_weight);
    DevBuf<double> w_d, nbr_d, coef_d, mis_d, piv_d, normal_d;
    DevBuf<int> st_d, best_d;
    Bufs bufs;
    w_d.alloc((size_t)nrec, &c->dev_bytes);
    HIPCHECK(hipMemcpyAsync(w_d.p, w.data(), (size_t)nrec * sizeof(double), hipMemcpyHostToDevice, c->stream));
    HIPCHECK(hipStreamSynchronize(c->stream));

    const PooledEvents<6> ev(c);
    // per group: the sums by receiver and their fold at every offset, the candidate outputs
    const size_t per_group = (size_t)nk * (nrec + 1) * NN * sizeof(double) + bytes_per_group(sc, nrec, nk);
    int g0 = 0;
    while (g0 < ngroup) {
        const int ng = next_group_chunk(c, isrc0, g0, ngroup, K, 1, per_group, kNoSourceCap);
        const int s0 = isrc0 + g0 * K;
        const size_t nsolve = (size_t)ng * nk;
        HIPCHECK(hipEventRecord(ev[0], c->stream));
        run_chunk(c, s0, ng * K, 0);
        HIPCHECK(hipEventRecord(ev[1], c->stream));
        nbr_d.ensure(nsolve * nrec * NN, &c->dev_bytes);
        coef_d.ensure(nsolve * K, &c->dev_bytes); mis_d.ensure(nsolve, &c->dev_bytes); piv_d.ensure(nsolve, &c->dev_bytes);
        st_d.ensure(nsolve, &c->dev_bytes); best_d.ensure((size_t)ng, &c->dev_bytes);
        normal_d.ensure(nsolve * NN, &c->dev_bytes);
        HIPCHECK(hipMemsetAsync(nbr_d.p, 0, nsolve * nrec * NN * sizeof(double), c->stream));
        linfit_timescan::GramArgs a;
        a.sr = SynRows{ c->syn_d.p, c->syn_stride, c->comps_d.p, c->tw_d.p, c->moment_d.p, c->risetime_d.p, nullptr };
        a.recv = c->recv_d.p;
        a.reft = c->reft_d.p;
        a.isrc0 = s0; a.nrec = nrec; a.k0 = of.k0; a.kstep = of.kstep; a.nk = nk;
        a.lds_row = linfit_timescan::kTile + (std::min(linfit_timescan::kPerPass[K], nk) - 1) * of.kstep;
        a.dt = c->gm.dt; a.syn_factor = c->syn_factor;
        a.nbr = nbr_d.p;
        linfit_timescan::launch_any(c, K, a, ng, w_d.p, anarchy ? 1 : 0, coef_d.p, mis_d.p, st_d.p, piv_d.p, normal_d.p, best_d.p, ev[2]);
        HIPCHECK(hipEventRecord(ev[3], c->stream));
        chunk(c, K, g0, ng, nk, w_d.p, anarchy ? 1 : 0, nbr_d.p, normal_d.p, sc, bufs, ev[4]);       // (its downloads are queued behind ev[4])
        const size_t o = (size_t)g0 * nk;
        HIPCHECK(hipMemcpyAsync(fit.coef + o * K, coef_d.p, nsolve * K * sizeof(double), hipMemcpyDeviceToHost, c->stream));
        HIPCHECK(hipMemcpyAsync(fit.misfit + o, mis_d.p, nsolve * sizeof(double), hipMemcpyDeviceToHost, c->stream));
        HIPCHECK(hipMemcpyAsync(fit.status + o, st_d.p, nsolve * sizeof(int), hipMemcpyDeviceToHost, c->stream));
        HIPCHECK(hipEventRecord(ev[5], c->stream));
        HIPCHECK(hipStreamSynchronize(c->stream));
        for (int i = 0; i < 5; i++) ev.add_elapsed(c->linfit_cand_timescan_ms, i, i, i + 1);
        g0 += ng;
    }
    leave_evaluated(c, isrc0, ngroup * K, 0);              // the plain evaluation of the basis sources was made on the way
    for_each_failed_group(c, isrc0, ngroup, K, [&](int g) {
        linfit_timescan::mark_failed((size_t)g, (size_t)K, (size_t)nk, fit);
        fill_failed(1, (size_t)nk, (size_t)nrec, sc.at((size_t)g, (size_t)nk, (size_t)nrec));
    });
}

// kiwi_hip_linear_fit_candidates_time_scan_params piece by piece (PieceCall, kiwi_group_run.hpp); fit: the free fit made on the way
static PieceCall piece_call(int K, const timescan::Offsets &of, const double *receiver_weight, int anarchy, const linfit_timescan::Out &fit,
                            const Scan &sc)
{
    const size_t nk = (size_t)of.nk;
    return PieceCall{ K,
        [=](kiwi_hip_ctx *c) { check_setup(c, K, of, fit, sc); },
        [=](kiwi_hip_ctx *c, int s0, int n) {
            const size_t g = (size_t)(s0 / K), ng = (size_t)(n / K), nrec = c->recv.size();
            linfit_timescan::fill_failed(ng, (size_t)K, nk, fit.at(g, (size_t)K, nk));
            fill_failed(ng, nk, nrec, sc.at(g, nk, nrec));
        },
        [=](kiwi_hip_ctx *c, int s0, int n) {
            const size_t g = (size_t)(s0 / K);
            run(c, 0, n / K, K, of, receiver_weight, anarchy, fit.at(g, (size_t)K, nk), sc.at(g, nk, c->recv.size()));
        } };
}

} // namespace linfit_candidates_timescan
