// kiwi_linfit_candidates_timescan.hpp -- the misfits of many GIVEN coefficient vectors per group at MANY origin times from ONE
// synthesis of the basis (kiwi_hip_linear_fit_candidates_time_scan): kiwi_linfit_timescan.hpp's sums per offset with
// kiwi_linfit_candidates.hpp's evaluation on them.  Nothing new is computed: per chunk of whole groups
//   linfit_scan_gram_kernel<K, J>, linfit_solve_kernel<K>   unchanged: nbr[(g nk + j)][receiver][NN] and normal[(g nk + j)][NN]
//   linfit_candidates_scan_kernel<K>   one workgroup of kCandThreads lanes per (group, tile of kCandThreads candidates); a lane owns
//       ONE candidate with its x in registers, loaded once, and walks the nk offsets itself.  Per offset the rows of (g, j) are
//       staged in LDS (passes 0 and 2: kCandStage receivers at a time from nbr; pass 1: the one folded row from normal) and read as
//       a broadcast, receivers ascending, into the lane's own accumulators: linfit_candidates_kernel's passes operation for operation
//       (`quad`, the clamp, the roots), so offset j has the bits that kernel gives on the rows of (g, j).  The lane keeps its running
//       (minimum over j, argmin j, scale there) -- NaN passed over, the smaller value, the first j among equal values -- and writes
//       cand_misfit, cand_offset, cand_scale once at the end.  Per offset the workgroup folds its best in linfit_candidates_kernel's
//       order into tile_v, tile_i[g][j][tile].
//   linfit_candidates_scan_fold_kernel<K>   one wavefront per group: per offset the tiles' bests folded in the same order,
//       best_scale = (u.b) / (u.G.u) of the winner by `quad` on the folded row of (g, j) -- the bits scale[g][j][best_index] has --,
//       then the offsets walked for best_offset (the smaller best_misfit, then the lowest j); status and receiver_norm from the
//       rows of offset 0 (R_r does not depend on the offset).
// The order of "best" is total, so no answer depends on tile shape, chunking or pieces.  No atomics.  Included by kiwi_hip.hip after
// the other linfit headers, under the same -ffp-contract=off; tests/linfit_candidates_timescan_restatement.py restates the folds.

namespace linfit_candidates_timescan {

using linfit::kCandStage;
using linfit::kCandThreads;

// host arrays of the caller for the groups of ONE call of run(): best_offset, status [group]; best_index, best_misfit, best_scale
// [group][nk]; cand_misfit, cand_offset, cand_scale [group][ncand]; misfit, scale [group][nk][ncand]; receiver_misfit
// [group][nk][ncand][nrec]; receiver_norm [group][nrec].  x [ncand][K] is shared by all groups and offsets.  best_scale and
// everything after it may be null
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
        s.best_offset += g; s.status += g; s.best_index += g * nk; s.best_misfit += g * nk;
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

// nbr: [group][nk][nrec][NN], normal: [group][nk][NN], w: [nrec] (pass 1: not read).  x: [ncand][K].  misfit, scale:
// [group][nk][ncand] or null.  rmis: [group][nk][ncand][nrec] or null, zeroed before the launch.  cand_misfit, cand_offset,
// cand_scale: [group][ncand] or null.  tile_v, tile_i: [group][nk][gridDim.x] (pass 2: not written).  blockIdx.x = tile of
// candidates, blockIdx.y = group.  The passes are linfit_candidates_kernel's
template <int K>
__global__ __launch_bounds__(kCandThreads) void linfit_candidates_scan_kernel(const double *__restrict__ nbr, const double *__restrict__ normal,
                                                                              int nrec, int nk, const double *__restrict__ w, int anarchy,
                                                                              int pass, int free_scale, const double *__restrict__ x, int ncand,
                                                                              double *__restrict__ misfit, double *__restrict__ scale,
                                                                              float *__restrict__ rmis, double *__restrict__ cand_misfit,
                                                                              int *__restrict__ cand_offset, double *__restrict__ cand_scale,
                                                                              double *__restrict__ tile_v, int *__restrict__ tile_i)
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
    for (int j = 0; j < nk; j++) {
        const size_t gj = (size_t)g * nk + j;
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
            __syncthreads();                                // (the rows of the stage before, the bests of the offset before)
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
        if (mf == mf && (co < 0 || mf < cm)) { cm = mf; co = j; cs = a; }
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
    if (pass == 2 || !live) return;
    const size_t at = (size_t)g * ncand + cand;
    if (cand_misfit) cand_misfit[at] = cm;
    if (cand_offset) cand_offset[at] = co;
    if (cand_scale) cand_scale[at] = cs;
}

// tile_v, tile_i: [group][nk][ntile].  nbr, normal, w as above.  best_index, best_misfit, best_scale (or null): [group][nk];
// best_offset, status: [group]; rnorm: [group][nrec] or null.  blockIdx.x = group
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
        best_offset[g] = oj;
        status[g] = (outer == 2 ? normal[(size_t)g * nk * NN + NN - 1] > 0.0 : any != 0) ? 0 : 1;
    }
}

// device buffers of the candidate scan, kept over the chunks of one run
struct Bufs {
    DevBuf<double> x, misfit, scale, tile_v, best_misfit, best_scale, cand_misfit, cand_scale;
    DevBuf<float> rmis, rnorm;
    DevBuf<int> tile_i, best_index, best_offset, status, cand_offset;
};

// a refusal of one of the calls this one is made of, under this call's name
template <class F>
static void refusing(F &&f)
{
    try { f(); }
    catch (const std::runtime_error &e) {
        std::string m = e.what();
        const size_t colon = m.find(": ");
        if (colon != std::string::npos && m.find(' ') > colon) m = m.substr(colon + 2);       // (the other call's name in front)
        throw std::runtime_error("linear_fit_candidates_time_scan: " + m);
    }
}

// what the call cannot do is refused before anything runs: everything the linear fit's time scan and the candidate evaluation refuse
static void check_setup(kiwi_hip_ctx *c, int K, const timescan::Offsets &of, const linfit_timescan::Out &fit, const Scan &sc)
{
    refusing([&] {
        if (!sc.best_offset) throw std::runtime_error("null best_offset array");
        linfit::check_candidates(linfit::Candidates{ sc.x, sc.ncand, sc.outer_norm, sc.free_scale, sc.best_index, sc.best_misfit, sc.status,
                                                     nullptr, sc.scale, nullptr, nullptr }, K);
        if ((sc.best_scale || sc.cand_scale) && !sc.free_scale) throw std::runtime_error("a best_scale or cand_scale array without free_scale");
        if (sc.cand_offset && !sc.cand_misfit) throw std::runtime_error("a cand_offset array without cand_misfit");
        linfit_timescan::check_setup(c, K, of, fit);
    });
}

// device bytes of one group's candidate outputs (the chunk is bounded by them too)
static size_t bytes_per_group(const Scan &sc, int nrec, int nk)
{
    const size_t ntile = (size_t)(sc.ncand + kCandThreads - 1) / kCandThreads, nc = (size_t)sc.ncand;
    return (size_t)nk * (ntile * (sizeof(double) + sizeof(int)) + 2 * sizeof(double) + sizeof(int) +
                         nc * ((sc.misfit ? sizeof(double) : 0) + (sc.scaled() ? sizeof(double) : 0) +
                               (sc.receiver_misfit ? (size_t)nrec * sizeof(float) : 0))) +
           nc * (2 * sizeof(double) + sizeof(int)) + (size_t)nrec * sizeof(float);
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
    if (sc.outer_norm == 1) {
        hipLaunchKernelGGL(linfit_candidates_scan_kernel<K>, grid, dim3(kCandThreads), 0, c->stream, nbr, normal, nrec, nk, w_d, anarchy, 0, 0,
                           b.x.p, sc.ncand, mis, (double *)nullptr, rm, cm, co, (double *)nullptr, b.tile_v.p, b.tile_i.p);
        HIPCHECK(hipGetLastError());
    } else {
        hipLaunchKernelGGL(linfit_candidates_scan_kernel<K>, grid, dim3(kCandThreads), 0, c->stream, nbr, normal, nrec, nk, w_d, anarchy, 1,
                           sc.free_scale, b.x.p, sc.ncand, mis, scl, (float *)nullptr, cm, co, cs, b.tile_v.p, b.tile_i.p);
        HIPCHECK(hipGetLastError());
        if (rm) {
            hipLaunchKernelGGL(linfit_candidates_scan_kernel<K>, grid, dim3(kCandThreads), 0, c->stream, nbr, normal, nrec, nk, w_d, anarchy, 2,
                               sc.free_scale, b.x.p, sc.ncand, (double *)nullptr, scl, rm, (double *)nullptr, (int *)nullptr,
                               (double *)nullptr, (double *)nullptr, (int *)nullptr);
            HIPCHECK(hipGetLastError());
        }
    }
    hipLaunchKernelGGL(linfit_candidates_scan_fold_kernel<K>, dim3((unsigned)ng), dim3(64), 0, c->stream, b.tile_v.p, b.tile_i.p, ntile, nbr,
                       normal, w_d, nrec, nk, sc.outer_norm, b.x.p, b.best_offset.p, b.best_index.p, b.best_misfit.p,
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
    b.best_offset.ensure((size_t)ng, &c->dev_bytes); b.status.ensure((size_t)ng, &c->dev_bytes);
    if (sc.best_scale) b.best_scale.ensure(nj, &c->dev_bytes);
    if (sc.cand_misfit) b.cand_misfit.ensure(nc, &c->dev_bytes);
    if (sc.cand_offset) b.cand_offset.ensure(nc, &c->dev_bytes);
    if (sc.cand_scale) b.cand_scale.ensure(nc, &c->dev_bytes);
    if (sc.misfit) b.misfit.ensure(njc, &c->dev_bytes);
    if (sc.scaled()) b.scale.ensure(njc, &c->dev_bytes);
    if (sc.receiver_misfit) b.rmis.ensure(njc * nrec, &c->dev_bytes);
    if (sc.receiver_norm) b.rnorm.ensure((size_t)ng * nrec, &c->dev_bytes);
    switch (K) {
    case 1: launch<1>(c, ng, nk, w_d, anarchy, nbr, normal, sc, b); break;
    case 2: launch<2>(c, ng, nk, w_d, anarchy, nbr, normal, sc, b); break;
    case 3: launch<3>(c, ng, nk, w_d, anarchy, nbr, normal, sc, b); break;
    case 4: launch<4>(c, ng, nk, w_d, anarchy, nbr, normal, sc, b); break;
    case 5: launch<5>(c, ng, nk, w_d, anarchy, nbr, normal, sc, b); break;
    case 6: launch<6>(c, ng, nk, w_d, anarchy, nbr, normal, sc, b); break;
    case 7: launch<7>(c, ng, nk, w_d, anarchy, nbr, normal, sc, b); break;
    default: launch<8>(c, ng, nk, w_d, anarchy, nbr, normal, sc, b); break;
    }
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

// groups that have no fit (a basis source failed to discretise): status 2, NaN, -1 indices, zeros per receiver (cand_fill_failed)
static void fill_failed(size_t ngroup, size_t nk, size_t nrec, const Scan &sc)
{
    const double nan = std::numeric_limits<double>::quiet_NaN();
    const size_t nj = ngroup * nk, nc = ngroup * (size_t)sc.ncand, njc = nj * (size_t)sc.ncand;
    std::fill(sc.status, sc.status + ngroup, 2);
    std::fill(sc.best_offset, sc.best_offset + ngroup, -1);
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
    if (isrc0 < 0 || ngroup < 0 || (long long)isrc0 + (long long)ngroup * K > (long long)c->nsrc)
        throw std::runtime_error("linear_fit_candidates_time_scan: sources " + std::to_string(isrc0) + " .. " +
                                 std::to_string((long long)isrc0 + (long long)ngroup * K) + " are not inside the uploaded batch of " +
                                 std::to_string(c->nsrc));
    if (ngroup == 0) return;
    const int nrec = (int)c->recv.size(), NN = linfit::nn_of(K), nk = of.nk;
    c->misfit_d.ensure((size_t)c->nsrc * c->nmis, &c->dev_bytes);
    c->global_d.ensure((size_t)c->nsrc, &c->dev_bytes);
    const int base = c->halo, shalo = of.max_abs();
    c->fuse_now = false;                                   // the plain synthetics go to memory
    struct Restore {
        kiwi_hip_ctx *c; bool want; int halo;
        ~Restore()
        {
            c->want_spansrc = want;
            try { HIPCHECK(hipSetDevice(c->device)); timescan::set_halo(c, halo); }
            catch (...) { c->prepared = false; }           // (the next call lays everything out again)
        }
    } restore{ c, c->want_spansrc, base };
    c->want_spansrc = true;
    timescan::set_halo(c, base + shalo);

    std::vector<double> w((size_t)nrec, 0.0);
    for (int r = 0; r < nrec; r++)
        if (c->recv[r].enabled && c->recv[r].ncomp > 0) w[r] = receiver_weight ? receiver_weight[r] : 1.0;
    DevBuf<double> w_d, nbr_d, coef_d, mis_d, piv_d, normal_d;
    DevBuf<int> st_d, best_d;
    Bufs bufs;
    w_d.alloc((size_t)nrec, &c->dev_bytes);
    HIPCHECK(hipMemcpyAsync(w_d.p, w.data(), (size_t)nrec * sizeof(double), hipMemcpyHostToDevice, c->stream));
    HIPCHECK(hipStreamSynchronize(c->stream));

    hipEvent_t ev[6];
    for (int i = 0; i < 6; i++) ev[i] = c->get_event();
    struct Return { kiwi_hip_ctx *c; hipEvent_t *ev; ~Return() { for (int i = 0; i < 6; i++) c->event_pool.push_back(ev[i]); } } ret{ c, ev };
    const size_t per_group = bytes_per_group(sc, nrec, nk);
    int g0 = 0;
    while (g0 < ngroup) {
        // whole groups, bounded by workspace bytes the way linfit_timescan::run bounds its chunks, and by the candidate outputs
        size_t bytes = 0;
        int ng = 0;
        while (g0 + ng < ngroup) {
            size_t add = 0;
            for (int s = isrc0 + (g0 + ng) * K; s < isrc0 + (g0 + ng + 1) * K; s++) {
                const size_t ncent = (size_t)(c->cent_ofs[s + 1] - c->cent_ofs[s]);
                add += ncent * nrec * (sizeof(GeoRec) + (c->accum_mode == 0 ? 512 + kCoefLine * sizeof(float) : 0)) + plan_bytes(c, s, (size_t)nrec) + c->syn_stride * sizeof(float);
            }
            add += (size_t)nk * (nrec + 1) * NN * sizeof(double) + per_group;
            if (ng > 0 && (bytes + add > c->chunk_bytes_limit || (ng + 1) * K > 65535)) break;
            bytes += add; ng++;
        }
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
        for (int i = 0; i < 5; i++) {
            float t = 0.f;
            HIPCHECK(hipEventElapsedTime(&t, ev[i], ev[i + 1]));
            c->linfit_cand_timescan_ms[i] += t;
        }
        g0 += ng;
    }
    // what an evaluation of the range leaves behind (eval_impl): the plain evaluation of the basis sources was made on the way
    c->last_isrc0 = isrc0; c->last_nsrc = ngroup * K; c->last_proc_which = 0;
    c->evaluated.resize((size_t)c->nsrc, 0);
    std::fill(c->evaluated.begin() + isrc0, c->evaluated.begin() + isrc0 + ngroup * K, 1);
    for (int g = 0; g < ngroup; g++) {
        bool bad = false;
        for (int i = 0; i < K; i++) if (c->src_status[(size_t)isrc0 + (size_t)g * K + i]) bad = true;
        if (!bad) continue;
        linfit_timescan::mark_failed((size_t)g, (size_t)K, (size_t)nk, fit);
        fill_failed(1, (size_t)nk, (size_t)nrec, sc.at((size_t)g, (size_t)nk, (size_t)nrec));
    }
}

} // namespace linfit_candidates_timescan
