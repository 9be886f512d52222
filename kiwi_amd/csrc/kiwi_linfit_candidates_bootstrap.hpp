// kiwi_linfit_candidates_bootstrap.hpp -- the bootstrap over the receivers of a candidate search, joint over group (location), origin
// time and candidate (mechanism), without the [candidate][receiver] matrix: kiwi_hip_linear_fit_candidates_bootstrap.  What it
// answers is DEFINED by two existing calls: kiwi_hip_linear_fit_candidates_time_scan (free_scale = 0) writes receiver_misfit
// [ngroup][nk][ncand][nrec] and receiver_norm [ngroup][nrec] as floats, kiwi_hip_outer_misfits reads them as ngroup nk ncand sources
// of one slot per receiver and returns the best source of every draw.  Here a candidate's m_r stays in LDS between the quadratic form
// and the draw loop, and the norm side of the fold -- b, and the denominator of every draw -- is made once per group, because it does
// not depend on the candidate.  Included by kiwi_hip.hip after kiwi_linfit_candidates_timescan.hpp, under the same -ffp-contract=off:
// every fp64 operation below is rounded on its own; tests/linfit_candidates_bootstrap_restatement.py composes the two restatements
// of the parents, and the GPU tests ask for bit identity with the host route.  Per chunk of whole groups, behind the unchanged
// linfit_scan_gram_kernel and linfit_solve_kernel (nbr[(g nk + j)][receiver][NN], normal[(g nk + j)][NN] on the stream):
//   bootstrap_prepare_kernel   one workgroup per group.  From the rows of offset 0 (R_r does not depend on the offset), per receiver:
//       counted = w_r != 0 and R_r > 0;  N = counted ? (double)(float) sqrt(R_r) : 0 -- the norm passes through float as on the host
//       route --;  rw = w_r, under anarchy q = rw / (N != 0 ? N : -1), rw = q > 0 or NaN ? q : 0 (outer_prepare_kernel);  b = N rw,
//       squared under l2norm.  Per draw: ns = 0; ns = ns + b_r c_dr, r ascending (outer_draw_kernel).  status as the candidate call
//       has it (l2norm: folded R > 0; l1norm: a receiver counts; 2 for a group with a failed basis source, flagged by the host).
//   linfit_candidates_bootstrap_kernel<K>   one workgroup of kCandThreads lanes per ((g, j), tile of kCandThreads candidates), a
//       lane owns ONE candidate.  Phase 1 is pass 0 / pass 2 of candidates_body: rows staged in LDS, broadcast reads, receivers
//       ascending, linfit::quad, val = (R - 2 xb) + xgx clamped at 0, m = sqrt(val); (float) m -- 0 for a receiver that is not
//       counted -- goes to LDS as sm[r][lane].  Phase 2 walks the draws of the pass in tiles of kTileD: the weight rows staged as
//       cs[r][t]; per receiver mv = (double) sm[r][lane] -- under l2norm the host route forms sqrt(mv mv), which IS mv for a float
//       (tests) --, a = mv rw_r, squared under l2norm; ms_t = ms_t + a c_rt from zero, r ascending; v = ms / ns (root under l2norm),
//       excluded (NaN) where not ns > 0 or not v >= 0.  (value, candidate) folded over wavefront and workgroup; the tile's best of
//       every draw goes to slab_v, slab_i[(g, j)][tile][draw of the pass].  Nothing per candidate goes to global memory.
//   bootstrap_fold_kernel   per (group, draw): the slab's offsets and tiles folded into grp_v, grp_j, grp_c[group][draw].
//   bootstrap_best_kernel   per draw: the chunk's groups folded into the running best of the run.
// The order of "best" is total -- excluded last, then the smaller value, then the lowest (g, j, c) --, so no answer depends on
// tiles, draw passes, chunks, pieces or devices.  No atomics.  A draw with every source excluded: NaN, -1, -1, -1.

namespace linfit_candidates_bootstrap {

using linfit::kCandThreads;

constexpr int kTileD = 16;                          // draws per tile: 16 fp64 accumulators per lane
constexpr int kStage = 16;                          // receivers per stage of phase 1: 16 x NN x 8 bytes = 5.6 KiB at K = 8
constexpr int kLdsBytes = 152 * 1024;               // of the 160 KiB a workgroup may hold
// LDS of the candidate kernel: what does not grow with the receivers (the row stage, the wavefronts' bests) and what one receiver
// adds (its column of m, its weight row of a draw tile, its rw)
__host__ __device__ constexpr int lds_fixed(int K) { return kStage * linfit::nn_of(K) * 8 + (kCandThreads / 64) * kTileD * 12; }
constexpr int kLdsPerRec = kCandThreads * 4 + kTileD * 8 + 8;
constexpr int kMaxRec = (kLdsBytes - lds_fixed(linfit::kMaxBasis)) / kLdsPerRec;       // 128, for every K
static_assert(kMaxRec >= 64, "the layout must hold 64 receivers");
static size_t lds_bytes(int K, int nrec) { return (size_t)lds_fixed(K) + (size_t)nrec * kLdsPerRec; }

static const char *const kName = "linear_fit_candidates_bootstrap";

// host arrays of the caller for the groups of ONE call of run(): status [group]; group_value, group_offset, group_cand
// [group][ndraw], all three or none.  best_value, best_group, best_offset, best_cand [ndraw] belong to the WHOLE call: the caller
// fills them with NaN / -1 (begin), every run() folds its own bests into them with `group0` added to its group indices, under `mu`
// where runs of several devices share them.  x [ncand][K] and draw_weights [ndraw][nrec] are shared by all groups
struct Boot {
    const double *x; int ncand, outer_norm, ndraw; const double *draw_weights;
    double *best_value; int *best_group, *best_offset, *best_cand;
    int *status;
    double *group_value; int *group_offset, *group_cand;
    int group0; std::mutex *mu;
    Boot at(size_t g) const
    {
        Boot b = *this;
        b.status += g; b.group0 += (int)g;
        if (group_value) { b.group_value += g * (size_t)ndraw; b.group_offset += g * (size_t)ndraw; b.group_cand += g * (size_t)ndraw; }
        return b;
    }
    void begin() const
    {
        std::fill(best_value, best_value + ndraw, std::numeric_limits<double>::quiet_NaN());
        std::fill(best_group, best_group + ndraw, -1); std::fill(best_offset, best_offset + ndraw, -1); std::fill(best_cand, best_cand + ndraw, -1);
    }
};

// w: [nrec]; nbr: [group][nk][nrec][NN]; normal: [group][nk][NN]; cw: [ndraw][nrec]; failed: [group].  rw, b: [group][nrec];
// ns: [group][ndraw]; status: [group].  blockIdx.x = group
__global__ __launch_bounds__(256) void bootstrap_prepare_kernel(const double *__restrict__ nbr, const double *__restrict__ normal, int NN,
                                                                int nrec, int nk, const double *__restrict__ w, int anarchy, int l2,
                                                                const double *__restrict__ cw, int ndraw, const int *__restrict__ failed,
                                                                double *__restrict__ rw_out, double *__restrict__ b_out,
                                                                double *__restrict__ ns, int *__restrict__ status)
{
    __shared__ int any;
    const int g = (int)blockIdx.x, tid = (int)threadIdx.x;
    if (tid == 0) any = 0;
    __syncthreads();
    for (int r = tid; r < nrec; r += 256) {
        const double Rr = nbr[((size_t)g * nk * nrec + r) * NN + NN - 1];
        const bool in = w[r] != 0.0 && Rr > 0.0;
        const double N = in ? (double)(float)sqrt(Rr) : 0.0;
        double rw = w[r];
        if (anarchy) {
            const double q = rw / (N != 0.0 ? N : -1.0);
            rw = (q > 0.0 || q != q) ? q : 0.0;
        }
        double bv = N * rw;
        if (l2) bv = bv * bv;
        rw_out[(size_t)g * nrec + r] = rw;
        b_out[(size_t)g * nrec + r] = bv;
        if (in) any = 1;
    }
    __syncthreads();                                        // (b_out of this group: written by this workgroup, visible to it)
    const double *b = b_out + (size_t)g * nrec;
    for (int d = tid; d < ndraw; d += 256) {
        double s = 0.0;
        for (int r = 0; r < nrec; r++) s = s + b[r] * cw[(size_t)d * nrec + r];
        ns[(size_t)g * ndraw + d] = s;
    }
    if (tid == 0) status[g] = failed[g] ? 2 : (l2 ? normal[(size_t)g * nk * NN + NN - 1] > 0.0 : any != 0) ? 0 : 1;
}

// nbr, w as above; x: [ncand][K]; rw: [group][nrec]; ns: [group][ndraw]; cw: [ndraw][nrec].  The draws [d0, d0 + nd) of this pass;
// slab_v, slab_i: [group nk][ntile][ndp].  blockIdx.x = (g nk + j) ntile + tile.  Dynamic LDS: lds_bytes(K, nrec)
template <int K>
__global__ __launch_bounds__(kCandThreads) void linfit_candidates_bootstrap_kernel(const double *__restrict__ nbr, int nrec, int nk,
                                                                                   const double *__restrict__ w, const double *__restrict__ x,
                                                                                   int ncand, int ntile, const double *__restrict__ rw,
                                                                                   const double *__restrict__ ns, const double *__restrict__ cw,
                                                                                   int ndraw, int d0, int nd, int ndp, int l2,
                                                                                   double *__restrict__ slab_v, int *__restrict__ slab_i)
{
    constexpr int NN = K * (K + 1) / 2 + K + 1, NW = kCandThreads / 64;
    extern __shared__ double lds[];
    double *sq = lds;                                       // [kStage][NN]
    double *srw = sq + kStage * NN;                         // [nrec]
    double *cs = srw + nrec;                                // [nrec][kTileD]
    double *red_v = cs + (size_t)nrec * kTileD;             // [NW][kTileD]
    int *red_i = (int *)(red_v + NW * kTileD);              // [NW][kTileD]
    float *sm = (float *)(red_i + NW * kTileD);             // [nrec][kCandThreads]
    const int tid = (int)threadIdx.x, tile = (int)(blockIdx.x % (unsigned)ntile);
    const size_t gj = blockIdx.x / (unsigned)ntile;
    const int g = (int)(gj / (unsigned)nk);
    const int cand = tile * kCandThreads + tid;
    const bool live = cand < ncand;
    const double nan = __longlong_as_double(0x7ff8000000000000LL);
    {
        double xc[K];
#pragma unroll
        for (int i = 0; i < K; i++) xc[i] = live ? x[(size_t)cand * K + i] : 0.0;
        const double *__restrict__ rows = nbr + gj * nrec * NN;
        for (int r0 = 0; r0 < nrec; r0 += kStage) {
            const int nr = nrec - r0 < kStage ? nrec - r0 : kStage;
            if (r0 > 0) __syncthreads();
            const double *__restrict__ src = rows + (size_t)r0 * NN;
            for (int p = tid; p < nr * NN; p += kCandThreads) sq[p] = src[p];
            __syncthreads();
            for (int r = 0; r < nr; r++) {
                const double *q = sq + r * NN;
                const double Rr = q[NN - 1];
                float mf = 0.f;
                if (w[r0 + r] != 0.0 && Rr > 0.0) {
                    double xb, xgx;
                    linfit::quad<K>(q, xc, xb, xgx);
                    double val = (Rr - 2.0 * xb) + xgx;
                    val = val > 0.0 ? val : 0.0;
                    mf = (float)sqrt(val);
                }
                sm[(r0 + r) * kCandThreads + tid] = mf;
            }
        }
    }
    for (int r = tid; r < nrec; r += kCandThreads) srw[r] = rw[(size_t)g * nrec + r];
    const int lane = tid & 63, wave = tid >> 6;
    for (int t0 = 0; t0 < nd; t0 += kTileD) {
        __syncthreads();                                    // (srw; the weight rows and the bests of the tile before)
        for (int i = tid; i < nrec * kTileD; i += kCandThreads) {
            const int t = i / nrec, r = i - t * nrec;
            cs[r * kTileD + t] = t0 + t < nd ? cw[(size_t)(d0 + t0 + t) * nrec + r] : 0.0;
        }
        __syncthreads();
        double ms[kTileD];
#pragma unroll
        for (int t = 0; t < kTileD; t++) ms[t] = 0.0;
        for (int r = 0; r < nrec; r++) {
            const double mv = (double)sm[r * kCandThreads + tid];
            double av = mv * srw[r];
            if (l2) av = av * av;
            const double *c = cs + r * kTileD;
#pragma unroll
            for (int t = 0; t < kTileD; t++) ms[t] = ms[t] + av * c[t];
        }
#pragma unroll
        for (int t = 0; t < kTileD; t++) {
            const double den = t0 + t < nd ? ns[(size_t)g * ndraw + d0 + t0 + t] : 0.0;
            double v = nan;
            if (live && den > 0.0) {
                v = ms[t] / den;
                if (l2) v = sqrt(v);
                if (!(v >= 0.0)) v = nan;
            }
            int bi = v == v ? cand : -1;
            linfit::wave_best(v, bi);
            if (lane == 0) { red_v[wave * kTileD + t] = v; red_i[wave * kTileD + t] = bi; }
        }
        __syncthreads();
        if (tid < kTileD && t0 + tid < nd) {
            double v = red_v[tid];
            int bi = red_i[tid];
            for (int k = 1; k < NW; k++) linfit::take_better(v, bi, red_v[k * kTileD + tid], red_i[k * kTileD + tid]);
            const size_t at = ((size_t)gj * ntile + tile) * ndp + t0 + tid;
            slab_v[at] = v;
            slab_i[at] = bi;
        }
    }
}

// slab_v, slab_i as above for the draws [d0, d0 + nd); grp_v, grp_j, grp_c: [group][ndraw].  blockIdx.y = group
__global__ __launch_bounds__(256) void bootstrap_fold_kernel(const double *__restrict__ slab_v, const int *__restrict__ slab_i, int nk, int ntile,
                                                             int ndp, int d0, int nd, int ndraw, const int *__restrict__ failed,
                                                             double *__restrict__ grp_v, int *__restrict__ grp_j, int *__restrict__ grp_c)
{
    const int d = (int)(blockIdx.x * 256 + threadIdx.x), g = (int)blockIdx.y;
    if (d >= nd) return;
    double v = 0.0;
    int bj = -1, bc = -1;
    if (!failed[g])
        for (int j = 0; j < nk; j++)
            for (int t = 0; t < ntile; t++) {
                const size_t at = (((size_t)g * nk + j) * ntile + t) * ndp + d;
                const double v2 = slab_v[at];
                const int c2 = slab_i[at];
                if (c2 >= 0 && (bc < 0 || v2 < v)) { v = v2; bj = j; bc = c2; }         // (j, tile ascending: the first among equals)
            }
    const size_t o = (size_t)g * ndraw + d0 + d;
    grp_v[o] = bc >= 0 ? v : __longlong_as_double(0x7ff8000000000000LL);
    grp_j[o] = bj;
    grp_c[o] = bc;
}

// run_v, run_g, run_j, run_c [ndraw]: the running best of the run (NaN, -1 before the first chunk); g0: the chunk's first group
__global__ __launch_bounds__(256) void bootstrap_best_kernel(const double *__restrict__ grp_v, const int *__restrict__ grp_j,
                                                             const int *__restrict__ grp_c, int ng, int g0, int ndraw, double *__restrict__ run_v,
                                                             int *__restrict__ run_g, int *__restrict__ run_j, int *__restrict__ run_c)
{
    const int d = (int)(blockIdx.x * 256 + threadIdx.x);
    if (d >= ndraw) return;
    double v = run_v[d];
    int bg = run_g[d], bj = run_j[d], bc = run_c[d];
    for (int g = 0; g < ng; g++) {
        const size_t o = (size_t)g * ndraw + d;
        const double v2 = grp_v[o];
        const int c2 = grp_c[o];
        if (c2 >= 0 && (bc < 0 || v2 < v)) { v = v2; bg = g0 + g; bj = grp_j[o]; bc = c2; }   // (groups ascending, over the chunks too)
    }
    run_v[d] = v; run_g[d] = bg; run_j[d] = bj; run_c[d] = bc;
}

// what the call cannot do is refused before anything runs: everything the candidate time scan refuses, and what the draws add
static void check_setup(kiwi_hip_ctx *c, int K, const timescan::Offsets &of, const double *receiver_weight, const Boot &bt)
{
    refusing(kName, [&] {
        if (bt.ndraw < 1) throw std::runtime_error("ndraw = " + std::to_string(bt.ndraw) + "; at least one draw is needed");
        if (!bt.draw_weights || !bt.best_value || !bt.best_group || !bt.best_offset || !bt.best_cand || !bt.status)
            throw std::runtime_error("null draw_weights, best_value, best_group, best_offset, best_cand or status array");
        const int ngiven = (bt.group_value ? 1 : 0) + (bt.group_offset ? 1 : 0) + (bt.group_cand ? 1 : 0);
        if (ngiven != 0 && ngiven != 3) throw std::runtime_error("group_value, group_offset and group_cand are given all three or not at all");
        int idummy = 0; double ddummy = 0.0;               // (the parents' arrays: checked for null only)
        linfit_candidates_timescan::check_setup(c, K, of, linfit_timescan::Out{ &ddummy, &ddummy, &idummy, nullptr, nullptr, nullptr },
                                                linfit_candidates_timescan::Scan{ bt.x, bt.ncand, bt.outer_norm, 0, &idummy, &idummy, &ddummy, nullptr,
                                                                                  &idummy, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr });
        const size_t nrec = c->recv.size();
        if (nrec > (size_t)kMaxRec)
            throw std::runtime_error(std::to_string(nrec) + " receivers; a candidate's misfits of all receivers stay in LDS, which holds at most " +
                                     std::to_string(kMaxRec));
        if (receiver_weight)
            for (size_t r = 0; r < nrec; r++)
                if (!std::isfinite(receiver_weight[r])) throw std::runtime_error("receiver_weight of receiver " + std::to_string(r + 1) + " is not finite");
        for (size_t p = 0; p < (size_t)bt.ndraw * nrec; p++)
            if (!std::isfinite(bt.draw_weights[p]))
                throw std::runtime_error("draw_weights of draw " + std::to_string(p / nrec) + ", receiver " + std::to_string(p % nrec + 1) + " is not finite");
    });
}

// groups whose basis sources could not be discretised at all (nothing was uploaded for them): status 2, no best in any draw
static void fill_failed(size_t ngroup, const Boot &bt)
{
    std::fill(bt.status, bt.status + ngroup, 2);
    if (!bt.group_value) return;
    std::fill(bt.group_value, bt.group_value + ngroup * (size_t)bt.ndraw, std::numeric_limits<double>::quiet_NaN());
    std::fill(bt.group_offset, bt.group_offset + ngroup * (size_t)bt.ndraw, -1);
    std::fill(bt.group_cand, bt.group_cand + ngroup * (size_t)bt.ndraw, -1);
}

// the bests of one run folded into those of the call, in the total order; g: indices inside the run
static void merge(const Boot &bt, const double *v, const int *g, const int *j, const int *cd)
{
    std::unique_lock<std::mutex> lk;
    if (bt.mu) lk = std::unique_lock<std::mutex>(*bt.mu);
    for (int d = 0; d < bt.ndraw; d++) {
        if (cd[d] < 0) continue;
        const int g2 = bt.group0 + g[d];
        const double v1 = bt.best_value[d];
        const bool better = bt.best_cand[d] < 0 || v[d] < v1 ||
                            (v[d] == v1 && std::make_tuple(g2, j[d], cd[d]) < std::make_tuple(bt.best_group[d], bt.best_offset[d], bt.best_cand[d]));
        if (better) { bt.best_value[d] = v[d]; bt.best_group[d] = g2; bt.best_offset[d] = j[d]; bt.best_cand[d] = cd[d]; }
    }
}

template <int K>
static void launch_candidates(kiwi_hip_ctx *c, size_t nblocks, size_t dyn, const double *nbr, int nrec, int nk, const double *w, const double *x,
                              int ncand, int ntile, const double *rw, const double *ns, const double *cw, int ndraw, int d0, int nd, int ndp,
                              int l2, double *slab_v, int *slab_i)
{
    if (!(c->linfit_cand_boot_attr & (1u << K))) {         // (the attribute belongs to the function on this context's device)
        HIPCHECK(hipFuncSetAttribute(reinterpret_cast<const void *>(&linfit_candidates_bootstrap_kernel<K>),
                                     hipFuncAttributeMaxDynamicSharedMemorySize, kLdsBytes));
        c->linfit_cand_boot_attr |= 1u << K;
    }
    hipLaunchKernelGGL(linfit_candidates_bootstrap_kernel<K>, dim3((unsigned)nblocks), dim3(kCandThreads), dyn, c->stream, nbr, nrec, nk, w, x,
                       ncand, ntile, rw, ns, cw, ndraw, d0, nd, ndp, l2, slab_v, slab_i);
    HIPCHECK(hipGetLastError());
}

// the groups [isrc0, isrc0 + ngroup K) of the uploaded batch; adds its HIP-event times to c->linfit_cand_boot_ms.  The skeleton is
// linfit_candidates_timescan::run's: the halo put back on the way out, every source synthesised, chunks of whole groups
static void run(kiwi_hip_ctx *c, int isrc0, int ngroup, int K, const timescan::Offsets &of, const double *receiver_weight, int anarchy,
                const Boot &bt)
{
    check_setup(c, K, of, receiver_weight, bt);
    check_group_range(kName, c, isrc0, ngroup, K);
    if (ngroup == 0) return;
    const int nrec = (int)c->recv.size(), NN = linfit::nn_of(K), nk = of.nk, ndraw = bt.ndraw, l2 = bt.outer_norm == 2 ? 1 : 0;
    const int ntile = (bt.ncand + kCandThreads - 1) / kCandThreads;
    // the draws of one pass: all of them, unless the slab of ONE group would exceed the chunk bound; then whole tiles of draws
    const size_t slab_per_draw = (size_t)nk * ntile * (sizeof(double) + sizeof(int));
    int ndp = ndraw;
    if (slab_per_draw * (size_t)ndraw > c->chunk_bytes_limit)
        ndp = (int)std::min<size_t>((size_t)ndraw, std::max<size_t>(c->chunk_bytes_limit / slab_per_draw / kTileD, 1) * kTileD);
    if ((long long)nk * ntile > (1LL << 30))
        throw std::runtime_error(std::string(kName) + ": " + std::to_string(nk) + " offsets x " + std::to_string(ntile) + " candidate tiles exceed a launch");
    c->misfit_d.ensure((size_t)c->nsrc * c->nmis, &c->dev_bytes);
    c->global_d.ensure((size_t)c->nsrc, &c->dev_bytes);
    c->fuse_now = false;                                   // the plain synthetics go to memory
    timescan::HaloScope halo(c);
    halo.widen(of.max_abs());

    const std::vector<double> w = receiver_weights(c, receiver_weight);
    const std::vector<double> nanv((size_t)ndraw, std::numeric_limits<double>::quiet_NaN());
    const std::vector<int> nonev((size_t)ndraw, -1);
    std::vector<int> failed;
    DevBuf<double> w_d, nbr_d, coef_d, mis_d, piv_d, normal_d, x_d, cw_d, rw_d, b_d, ns_d, slabv_d, grpv_d, runv_d;
    DevBuf<int> st_d, best_d, failed_d, status_d, slabi_d, grpj_d, grpc_d, rung_d, runj_d, runc_d;
    w_d.alloc((size_t)nrec, &c->dev_bytes);
    x_d.alloc((size_t)bt.ncand * K, &c->dev_bytes);
    cw_d.alloc((size_t)ndraw * nrec, &c->dev_bytes);
    runv_d.alloc((size_t)ndraw, &c->dev_bytes); rung_d.alloc((size_t)ndraw, &c->dev_bytes);
    runj_d.alloc((size_t)ndraw, &c->dev_bytes); runc_d.alloc((size_t)ndraw, &c->dev_bytes);
    HIPCHECK(hipMemcpyAsync(w_d.p, w.data(), (size_t)nrec * sizeof(double), hipMemcpyHostToDevice, c->stream));
    HIPCHECK(hipMemcpyAsync(x_d.p, bt.x, (size_t)bt.ncand * K * sizeof(double), hipMemcpyHostToDevice, c->stream));
    HIPCHECK(hipMemcpyAsync(cw_d.p, bt.draw_weights, (size_t)ndraw * nrec * sizeof(double), hipMemcpyHostToDevice, c->stream));
    HIPCHECK(hipMemcpyAsync(runv_d.p, nanv.data(), (size_t)ndraw * sizeof(double), hipMemcpyHostToDevice, c->stream));
    for (int *p : { rung_d.p, runj_d.p, runc_d.p })
        HIPCHECK(hipMemcpyAsync(p, nonev.data(), (size_t)ndraw * sizeof(int), hipMemcpyHostToDevice, c->stream));
    HIPCHECK(hipStreamSynchronize(c->stream));

    const PooledEvents<6> ev(c);
    // per group: the sums by receiver and their fold at every offset, the slab of one pass, ns and the group's bests per draw, rw and b
    const size_t per_group = (size_t)nk * (nrec + 1) * NN * sizeof(double) + slab_per_draw * (size_t)ndp +
                             (size_t)ndraw * (2 * sizeof(double) + 2 * sizeof(int)) + (size_t)nrec * 2 * sizeof(double) + 2 * sizeof(int);
    const size_t dyn = lds_bytes(K, nrec);
    int g0 = 0;
    while (g0 < ngroup) {
        int ng = next_group_chunk(c, isrc0, g0, ngroup, K, 1, per_group, kNoSourceCap);
        ng = (int)std::min<long long>(ng, std::max<long long>((1LL << 30) / ((long long)nk * ntile), 1));       // (the candidate kernel's grid)
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

        failed.assign((size_t)ng, 0);
        for_each_failed_group(c, s0, ng, K, [&](int g) { failed[(size_t)g] = 1; });
        failed_d.ensure((size_t)ng, &c->dev_bytes); status_d.ensure((size_t)ng, &c->dev_bytes);
        rw_d.ensure((size_t)ng * nrec, &c->dev_bytes); b_d.ensure((size_t)ng * nrec, &c->dev_bytes);
        ns_d.ensure((size_t)ng * ndraw, &c->dev_bytes);
        slabv_d.ensure(nsolve * ntile * ndp, &c->dev_bytes); slabi_d.ensure(nsolve * ntile * ndp, &c->dev_bytes);
        grpv_d.ensure((size_t)ng * ndraw, &c->dev_bytes); grpj_d.ensure((size_t)ng * ndraw, &c->dev_bytes);
        grpc_d.ensure((size_t)ng * ndraw, &c->dev_bytes);
        HIPCHECK(hipMemcpyAsync(failed_d.p, failed.data(), (size_t)ng * sizeof(int), hipMemcpyHostToDevice, c->stream));
        hipLaunchKernelGGL(bootstrap_prepare_kernel, dim3((unsigned)ng), dim3(256), 0, c->stream, nbr_d.p, normal_d.p, NN, nrec, nk, w_d.p,
                           anarchy ? 1 : 0, l2, cw_d.p, ndraw, failed_d.p, rw_d.p, b_d.p, ns_d.p, status_d.p);
        HIPCHECK(hipGetLastError());
        for (int d0 = 0; d0 < ndraw; d0 += ndp) {
            const int nd = std::min(ndp, ndraw - d0);
            by_basis(K, [&](auto k) {
                launch_candidates<k.value>(c, nsolve * ntile, dyn, nbr_d.p, nrec, nk, w_d.p, x_d.p, bt.ncand, ntile, rw_d.p, ns_d.p, cw_d.p, ndraw,
                                           d0, nd, ndp, l2, slabv_d.p, slabi_d.p);
            });
            hipLaunchKernelGGL(bootstrap_fold_kernel, dim3((unsigned)((nd + 255) / 256), (unsigned)ng), dim3(256), 0, c->stream, slabv_d.p,
                               slabi_d.p, nk, ntile, ndp, d0, nd, ndraw, failed_d.p, grpv_d.p, grpj_d.p, grpc_d.p);
            HIPCHECK(hipGetLastError());
        }
        hipLaunchKernelGGL(bootstrap_best_kernel, dim3((unsigned)((ndraw + 255) / 256)), dim3(256), 0, c->stream, grpv_d.p, grpj_d.p, grpc_d.p,
                           ng, g0, ndraw, runv_d.p, rung_d.p, runj_d.p, runc_d.p);
        HIPCHECK(hipGetLastError());
        HIPCHECK(hipEventRecord(ev[4], c->stream));
        const Boot o = bt.at((size_t)g0);
        HIPCHECK(hipMemcpyAsync(o.status, status_d.p, (size_t)ng * sizeof(int), hipMemcpyDeviceToHost, c->stream));
        if (o.group_value) {
            HIPCHECK(hipMemcpyAsync(o.group_value, grpv_d.p, (size_t)ng * ndraw * sizeof(double), hipMemcpyDeviceToHost, c->stream));
            HIPCHECK(hipMemcpyAsync(o.group_offset, grpj_d.p, (size_t)ng * ndraw * sizeof(int), hipMemcpyDeviceToHost, c->stream));
            HIPCHECK(hipMemcpyAsync(o.group_cand, grpc_d.p, (size_t)ng * ndraw * sizeof(int), hipMemcpyDeviceToHost, c->stream));
        }
        HIPCHECK(hipEventRecord(ev[5], c->stream));
        HIPCHECK(hipStreamSynchronize(c->stream));
        for (int i = 0; i < 5; i++) ev.add_elapsed(c->linfit_cand_boot_ms, i, i, i + 1);
        g0 += ng;
    }
    std::vector<double> rv((size_t)ndraw);
    std::vector<int> rg((size_t)ndraw), rj((size_t)ndraw), rc((size_t)ndraw);
    HIPCHECK(hipEventRecord(ev[0], c->stream));
    HIPCHECK(hipMemcpyAsync(rv.data(), runv_d.p, (size_t)ndraw * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIPCHECK(hipMemcpyAsync(rg.data(), rung_d.p, (size_t)ndraw * sizeof(int), hipMemcpyDeviceToHost, c->stream));
    HIPCHECK(hipMemcpyAsync(rj.data(), runj_d.p, (size_t)ndraw * sizeof(int), hipMemcpyDeviceToHost, c->stream));
    HIPCHECK(hipMemcpyAsync(rc.data(), runc_d.p, (size_t)ndraw * sizeof(int), hipMemcpyDeviceToHost, c->stream));
    HIPCHECK(hipEventRecord(ev[1], c->stream));
    HIPCHECK(hipStreamSynchronize(c->stream));
    ev.add_elapsed(c->linfit_cand_boot_ms, 4, 0, 1);
    merge(bt, rv.data(), rg.data(), rj.data(), rc.data());
    leave_evaluated(c, isrc0, ngroup * K, 0);              // the plain evaluation of the basis sources was made on the way
}

// kiwi_hip_linear_fit_candidates_bootstrap_params piece by piece (PieceCall, kiwi_group_run.hpp): every piece's and device's run
// folds its bests into those of the call under bt.mu.  check_fn, run_fn: kiwi_waveform_candidates_bootstrap.hpp passes its own, the
// rest is the same
static PieceCall piece_call(int K, const timescan::Offsets &of, const double *receiver_weight, int anarchy, const Boot &bt,
                            decltype(&check_setup) check_fn = &check_setup, decltype(&run) run_fn = &run)
{
    return PieceCall{ K,
        [=](kiwi_hip_ctx *c) { check_fn(c, K, of, receiver_weight, bt); },
        [=](kiwi_hip_ctx *, int s0, int n) { fill_failed((size_t)(n / K), bt.at((size_t)(s0 / K))); },
        [=](kiwi_hip_ctx *c, int s0, int n) { run_fn(c, 0, n / K, K, of, receiver_weight, anarchy, bt.at((size_t)(s0 / K))); } };
}

} // namespace linfit_candidates_bootstrap
