// kiwi_linfit_candidates_floating_bootstrap.hpp -- the bootstrap over the receivers of a candidate search under floating_l2norm, joint
// over group (location) and candidate (mechanism), without the [candidate][receiver] matrices: kiwi_hip_linear_fit_candidates_floating_
// bootstrap.  What it answers is DEFINED by two existing calls: kiwi_hip_linear_fit_candidates_floating writes receiver_misfit
// [ngroup][ncand][nrec], receiver_norm [ngroup][nrec] as floats and cand_shift [ngroup][ncand][nrec]; kiwi_hip_outer_misfits reads the
// first two as ngroup ncand sources of one slot per receiver and returns the best source of every draw; the winner's row of cand_shift
// is the draw's set of station delays.  The shift of a receiver is chosen per (candidate, receiver) before any weight is applied, so
// the draws do not interact with the shift search.  Included by kiwi_hip.hip behind kiwi_linfit_candidates_floating.hpp and
// kiwi_linfit_candidates_bootstrap.hpp, under the same -ffp-contract=off: every fp64 operation below is rounded on its own;
// tests/linfit_candidates_floating_bootstrap_restatement.py composes the two restatements of the parents, and the GPU tests ask for
// bit identity with the host route.  Per chunk of whole groups, behind the unchanged linfit_gram_kernel, linfit_float_xcorr_kernel<K>
// and linfit_float_norm_kernel (nbr[g][receiver][NN], xc[g][receiver][max_ns][K + 1], nr[g][receiver] on the stream):
//   float_bootstrap_prepare_kernel   bootstrap_prepare_kernel's sibling, one workgroup per group, from the floating norm: a receiver
//       counts where n_r > 0;  N = counts ? (double)(float) n_r : 0 -- the norm passes through float as on the host route --;  rw, b
//       and the denominator ns of every draw as the sibling makes them.  status as the parent call has it (0; 1 no receiver counts; 2 for
//       a group with a failed basis source, flagged by the host).
//   linfit_candidates_float_bootstrap_kernel<K>   one workgroup of kThreads lanes per (group, tile of kThreads candidates), a lane
//       owns ONE candidate with its x in registers.  Phase 1 is linfit_candidates_float_kernel's receiver walk: `quad` on G_r once, the
//       rows (b_r[q], R_r[q]) staged kFloatShiftStage at a time, float_scan's first minimum; (float) sqrt(min val) -- 0 for a receiver
//       that is skipped -- goes to LDS as sm[r][lane] (a wavefront's lanes on consecutive banks).  Phase 2 is
//       linfit_candidates_bootstrap_kernel's draw walk: the weight rows staged as cs[r][t] in tiles of kTileD draws; a = mv rw_r,
//       squared under l2norm; ms_t = ms_t + a c_rt from zero, r ascending; v = ms / ns (root under l2norm), excluded (NaN) where not
//       ns > 0 or not v >= 0.  (value, candidate) folded over wavefront and workgroup; the tile's best of every draw goes to
//       slab_v, slab_i[g][tile][draw of the pass].  Nothing per candidate goes to global memory.
//   bootstrap_fold_kernel, bootstrap_best_kernel   the Gram sibling's, unchanged, with nk = 1.
//   float_bootstrap_shift_kernel<K>   behind every chunk's bootstrap_best_kernel, one wavefront per draw, a lane per receiver
//       (strided): for a draw whose running winner lies in this chunk the winner's argmin of every receiver is recomputed with `quad`
//       and float_scan -- the expressions of phase 1, as linfit_candidates_float_fold_kernel recomputes best_shift -- into
//       run_shift[draw][receiver].  A later chunk that takes the draw over overwrites the row, so the row belongs to the final winner
//       and no chunk's sums are kept.  The same kernel writes group_shift, one row per (group, draw) of the chunk.
// The order of "best" is total -- excluded last, then the smaller value, then the lowest (g, c) --, so no answer depends on tiles, draw
// passes, chunks, pieces or devices.  No atomics.  A draw with every source excluded: NaN, -1, -1 and a row of zeros.

namespace linfit_candidates_floating_bootstrap {

using linfit::nn_of;
using linfit_candidates_bootstrap::kTileD;
using linfit_candidates_floating::float_scan;
using linfit_candidates_floating::kFloatShiftStage;

constexpr int kThreads = 256;                       // candidates per workgroup
constexpr int kLdsBytes = 152 * 1024;               // of the 160 KiB a workgroup may hold
// LDS of the candidate kernel: what does not grow with the receivers (G_r, the stage of shift rows, the wavefronts' bests) and what one
// receiver adds (its column of m, its weight row of a draw tile, its rw)
__host__ __device__ constexpr int lds_fixed(int K) { return (nn_of(K) + kFloatShiftStage * (K + 1)) * 8 + (kThreads / 64) * kTileD * 12; }
constexpr int kLdsPerRec = kThreads * 4 + kTileD * 8 + 8;
constexpr int kMaxRec = (kLdsBytes - lds_fixed(linfit::kMaxBasis)) / kLdsPerRec;       // 131, for every K
static_assert(kMaxRec >= 64, "the layout must hold 64 receivers");
static size_t lds_bytes(int K, int nrec) { return (size_t)lds_fixed(K) + (size_t)nrec * kLdsPerRec; }

static const char *const kName = "linear_fit_candidates_floating_bootstrap";

// host arrays of the caller for the groups of ONE call of run(): status [group]; group_value, group_cand [group][ndraw] and group_shift
// [group][ndraw][nrec], all three or none.  best_value, best_group, best_cand [ndraw] and best_shift [ndraw][nrec] belong to the WHOLE
// call: the caller fills them with NaN / -1 / 0 (begin), every run() folds its own bests into them with `group0` added to its group
// indices, under `mu` where runs of several devices share them.  x [ncand][K] and draw_weights [ndraw][nrec] are shared by all groups
struct Boot {
    const double *x; int ncand, outer_norm, ndraw; const double *draw_weights;
    double *best_value; int *best_group, *best_cand, *best_shift;
    int *status;
    double *group_value; int *group_cand, *group_shift;
    int group0; std::mutex *mu;
    Boot at(size_t g, size_t nrec) const
    {
        Boot b = *this;
        b.status += g; b.group0 += (int)g;
        if (group_value) { b.group_value += g * (size_t)ndraw; b.group_cand += g * (size_t)ndraw; b.group_shift += g * (size_t)ndraw * nrec; }
        return b;
    }
    void begin(size_t nrec) const
    {
        std::fill(best_value, best_value + ndraw, std::numeric_limits<double>::quiet_NaN());
        std::fill(best_group, best_group + ndraw, -1); std::fill(best_cand, best_cand + ndraw, -1);
        std::fill(best_shift, best_shift + (size_t)ndraw * nrec, 0);
    }
};

// nr: [group][nrec] the floating norm, 0 for a receiver that does not count; w: [nrec]; cw: [ndraw][nrec]; failed: [group].  rw, b:
// [group][nrec]; ns: [group][ndraw]; status: [group].  blockIdx.x = group
__global__ __launch_bounds__(256) void float_bootstrap_prepare_kernel(const double *__restrict__ nr, int nrec, const double *__restrict__ w,
                                                                      int anarchy, int l2, const double *__restrict__ cw, int ndraw,
                                                                      const int *__restrict__ failed, double *__restrict__ rw_out,
                                                                      double *__restrict__ b_out, double *__restrict__ ns,
                                                                      int *__restrict__ status)
{
    __shared__ int any;
    const int g = (int)blockIdx.x, tid = (int)threadIdx.x;
    if (tid == 0) any = 0;
    __syncthreads();
    for (int r = tid; r < nrec; r += 256) {
        const double n = nr[(size_t)g * nrec + r];
        const bool in = n > 0.0;
        const double N = in ? (double)(float)n : 0.0;
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
    if (tid == 0) status[g] = failed[g] ? 2 : any != 0 ? 0 : 1;
}

// nbr: [group][nrec][NN] (G_r of it), xc: [group][nrec][max_ns][K + 1], nr: [group][nrec], x: [ncand][K]; rw: [group][nrec]; ns:
// [group][ndraw]; cw: [ndraw][nrec].  The draws [d0, d0 + nd) of this pass; slab_v, slab_i: [group][ntile][ndp].  blockIdx.x =
// g ntile + tile.  Dynamic LDS: lds_bytes(K, nrec)
template <int K>
__global__ __launch_bounds__(kThreads) void linfit_candidates_float_bootstrap_kernel(
    const double *__restrict__ nbr, const double *__restrict__ xc, const double *__restrict__ nr, const RecvDev *__restrict__ recv,
    const CompDev *__restrict__ comps, int nrec, int max_ns, const double *__restrict__ x, int ncand, int ntile,
    const double *__restrict__ rw, const double *__restrict__ ns, const double *__restrict__ cw, int ndraw, int d0, int nd, int ndp, int l2,
    double *__restrict__ slab_v, int *__restrict__ slab_i)
{
    constexpr int NN = K * (K + 1) / 2 + K + 1, M = K + 1, NW = kThreads / 64;
    extern __shared__ double lds[];
    double *sg = lds;                                       // [NN]
    double *sx = sg + NN;                                   // [kFloatShiftStage][M]
    double *srw = sx + kFloatShiftStage * M;                // [nrec]
    double *cs = srw + nrec;                                // [nrec][kTileD]
    double *red_v = cs + (size_t)nrec * kTileD;             // [NW][kTileD]
    int *red_i = (int *)(red_v + NW * kTileD);              // [NW][kTileD]
    float *sm = (float *)(red_i + NW * kTileD);             // [nrec][kThreads]
    const int tid = (int)threadIdx.x, tile = (int)(blockIdx.x % (unsigned)ntile);
    const size_t g = blockIdx.x / (unsigned)ntile;
    const int cand = tile * kThreads + tid;
    const bool live = cand < ncand;
    const double nan = __longlong_as_double(0x7ff8000000000000LL);
    {
        double xv[K];
#pragma unroll
        for (int i = 0; i < K; i++) xv[i] = live ? x[(size_t)cand * K + i] : 0.0;
        for (int r = 0; r < nrec; r++) {                    // (everything that decides a branch here is the same for all lanes)
            const double n = nr[g * nrec + r];
            if (!(n > 0.0)) { sm[r * kThreads + tid] = 0.f; continue; }
            const int ns_r = comps[recv[r].slot0].fl_ns;
            const double *__restrict__ grow = nbr + (g * nrec + r) * NN;
            const double *__restrict__ xrow = xc + (g * nrec + r) * max_ns * M;
            double xgx = 0.0, minv = 0.0;
            int arg = -1;
            for (int q0 = 0; q0 < ns_r; q0 += kFloatShiftStage) {
                const int nq = ns_r - q0 < kFloatShiftStage ? ns_r - q0 : kFloatShiftStage;
                __syncthreads();                            // the stage before this one has been read by every wavefront
                if (q0 == 0 && tid < NN) sg[tid] = grow[tid];
                for (int p = tid; p < nq * M; p += kThreads) sx[p] = xrow[(size_t)q0 * M + p];
                __syncthreads();
                if (q0 == 0) {
                    double xb0;
                    linfit::quad<K>(sg, xv, xb0, xgx);
                }
                float_scan<K>(sx, nq, q0, xv, xgx, minv, arg);
            }
            sm[r * kThreads + tid] = (float)sqrt(minv);
        }
    }
    for (int r = tid; r < nrec; r += kThreads) srw[r] = rw[g * nrec + r];
    const int lane = tid & 63, wave = tid >> 6;
    for (int t0 = 0; t0 < nd; t0 += kTileD) {
        __syncthreads();                                    // (srw; the weight rows and the bests of the tile before)
        for (int i = tid; i < nrec * kTileD; i += kThreads) {
            const int t = i / nrec, r = i - t * nrec;
            cs[r * kTileD + t] = t0 + t < nd ? cw[(size_t)(d0 + t0 + t) * nrec + r] : 0.0;
        }
        __syncthreads();
        double ms[kTileD];
#pragma unroll
        for (int t = 0; t < kTileD; t++) ms[t] = 0.0;
        for (int r = 0; r < nrec; r++) {
            const double mv = (double)sm[r * kThreads + tid];
            double av = mv * srw[r];
            if (l2) av = av * av;
            const double *c = cs + r * kTileD;
#pragma unroll
            for (int t = 0; t < kTileD; t++) ms[t] = ms[t] + av * c[t];
        }
#pragma unroll
        for (int t = 0; t < kTileD; t++) {
            const double den = t0 + t < nd ? ns[g * ndraw + d0 + t0 + t] : 0.0;
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
            const size_t at = (g * ntile + tile) * ndp + t0 + tid;
            slab_v[at] = v;
            slab_i[at] = bi;
        }
    }
}

// the shifts of a winner, one row of out[blockIdx.y][ndraw][nrec] per wavefront; blockIdx.x = draw.  sel_c: [gridDim.y][ndraw], the
// winner's candidate, -1: none.  With sel_g ([ndraw], group indices of the whole run; gridDim.y = 1) only the draws whose winner lies
// in the chunk's groups [g0, g0 + ng) are written; without it blockIdx.y is the chunk's group and every row is written
template <int K>
__global__ __launch_bounds__(64) void float_bootstrap_shift_kernel(const double *__restrict__ nbr, const double *__restrict__ xc,
                                                                   const double *__restrict__ nr, const RecvDev *__restrict__ recv,
                                                                   const CompDev *__restrict__ comps, int nrec, int max_ns,
                                                                   const double *__restrict__ x, const int *__restrict__ sel_g,
                                                                   const int *__restrict__ sel_c, int g0, int ng, int ndraw,
                                                                   int *__restrict__ out)
{
    constexpr int NN = K * (K + 1) / 2 + K + 1, M = K + 1;
    const int d = (int)blockIdx.x, lane = (int)threadIdx.x;
    const size_t row = (size_t)blockIdx.y * ndraw + d;
    const int bi = sel_c[row];
    int g = (int)blockIdx.y;
    if (sel_g) {
        g = sel_g[d] - g0;
        if (bi < 0 || g < 0 || g >= ng) return;
    }
    double xv[K];
#pragma unroll
    for (int i = 0; i < K; i++) xv[i] = bi >= 0 ? x[(size_t)bi * K + i] : 0.0;
    for (int r = lane; r < nrec; r += 64) {
        const double n = nr[(size_t)g * nrec + r];
        int sh = 0;
        if (n > 0.0 && bi >= 0) {
            const CompDev c0 = comps[recv[r].slot0];
            double xb0, xgx, minv = 0.0;
            int arg = -1;
            linfit::quad<K>(nbr + ((size_t)g * nrec + r) * NN, xv, xb0, xgx);
            float_scan<K>(xc + ((size_t)g * nrec + r) * max_ns * M, c0.fl_ns, 0, xv, xgx, minv, arg);
            sh = c0.fl_lo + arg;
        }
        out[row * nrec + r] = sh;
    }
}

// what the call cannot do is refused before anything runs: everything the parent call refuses of the set-up (a shift range beyond 16
// bits is not among it: that belongs to the parent's cand_shift array), and what the draws add.  Leaves the context prepared
static void check_setup(kiwi_hip_ctx *c, int K, const double *receiver_weight, const Boot &bt)
{
    refusing(kName, [&] {
        if (bt.ndraw < 1) throw std::runtime_error("ndraw = " + std::to_string(bt.ndraw) + "; at least one draw is needed");
        if (!bt.draw_weights || !bt.best_value || !bt.best_group || !bt.best_cand || !bt.best_shift || !bt.status)
            throw std::runtime_error("null draw_weights, best_value, best_group, best_cand, best_shift or status array");
        const int ngiven = (bt.group_value ? 1 : 0) + (bt.group_cand ? 1 : 0) + (bt.group_shift ? 1 : 0);
        if (ngiven != 0 && ngiven != 3) throw std::runtime_error("group_value, group_cand and group_shift are given all three or not at all");
        int idummy = 0; double ddummy = 0.0;               // (the parent's arrays: checked for null only)
        linfit_candidates_floating::check_setup(c, K, linfit_candidates_floating::Floating{ bt.x, bt.ncand, bt.outer_norm, &idummy, &ddummy, &idummy,
                                                                                            &idummy, nullptr, nullptr, nullptr, nullptr });
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
static void fill_failed(size_t ngroup, size_t nrec, const Boot &bt)
{
    std::fill(bt.status, bt.status + ngroup, 2);
    if (!bt.group_value) return;
    std::fill(bt.group_value, bt.group_value + ngroup * (size_t)bt.ndraw, std::numeric_limits<double>::quiet_NaN());
    std::fill(bt.group_cand, bt.group_cand + ngroup * (size_t)bt.ndraw, -1);
    std::fill(bt.group_shift, bt.group_shift + ngroup * (size_t)bt.ndraw * nrec, 0);
}

// the bests of one run folded into those of the call, in the total order, the winner's shift row with it; g: indices inside the run
static void merge(const Boot &bt, size_t nrec, const double *v, const int *g, const int *cd, const int *shift)
{
    std::unique_lock<std::mutex> lk;
    if (bt.mu) lk = std::unique_lock<std::mutex>(*bt.mu);
    for (int d = 0; d < bt.ndraw; d++) {
        if (cd[d] < 0) continue;
        const int g2 = bt.group0 + g[d];
        const double v1 = bt.best_value[d];
        const bool better = bt.best_cand[d] < 0 || v[d] < v1 ||
                            (v[d] == v1 && std::make_tuple(g2, cd[d]) < std::make_tuple(bt.best_group[d], bt.best_cand[d]));
        if (!better) continue;
        bt.best_value[d] = v[d]; bt.best_group[d] = g2; bt.best_cand[d] = cd[d];
        std::copy(shift + (size_t)d * nrec, shift + (size_t)(d + 1) * nrec, bt.best_shift + (size_t)d * nrec);
    }
}

template <int K>
static void launch_candidates(kiwi_hip_ctx *c, size_t nblocks, size_t dyn, const double *nbr, const double *xc, const double *nr, int nrec,
                              const double *x, int ncand, int ntile, const double *rw, const double *ns, const double *cw, int ndraw, int d0,
                              int nd, int ndp, int l2, double *slab_v, int *slab_i)
{
    if (!(c->linfit_cand_float_boot_attr & (1u << K))) {   // (the attribute belongs to the function on this context's device)
        HIPCHECK(hipFuncSetAttribute(reinterpret_cast<const void *>(&linfit_candidates_float_bootstrap_kernel<K>),
                                     hipFuncAttributeMaxDynamicSharedMemorySize, kLdsBytes));
        c->linfit_cand_float_boot_attr |= 1u << K;
    }
    hipLaunchKernelGGL(linfit_candidates_float_bootstrap_kernel<K>, dim3((unsigned)nblocks), dim3(kThreads), dyn, c->stream, nbr, xc, nr,
                       c->recv_d.p, c->comps_d.p, nrec, c->max_ns, x, ncand, ntile, rw, ns, cw, ndraw, d0, nd, ndp, l2, slab_v, slab_i);
    HIPCHECK(hipGetLastError());
}

template <int K>
static void launch_shift(kiwi_hip_ctx *c, int nrows_y, const double *nbr, const double *xc, const double *nr, int nrec, const double *x,
                         const int *sel_g, const int *sel_c, int g0, int ng, int ndraw, int *out)
{
    hipLaunchKernelGGL(float_bootstrap_shift_kernel<K>, dim3((unsigned)ndraw, (unsigned)nrows_y), dim3(64), 0, c->stream, nbr, xc, nr,
                       c->recv_d.p, c->comps_d.p, nrec, c->max_ns, x, sel_g, sel_c, g0, ng, ndraw, out);
    HIPCHECK(hipGetLastError());
}

// the groups [isrc0, isrc0 + ngroup K) of the uploaded batch: the front of linfit_candidates_floating::run (the floating evaluation
// with the tapered synthetics kept, the Gram and xcorr kernels), the bootstrap kernels behind.  Adds its HIP-event times to
// c->linfit_cand_float_boot_ms: evaluation, Gram + xcorr kernels, bootstrap kernels, downloads
static void run(kiwi_hip_ctx *c, int isrc0, int ngroup, int K, const double *receiver_weight, int anarchy, const Boot &bt)
{
    check_setup(c, K, receiver_weight, bt);
    check_group_range(kName, c, isrc0, ngroup, K);
    if (ngroup == 0) return;
    const int nrec = (int)c->recv.size(), NN = nn_of(K), M = K + 1, max_ns = c->max_ns, ndraw = bt.ndraw, l2 = bt.outer_norm == 2 ? 1 : 0;
    const int ntile = (bt.ncand + kThreads - 1) / kThreads;
    // the draws of one pass: all of them, unless the slab of ONE group would exceed the chunk bound; then whole tiles of draws
    const size_t slab_per_draw = (size_t)ntile * (sizeof(double) + sizeof(int));
    int ndp = ndraw;
    if (slab_per_draw * (size_t)ndraw > c->chunk_bytes_limit)
        ndp = (int)std::min<size_t>((size_t)ndraw, std::max<size_t>(c->chunk_bytes_limit / slab_per_draw / kTileD, 1) * kTileD);
    c->misfit_d.ensure((size_t)c->nsrc * c->nmis, &c->dev_bytes);
    c->global_d.ensure((size_t)c->nsrc, &c->dev_bytes);
    const int proc_which = 2;                               // (the context refuses a misfit filter under a floating norm)
    c->fuse_now = can_fuse(c, proc_which, isrc0, ngroup * K);

    const std::vector<double> w = receiver_weights(c, receiver_weight);
    const std::vector<double> nanv((size_t)ndraw, std::numeric_limits<double>::quiet_NaN());
    const std::vector<int> nonev((size_t)ndraw, -1);
    std::vector<int> failed;
    linfit_candidates_floating::Bufs fb;                    // (w, x, nbr, xc, nr of it: what the parent's launches read and write)
    DevBuf<double> cw_d, rw_d, b_d, ns_d, slabv_d, grpv_d, runv_d;
    DevBuf<int> failed_d, status_d, slabi_d, grpj_d, grpc_d, grps_d, rung_d, runj_d, runc_d, runs_d;
    fb.w.alloc((size_t)nrec, &c->dev_bytes);
    fb.x.alloc((size_t)bt.ncand * K, &c->dev_bytes);
    cw_d.alloc((size_t)ndraw * nrec, &c->dev_bytes);
    runv_d.alloc((size_t)ndraw, &c->dev_bytes); rung_d.alloc((size_t)ndraw, &c->dev_bytes);
    runj_d.alloc((size_t)ndraw, &c->dev_bytes); runc_d.alloc((size_t)ndraw, &c->dev_bytes);
    runs_d.alloc((size_t)ndraw * nrec, &c->dev_bytes);
    HIPCHECK(hipMemcpyAsync(fb.w.p, w.data(), (size_t)nrec * sizeof(double), hipMemcpyHostToDevice, c->stream));
    HIPCHECK(hipMemcpyAsync(fb.x.p, bt.x, (size_t)bt.ncand * K * sizeof(double), hipMemcpyHostToDevice, c->stream));
    HIPCHECK(hipMemcpyAsync(cw_d.p, bt.draw_weights, (size_t)ndraw * nrec * sizeof(double), hipMemcpyHostToDevice, c->stream));
    HIPCHECK(hipMemcpyAsync(runv_d.p, nanv.data(), (size_t)ndraw * sizeof(double), hipMemcpyHostToDevice, c->stream));
    for (int *p : { rung_d.p, runj_d.p, runc_d.p })
        HIPCHECK(hipMemcpyAsync(p, nonev.data(), (size_t)ndraw * sizeof(int), hipMemcpyHostToDevice, c->stream));
    HIPCHECK(hipMemsetAsync(runs_d.p, 0, (size_t)ndraw * nrec * sizeof(int), c->stream));
    HIPCHECK(hipStreamSynchronize(c->stream));

    const PooledEvents<5> ev(c);
    // per group: the sums by receiver and per shift, the norm, rw and b, the slab of one pass, ns and the group's bests per draw, the
    // flags; the shift rows where the caller wants them per group
    const size_t per_group = (size_t)nrec * ((size_t)NN + (size_t)max_ns * M + 3) * sizeof(double) + slab_per_draw * (size_t)ndp +
                             (size_t)ndraw * (2 * sizeof(double) + 2 * sizeof(int)) + 2 * sizeof(int) +
                             (bt.group_shift ? (size_t)ndraw * nrec * sizeof(int) : 0);
    const size_t dyn = lds_bytes(K, nrec);
    int g0 = 0;
    while (g0 < ngroup) {
        int ng = next_group_chunk(c, isrc0, g0, ngroup, K, 3, per_group, kNoSourceCap);
        ng = (int)std::min<long long>(ng, std::max<long long>((1LL << 30) / ntile, 1));          // (the candidate kernel's grid)
        const int s0 = isrc0 + g0 * K;
        const size_t ngr = (size_t)ng * nrec, ngd = (size_t)ng * ndraw;
        HIPCHECK(hipEventRecord(ev[0], c->stream));
        run_chunk(c, s0, ng * K, proc_which);
        HIPCHECK(hipEventRecord(ev[1], c->stream));
        fb.nbr.ensure(ngr * NN, &c->dev_bytes);
        fb.xc.ensure(ngr * max_ns * M, &c->dev_bytes);
        fb.nr.ensure(ngr, &c->dev_bytes);
        HIPCHECK(hipMemsetAsync(fb.nbr.p, 0, ngr * NN * sizeof(double), c->stream));
        HIPCHECK(hipMemsetAsync(fb.xc.p, 0, ngr * max_ns * M * sizeof(double), c->stream));
        linfit::launch_gram_any(c, K, ng, nullptr, fb.nbr.p);
        by_basis(K, [&](auto k) { linfit_candidates_floating::launch_xcorr<k.value>(c, ng, fb); });
        HIPCHECK(hipEventRecord(ev[2], c->stream));

        failed.assign((size_t)ng, 0);
        for_each_failed_group(c, s0, ng, K, [&](int g) { failed[(size_t)g] = 1; });
        failed_d.ensure((size_t)ng, &c->dev_bytes); status_d.ensure((size_t)ng, &c->dev_bytes);
        rw_d.ensure(ngr, &c->dev_bytes); b_d.ensure(ngr, &c->dev_bytes);
        ns_d.ensure(ngd, &c->dev_bytes);
        slabv_d.ensure((size_t)ng * ntile * ndp, &c->dev_bytes); slabi_d.ensure((size_t)ng * ntile * ndp, &c->dev_bytes);
        grpv_d.ensure(ngd, &c->dev_bytes); grpj_d.ensure(ngd, &c->dev_bytes); grpc_d.ensure(ngd, &c->dev_bytes);
        if (bt.group_shift) grps_d.ensure(ngd * nrec, &c->dev_bytes);
        HIPCHECK(hipMemcpyAsync(failed_d.p, failed.data(), (size_t)ng * sizeof(int), hipMemcpyHostToDevice, c->stream));
        hipLaunchKernelGGL(linfit_candidates_floating::linfit_float_norm_kernel, dim3((unsigned)((ngr + 63) / 64)), dim3(64), 0, c->stream,
                           fb.xc.p, fb.w.p, c->recv_d.p, c->comps_d.p, nrec, max_ns, M, ng, fb.nr.p);
        HIPCHECK(hipGetLastError());
        hipLaunchKernelGGL(float_bootstrap_prepare_kernel, dim3((unsigned)ng), dim3(256), 0, c->stream, fb.nr.p, nrec, fb.w.p, anarchy ? 1 : 0,
                           l2, cw_d.p, ndraw, failed_d.p, rw_d.p, b_d.p, ns_d.p, status_d.p);
        HIPCHECK(hipGetLastError());
        for (int d0 = 0; d0 < ndraw; d0 += ndp) {
            const int nd = std::min(ndp, ndraw - d0);
            by_basis(K, [&](auto k) {
                launch_candidates<k.value>(c, (size_t)ng * ntile, dyn, fb.nbr.p, fb.xc.p, fb.nr.p, nrec, fb.x.p, bt.ncand, ntile, rw_d.p, ns_d.p,
                                           cw_d.p, ndraw, d0, nd, ndp, l2, slabv_d.p, slabi_d.p);
            });
            hipLaunchKernelGGL(linfit_candidates_bootstrap::bootstrap_fold_kernel, dim3((unsigned)((nd + 255) / 256), (unsigned)ng), dim3(256), 0,
                               c->stream, slabv_d.p, slabi_d.p, 1, ntile, ndp, d0, nd, ndraw, failed_d.p, grpv_d.p, grpj_d.p, grpc_d.p);
            HIPCHECK(hipGetLastError());
        }
        hipLaunchKernelGGL(linfit_candidates_bootstrap::bootstrap_best_kernel, dim3((unsigned)((ndraw + 255) / 256)), dim3(256), 0, c->stream,
                           grpv_d.p, grpj_d.p, grpc_d.p, ng, g0, ndraw, runv_d.p, rung_d.p, runj_d.p, runc_d.p);
        HIPCHECK(hipGetLastError());
        by_basis(K, [&](auto k) {
            launch_shift<k.value>(c, 1, fb.nbr.p, fb.xc.p, fb.nr.p, nrec, fb.x.p, rung_d.p, runc_d.p, g0, ng, ndraw, runs_d.p);
            if (bt.group_shift)
                launch_shift<k.value>(c, ng, fb.nbr.p, fb.xc.p, fb.nr.p, nrec, fb.x.p, nullptr, grpc_d.p, 0, ng, ndraw, grps_d.p);
        });
        HIPCHECK(hipEventRecord(ev[3], c->stream));
        const Boot o = bt.at((size_t)g0, (size_t)nrec);
        HIPCHECK(hipMemcpyAsync(o.status, status_d.p, (size_t)ng * sizeof(int), hipMemcpyDeviceToHost, c->stream));
        if (o.group_value) {
            HIPCHECK(hipMemcpyAsync(o.group_value, grpv_d.p, ngd * sizeof(double), hipMemcpyDeviceToHost, c->stream));
            HIPCHECK(hipMemcpyAsync(o.group_cand, grpc_d.p, ngd * sizeof(int), hipMemcpyDeviceToHost, c->stream));
            HIPCHECK(hipMemcpyAsync(o.group_shift, grps_d.p, ngd * nrec * sizeof(int), hipMemcpyDeviceToHost, c->stream));
        }
        HIPCHECK(hipEventRecord(ev[4], c->stream));
        HIPCHECK(hipStreamSynchronize(c->stream));
        for (int i = 0; i < 4; i++) ev.add_elapsed(c->linfit_cand_float_boot_ms, i, i, i + 1);
        g0 += ng;
    }
    std::vector<double> rv((size_t)ndraw);
    std::vector<int> rg((size_t)ndraw), rc((size_t)ndraw), rs((size_t)ndraw * nrec);
    HIPCHECK(hipEventRecord(ev[0], c->stream));
    HIPCHECK(hipMemcpyAsync(rv.data(), runv_d.p, (size_t)ndraw * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIPCHECK(hipMemcpyAsync(rg.data(), rung_d.p, (size_t)ndraw * sizeof(int), hipMemcpyDeviceToHost, c->stream));
    HIPCHECK(hipMemcpyAsync(rc.data(), runc_d.p, (size_t)ndraw * sizeof(int), hipMemcpyDeviceToHost, c->stream));
    HIPCHECK(hipMemcpyAsync(rs.data(), runs_d.p, (size_t)ndraw * nrec * sizeof(int), hipMemcpyDeviceToHost, c->stream));
    HIPCHECK(hipEventRecord(ev[1], c->stream));
    HIPCHECK(hipStreamSynchronize(c->stream));
    ev.add_elapsed(c->linfit_cand_float_boot_ms, 3, 0, 1);
    merge(bt, (size_t)nrec, rv.data(), rg.data(), rc.data(), rs.data());
    leave_evaluated(c, isrc0, ngroup * K, proc_which);
}

// kiwi_hip_linear_fit_candidates_floating_bootstrap_params piece by piece (PieceCall, kiwi_group_run.hpp): every piece's and device's
// run folds its bests, the shift rows with them, into those of the call under bt.mu
static PieceCall piece_call(int K, const double *receiver_weight, int anarchy, const Boot &bt)
{
    return PieceCall{ K,
        [=](kiwi_hip_ctx *c) { check_setup(c, K, receiver_weight, bt); },
        [=](kiwi_hip_ctx *c, int s0, int n) { fill_failed((size_t)(n / K), c->recv.size(), bt.at((size_t)(s0 / K), c->recv.size())); },
        [=](kiwi_hip_ctx *c, int s0, int n) { run(c, 0, n / K, K, receiver_weight, anarchy, bt.at((size_t)(s0 / K), c->recv.size())); } };
}

} // namespace linfit_candidates_floating_bootstrap
