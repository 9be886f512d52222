// kiwi_linfit_candidates_floating_bootstrap.hpp -- the bootstrap over the receivers of a candidate search under floating_l2norm, joint
// over group (location) and candidate (mechanism), without the [candidate][receiver] matrices: kiwi_hip_linear_fit_candidates_floating_
// bootstrap.  What it answers is DEFINED by two existing calls: kiwi_hip_linear_fit_candidates_floating writes receiver_misfit
// [ngroup][ncand][nrec], receiver_norm [ngroup][nrec] as floats and cand_shift [ngroup][ncand][nrec]; kiwi_hip_outer_misfits reads the
// first two as ngroup ncand sources of one slot per receiver and returns the best source of every draw; the winner's row of cand_shift
// is the draw's set of station delays.  The shift of a receiver is chosen per (candidate, receiver) before any weight is applied, so
// the draws do not interact with the shift search.  Included by kiwi_hip.hip behind kiwi_linfit_candidates_floating.hpp and
// kiwi_candidates_bootstrap.hpp (the draw walk, the norm side, the fold kernels with nk = 1, the caller's arrays and the run's: what
// the bootstraps share), under the same -ffp-contract=off; tests/linfit_candidates_floating_bootstrap_restatement.py composes the two
// restatements of the parents, and the GPU tests ask for bit identity with the host route.  Per chunk of whole groups, behind the
// unchanged linfit_gram_kernel, linfit_float_xcorr_kernel<K> and linfit_float_norm_kernel (nbr[g][receiver][NN],
// xc[g][receiver][max_ns][K + 1], nr[g][receiver] on the stream), this header's own:
//   float_bootstrap_prepare_kernel   one workgroup per group, from the floating norm: a receiver counts where n_r > 0;
//       N = counts ? (double)(float) n_r : 0 -- the norm passes through float as on the host route --; then the shared norm side.
//       status as the parent call has it (0; 1 no receiver counts; 2 for a group with a failed basis source, flagged by the host).
//   linfit_candidates_float_bootstrap_kernel<K>   one workgroup of kThreads lanes per (group, tile of kThreads candidates), a lane
//       owns ONE candidate with its x in registers.  Phase 1 is linfit_candidates_float_kernel's receiver walk: `quad` on G_r once, the
//       rows (b_r[q], R_r[q]) staged kFloatShiftStage at a time, float_scan's first minimum; (float) sqrt(min val) -- 0 for a receiver
//       that is skipped -- goes to LDS as sm[r][lane] (a wavefront's lanes on consecutive banks).  Phase 2 is the shared draw walk on
//       that column.
//   float_bootstrap_shift_kernel<K>   behind every chunk's bootstrap_best_kernel, one wavefront per draw, a lane per receiver
//       (strided): for a draw whose running winner lies in this chunk the winner's argmin of every receiver is recomputed with `quad`
//       and float_scan -- the expressions of phase 1, as linfit_candidates_float_fold_kernel recomputes best_shift -- into
//       run_shift[draw][receiver].  A later chunk that takes the draw over overwrites the row, so the row belongs to the final winner
//       and no chunk's sums are kept.  The same kernel writes group_shift, one row per (group, draw) of the chunk.
// A draw with every source excluded: NaN, -1, -1 and a row of zeros.

namespace linfit_candidates_floating_bootstrap {

using linfit::nn_of;
using candidates_bootstrap::Boot;
using candidates_bootstrap::kLdsBytes;
using linfit_candidates_floating::float_scan;
using linfit_candidates_floating::kFloatShiftStage;

constexpr int kThreads = 256;                       // candidates per workgroup
using Walk = candidates_bootstrap::WalkLds<kThreads>;
// LDS of the candidate kernel in front of and behind the walk's: G_r and the stage of shift rows, and a receiver's column of m
__host__ __device__ constexpr int lds_fixed(int K) { return (nn_of(K) + kFloatShiftStage * (K + 1)) * 8; }
constexpr int kLdsPerRec = kThreads * 4;
constexpr int kMaxRec = Walk::max_rec(lds_fixed(linfit::kMaxBasis), kLdsPerRec);
static_assert(kMaxRec == 131, "the layout holds 131 receivers, for every K");
static size_t lds_bytes(int K, int nrec) { return Walk::bytes(lds_fixed(K), kLdsPerRec, nrec); }

static const char *const kName = "linear_fit_candidates_floating_bootstrap";

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
        candidates_bootstrap::norm_side(in ? (double)(float)n : 0.0, w[r], anarchy, l2, rw_out[(size_t)g * nrec + r], b_out[(size_t)g * nrec + r]);
        if (in) any = 1;
    }
    candidates_bootstrap::draw_norms(b_out + (size_t)g * nrec, cw, nrec, ndraw, ns + (size_t)g * ndraw);
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
    constexpr int NN = K * (K + 1) / 2 + K + 1, M = K + 1;
    extern __shared__ double lds[];
    double *sg = lds;                                       // [NN]
    double *sx = sg + NN;                                   // [kFloatShiftStage][M]
    const Walk wl(sx + kFloatShiftStage * M, nrec);
    float *sm = (float *)wl.end();                          // [nrec][kThreads]
    const int tid = (int)threadIdx.x, tile = (int)(blockIdx.x % (unsigned)ntile);
    const size_t g = blockIdx.x / (unsigned)ntile;
    const int cand = tile * kThreads + tid;
    const bool live = cand < ncand;
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
    wl.load_rw(rw + g * nrec, nrec);
    candidates_bootstrap::draw_walk(wl, nrec, cw, ns + g * ndraw, d0, nd, ndp, l2, live, cand, g * ntile + tile, slab_v, slab_i,
                                    candidates_bootstrap::FloatColumn<kThreads>{ sm, wl.srw, l2 });
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
    candidates_bootstrap::check_draws(kName, c, candidates_bootstrap::Extra::shift, kMaxRec, receiver_weight, bt, [&] {
        int idummy = 0; double ddummy = 0.0;               // (the parent's arrays: checked for null only)
        linfit_candidates_floating::check_setup(c, K, linfit_candidates_floating::Floating{ bt.x, bt.ncand, bt.outer_norm, &idummy, &ddummy, &idummy,
                                                                                            &idummy, nullptr, nullptr, nullptr, nullptr });
    });
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
    c->misfit_d.ensure((size_t)c->nsrc * c->nmis, &c->dev_bytes);
    c->global_d.ensure((size_t)c->nsrc, &c->dev_bytes);
    const int proc_which = 2;                               // (the context refuses a misfit filter under a floating norm)
    c->fuse_now = can_fuse(c, proc_which, isrc0, ngroup * K);

    const std::vector<double> w = receiver_weights(c, receiver_weight);
    candidates_bootstrap::Run st(c, bt, nrec, 1, ntile, candidates_bootstrap::draws_per_pass(c, ndraw, 1, ntile));
    linfit_candidates_floating::Bufs fb;                    // (w, x, nbr, xc, nr of it: what the parent's launches read and write)
    DevBuf<int> status_d, grps_d, runs_d;                   // (the shift rows of the groups and of the running best: this family's own)
    fb.w.alloc((size_t)nrec, &c->dev_bytes);
    fb.x.alloc((size_t)bt.ncand * K, &c->dev_bytes);
    runs_d.alloc((size_t)ndraw * nrec, &c->dev_bytes);
    HIPCHECK(hipMemcpyAsync(fb.w.p, w.data(), (size_t)nrec * sizeof(double), hipMemcpyHostToDevice, c->stream));
    HIPCHECK(hipMemcpyAsync(fb.x.p, bt.x, (size_t)bt.ncand * K * sizeof(double), hipMemcpyHostToDevice, c->stream));
    HIPCHECK(hipMemsetAsync(runs_d.p, 0, (size_t)ndraw * nrec * sizeof(int), c->stream));
    st.begin();

    const PooledEvents<5> ev(c);
    // per group: the sums by receiver and per shift, the norm, the run's arrays, the status; the shift rows where the caller wants
    // them per group
    const size_t per_group = (size_t)nrec * ((size_t)NN + (size_t)max_ns * M + 1) * sizeof(double) + st.per_group() + sizeof(int) +
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

        st.ensure(ng);
        status_d.ensure((size_t)ng, &c->dev_bytes);
        if (bt.group_shift) grps_d.ensure(ngd * nrec, &c->dev_bytes);
        st.mark_failed(s0, ng, K);
        hipLaunchKernelGGL(linfit_candidates_floating::linfit_float_norm_kernel, dim3((unsigned)((ngr + 63) / 64)), dim3(64), 0, c->stream,
                           fb.xc.p, fb.w.p, c->recv_d.p, c->comps_d.p, nrec, max_ns, M, ng, fb.nr.p);
        HIPCHECK(hipGetLastError());
        hipLaunchKernelGGL(float_bootstrap_prepare_kernel, dim3((unsigned)ng), dim3(256), 0, c->stream, fb.nr.p, nrec, fb.w.p, anarchy ? 1 : 0,
                           l2, st.cw.p, ndraw, st.failed_d.p, st.rw.p, st.b.p, st.ns.p, status_d.p);
        HIPCHECK(hipGetLastError());
        for (int d0 = 0; d0 < ndraw; d0 += st.ndp) {
            const int nd = std::min(st.ndp, ndraw - d0);
            by_basis(K, [&](auto k) {
                launch_candidates<k.value>(c, (size_t)ng * ntile, dyn, fb.nbr.p, fb.xc.p, fb.nr.p, nrec, fb.x.p, bt.ncand, ntile, st.rw.p, st.ns.p,
                                           st.cw.p, ndraw, d0, nd, st.ndp, l2, st.slab_v.p, st.slab_i.p);
            });
            st.fold(ng, d0, nd);
        }
        st.best(g0, ng);
        by_basis(K, [&](auto k) {
            launch_shift<k.value>(c, 1, fb.nbr.p, fb.xc.p, fb.nr.p, nrec, fb.x.p, st.run_g.p, st.run_c.p, g0, ng, ndraw, runs_d.p);
            if (bt.group_shift)
                launch_shift<k.value>(c, ng, fb.nbr.p, fb.xc.p, fb.nr.p, nrec, fb.x.p, nullptr, st.grp_c.p, 0, ng, ndraw, grps_d.p);
        });
        HIPCHECK(hipEventRecord(ev[3], c->stream));
        HIPCHECK(hipMemcpyAsync(bt.status + g0, status_d.p, (size_t)ng * sizeof(int), hipMemcpyDeviceToHost, c->stream));
        st.download_groups(g0, ng);
        if (bt.group_shift)
            HIPCHECK(hipMemcpyAsync(bt.at((size_t)g0, (size_t)nrec).group_shift, grps_d.p, ngd * nrec * sizeof(int), hipMemcpyDeviceToHost, c->stream));
        HIPCHECK(hipEventRecord(ev[4], c->stream));
        HIPCHECK(hipStreamSynchronize(c->stream));
        for (int i = 0; i < 4; i++) ev.add_elapsed(c->linfit_cand_float_boot_ms, i, i, i + 1);
        g0 += ng;
    }
    st.finish(c->linfit_cand_float_boot_ms + 3, runs_d.p);
    leave_evaluated(c, isrc0, ngroup * K, proc_which);
}

// kiwi_hip_linear_fit_candidates_floating_bootstrap_params piece by piece
static PieceCall piece_call(int K, const double *receiver_weight, int anarchy, const Boot &bt)
{
    return candidates_bootstrap::piece_call(K, bt,
        [=](kiwi_hip_ctx *c, const Boot &b) { check_setup(c, K, receiver_weight, b); },
        [=](kiwi_hip_ctx *c, int ng, const Boot &b) { run(c, 0, ng, K, receiver_weight, anarchy, b); });
}

} // namespace linfit_candidates_floating_bootstrap
