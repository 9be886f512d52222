// kiwi_linfit_candidates_bootstrap.hpp -- the bootstrap over the receivers of a candidate search, joint over group (location), origin
// time and candidate (mechanism), without the [candidate][receiver] matrix: kiwi_hip_linear_fit_candidates_bootstrap.  What it
// answers is DEFINED by two existing calls: kiwi_hip_linear_fit_candidates_time_scan (free_scale = 0) writes receiver_misfit
// [ngroup][nk][ncand][nrec] and receiver_norm [ngroup][nrec] as floats, kiwi_hip_outer_misfits reads them as ngroup nk ncand sources
// of one slot per receiver and returns the best source of every draw.  Here a candidate's m_r stays in LDS between the quadratic form
// and the draw loop, and the norm side of the fold -- b, and the denominator of every draw -- is made once per group, because it does
// not depend on the candidate.  Included by kiwi_hip.hip behind kiwi_linfit_candidates_timescan.hpp and kiwi_candidates_bootstrap.hpp
// (the draw walk, the norm side, the fold kernels, the caller's arrays and the run's: what the bootstraps share), under the same
// -ffp-contract=off; tests/linfit_candidates_bootstrap_restatement.py composes the two restatements of the parents, and the GPU tests
// ask for bit identity with the host route.  Per chunk of whole groups, behind the unchanged linfit_scan_gram_kernel and
// linfit_solve_kernel (nbr[(g nk + j)][receiver][NN], normal[(g nk + j)][NN] on the stream), this header's own:
//   bootstrap_prepare_kernel   one workgroup per group.  From the rows of offset 0 (R_r does not depend on the offset), per receiver:
//       counted = w_r != 0 and R_r > 0;  N = counted ? (double)(float) sqrt(R_r) : 0 -- the norm passes through float as on the host
//       route --; then the shared norm side.  status as the candidate call has it (l2norm: folded R > 0; l1norm: a receiver counts;
//       2 for a group with a failed basis source, flagged by the host).
//   linfit_candidates_bootstrap_kernel<K>   one workgroup of kCandThreads lanes per ((g, j), tile of kCandThreads candidates), a
//       lane owns ONE candidate.  Phase 1 is pass 0 / pass 2 of candidates_body: rows staged in LDS, broadcast reads, receivers
//       ascending, linfit::quad, val = (R - 2 xb) + xgx clamped at 0, m = sqrt(val); (float) m -- 0 for a receiver that is not
//       counted -- goes to LDS as sm[r][lane].  Phase 2 is the draw walk on that column, and here, in this one kernel, its text
//       stands a second time, with the LDS pointers as plain locals in WalkLds' order: called through draw_walk / WalkLds the
//       compiler allots 66 instead of 98 VGPRs and unrolls phase 1 differently, and the bootstrap kernels' event time rose by
//       0.5 to 1 % against the parent, beyond the distance of two copies of the parent build
//       (profiles/candidates_bootstrap_refactor_speed.json).  With the text in place every instantiation has the parent's
//       instructions.  Whoever changes draw_walk changes this copy; the sizes (lds_bytes, kMaxRec) come from WalkLds either way.

namespace linfit_candidates_bootstrap {

using linfit::kCandThreads;
using candidates_bootstrap::Boot;
using candidates_bootstrap::kLdsBytes;
using Walk = candidates_bootstrap::WalkLds<kCandThreads>;

constexpr int kStage = 16;                          // receivers per stage of phase 1: 16 x NN x 8 bytes = 5.6 KiB at K = 8
// LDS of the candidate kernel in front of and behind the walk's: the row stage, and a receiver's column of m
__host__ __device__ constexpr int lds_fixed(int K) { return kStage * linfit::nn_of(K) * 8; }
constexpr int kLdsPerRec = kCandThreads * 4;
constexpr int kMaxRec = Walk::max_rec(lds_fixed(linfit::kMaxBasis), kLdsPerRec);
static_assert(kMaxRec == 128, "the layout holds 128 receivers, for every K");
static size_t lds_bytes(int K, int nrec) { return Walk::bytes(lds_fixed(K), kLdsPerRec, nrec); }

static const char *const kName = "linear_fit_candidates_bootstrap";

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
        candidates_bootstrap::norm_side(in ? (double)(float)sqrt(Rr) : 0.0, w[r], anarchy, l2, rw_out[(size_t)g * nrec + r],
                                        b_out[(size_t)g * nrec + r]);
        if (in) any = 1;
    }
    candidates_bootstrap::draw_norms(b_out + (size_t)g * nrec, cw, nrec, ndraw, ns + (size_t)g * ndraw);
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
    constexpr int NN = K * (K + 1) / 2 + K + 1, NW = Walk::NW, kTileD = candidates_bootstrap::kTileD;
    extern __shared__ double lds[];
    double *sq = lds;                                       // [kStage][NN]
    double *srw = sq + kStage * NN;                         // [nrec]          the walk's part, in WalkLds' order, and phase 2 below
    double *cs = srw + nrec;                                // [nrec][kTileD]  are this kernel's own text: see the head of the file
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
    for (int t0 = 0; t0 < nd; t0 += kTileD) {               // candidates_bootstrap::draw_walk's text with FloatColumn's a_r
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

// what the call cannot do is refused before anything runs: everything the candidate time scan refuses, and what the draws add
static void check_setup(kiwi_hip_ctx *c, int K, const timescan::Offsets &of, const double *receiver_weight, const Boot &bt)
{
    candidates_bootstrap::check_draws(kName, c, candidates_bootstrap::Extra::offset, kMaxRec, receiver_weight, bt, [&] {
        int idummy = 0; double ddummy = 0.0;               // (the parents' arrays: checked for null only)
        linfit_candidates_timescan::check_setup(c, K, of, linfit_timescan::Out{ &ddummy, &ddummy, &idummy, nullptr, nullptr, nullptr },
                                                linfit_candidates_timescan::Scan{ bt.x, bt.ncand, bt.outer_norm, 0, &idummy, &idummy, &ddummy, nullptr,
                                                                                  &idummy, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr });
    });
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
    if ((long long)nk * ntile > (1LL << 30))
        throw std::runtime_error(std::string(kName) + ": " + std::to_string(nk) + " offsets x " + std::to_string(ntile) + " candidate tiles exceed a launch");
    c->misfit_d.ensure((size_t)c->nsrc * c->nmis, &c->dev_bytes);
    c->global_d.ensure((size_t)c->nsrc, &c->dev_bytes);
    c->fuse_now = false;                                   // the plain synthetics go to memory
    timescan::HaloScope halo(c);
    halo.widen(of.max_abs());

    const std::vector<double> w = receiver_weights(c, receiver_weight);
    candidates_bootstrap::Run st(c, bt, nrec, nk, ntile, candidates_bootstrap::draws_per_pass(c, ndraw, nk, ntile));
    DevBuf<double> w_d, nbr_d, coef_d, mis_d, piv_d, normal_d, x_d;
    DevBuf<int> st_d, best_d, status_d;
    w_d.alloc((size_t)nrec, &c->dev_bytes);
    x_d.alloc((size_t)bt.ncand * K, &c->dev_bytes);
    HIPCHECK(hipMemcpyAsync(w_d.p, w.data(), (size_t)nrec * sizeof(double), hipMemcpyHostToDevice, c->stream));
    HIPCHECK(hipMemcpyAsync(x_d.p, bt.x, (size_t)bt.ncand * K * sizeof(double), hipMemcpyHostToDevice, c->stream));
    st.begin();

    const PooledEvents<6> ev(c);
    // per group: the sums by receiver and their fold at every offset, the run's arrays, the status
    const size_t per_group = (size_t)nk * (nrec + 1) * NN * sizeof(double) + st.per_group() + sizeof(int);
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

        st.ensure(ng);
        status_d.ensure((size_t)ng, &c->dev_bytes);
        st.mark_failed(s0, ng, K);
        hipLaunchKernelGGL(bootstrap_prepare_kernel, dim3((unsigned)ng), dim3(256), 0, c->stream, nbr_d.p, normal_d.p, NN, nrec, nk, w_d.p,
                           anarchy ? 1 : 0, l2, st.cw.p, ndraw, st.failed_d.p, st.rw.p, st.b.p, st.ns.p, status_d.p);
        HIPCHECK(hipGetLastError());
        for (int d0 = 0; d0 < ndraw; d0 += st.ndp) {
            const int nd = std::min(st.ndp, ndraw - d0);
            by_basis(K, [&](auto k) {
                launch_candidates<k.value>(c, nsolve * ntile, dyn, nbr_d.p, nrec, nk, w_d.p, x_d.p, bt.ncand, ntile, st.rw.p, st.ns.p, st.cw.p, ndraw,
                                           d0, nd, st.ndp, l2, st.slab_v.p, st.slab_i.p);
            });
            st.fold(ng, d0, nd);
        }
        st.best(g0, ng);
        HIPCHECK(hipEventRecord(ev[4], c->stream));
        HIPCHECK(hipMemcpyAsync(bt.status + g0, status_d.p, (size_t)ng * sizeof(int), hipMemcpyDeviceToHost, c->stream));
        st.download_groups(g0, ng);
        HIPCHECK(hipEventRecord(ev[5], c->stream));
        HIPCHECK(hipStreamSynchronize(c->stream));
        for (int i = 0; i < 5; i++) ev.add_elapsed(c->linfit_cand_boot_ms, i, i, i + 1);
        g0 += ng;
    }
    st.finish(c->linfit_cand_boot_ms + 4);
    leave_evaluated(c, isrc0, ngroup * K, 0);              // the plain evaluation of the basis sources was made on the way
}

// kiwi_hip_linear_fit_candidates_bootstrap_params piece by piece
static PieceCall piece_call(int K, const timescan::Offsets &of, const double *receiver_weight, int anarchy, const Boot &bt)
{
    return candidates_bootstrap::piece_call(K, bt,
        [=](kiwi_hip_ctx *c, const Boot &b) { check_setup(c, K, of, receiver_weight, b); },
        [=](kiwi_hip_ctx *c, int ng, const Boot &b) { run(c, 0, ng, K, of, receiver_weight, anarchy, b); });
}

} // namespace linfit_candidates_bootstrap
