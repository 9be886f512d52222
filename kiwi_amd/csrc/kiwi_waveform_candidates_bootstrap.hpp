// kiwi_waveform_candidates_bootstrap.hpp -- the bootstrap over the receivers of a waveform candidate search (l1norm or l2norm
// inside), joint over group (location), origin time and candidate (mechanism), without the [candidate][slot] array ever leaving the
// device: kiwi_hip_waveform_candidates_bootstrap.  What it answers is DEFINED by two existing calls:
// kiwi_hip_waveform_candidates_time_scan writes slot_misfit [ngroup][nk][ncand][nmis] and slot_norm [ngroup][nmis] as floats,
// kiwi_hip_outer_misfits reads them as ngroup nk ncand sources of nmis slots (slot m belongs to receiver slot_receiver[m]; the norm
// row of group g repeated for each of its sources) and returns the best source of every draw.  Here the scan's slab stays where
// wavecand_scan_kernel wrote it, [(group nk + j)][slot][candidate], and the norm side of the fold -- rw, b and the denominator of
// every draw -- is made once per group, because it depends neither on the candidate nor on the offset.  Included by kiwi_hip.hip
// behind kiwi_waveform_candidates_timescan.hpp and kiwi_candidates_bootstrap.hpp (the draw walk, the norm side, the fold kernels, the
// caller's arrays and the run's: what the bootstraps share) under the same -ffp-contract=off: every fp64 operation below is rounded on
// its own; tests/waveform_candidates_bootstrap_restatement.py composes the scan's slot arrays with tests/outer_restatement.py, and the
// GPU tests ask for bit identity with the host route.  Per chunk of whole groups, behind the unchanged rows, scan and fold kernels of
// the time scan (waveform_candidates_timescan::ChunkHook), this header's own:
//   wavecand_bootstrap_prepare_kernel   one workgroup per group.  Per receiver r, its slots k ascending (outer_prepare_kernel):
//       nv = (double) norm[k];  N = N + nv (l1norm outside) | N = N + nv nv, N = sqrt(N) behind the slots (l2norm); then the shared
//       norm side.  A receiver without slots has N = 0.
//   wavecand_bootstrap_kernel   one workgroup of kThreads lanes per ((g, j), tile of kThreads candidates), a lane owns ONE
//       candidate.  Phase 1 walks the slots of the slab ascending (a wavefront reads 64 consecutive floats of a slot) and folds them
//       per receiver: mv = (double) slab value;  M = M + mv | M = M + mv mv, M = sqrt(M);  a = M rw_r, squared under l2norm, to LDS
//       as sa[r][lane].  Phase 2 is the shared draw walk on that column.
// Zero scratch (profiles/waveform_candidates_bootstrap_kernel_resources.json).  A draw with every source excluded: NaN, -1, -1, -1 --
// the one difference from the host route, which answers NaN and index 0.  A group whose basis failed to discretise (status 2) or that
// no receiver counts for (status 1) has zero norms, so ns > 0 fails in every draw.  The kernels take slab, norms and the slot table as
// plain arguments: the floating and spectral families' slabs have the same layout.

namespace waveform_candidates_bootstrap {

using candidates_bootstrap::Boot;
using candidates_bootstrap::kLdsBytes;

constexpr int kThreads = 256;                       // candidates per workgroup, one per lane
using Walk = candidates_bootstrap::WalkLds<kThreads>;
// LDS of the candidate kernel in front of the walk's: a receiver's column of a
constexpr int kLdsPerRec = kThreads * 8;
constexpr int kMaxRec = Walk::max_rec(0, kLdsPerRec);
static_assert(kMaxRec == 70, "the layout holds 70 receivers");
static size_t lds_bytes(int nrec) { return Walk::bytes(0, kLdsPerRec, nrec); }

static const char *const kName = "waveform_candidates_bootstrap";

// norm: [group][nk][nmis] (read at offset 0: the norm factors do not depend on the offset); rec_first: [nrec + 1], the slots of
// receiver r are [rec_first[r], rec_first[r + 1]); w: [nrec]; cw: [ndraw][nrec].  rw, b: [group][nrec]; ns: [group][ndraw].
// blockIdx.x = group
__global__ __launch_bounds__(256) void wavecand_bootstrap_prepare_kernel(const float *__restrict__ norm, const int *__restrict__ rec_first,
                                                                         int nmis, int nrec, int nk, const double *__restrict__ w, int anarchy,
                                                                         int l2, const double *__restrict__ cw, int ndraw,
                                                                         double *__restrict__ rw_out, double *__restrict__ b_out,
                                                                         double *__restrict__ ns)
{
    const int g = (int)blockIdx.x, tid = (int)threadIdx.x;
    const float *__restrict__ n = norm + (size_t)g * nk * nmis;
    for (int r = tid; r < nrec; r += 256) {
        double N = 0.0;
        for (int k = rec_first[r]; k < rec_first[r + 1]; k++) {
            const double nv = (double)n[k];
            if (l2) N = N + nv * nv;
            else N = N + nv;
        }
        if (l2) N = sqrt(N);
        candidates_bootstrap::norm_side(N, w[r], anarchy, l2, rw_out[(size_t)g * nrec + r], b_out[(size_t)g * nrec + r]);
    }
    candidates_bootstrap::draw_norms(b_out + (size_t)g * nrec, cw, nrec, ndraw, ns + (size_t)g * ndraw);
}

// slab: [(group nk + j)][nmis][ncand]; rec_first as above; rw: [group][nrec]; ns: [group][ndraw]; cw: [ndraw][nrec]; failed:
// [group] (its slab was never written).  The draws [d0, d0 + nd) of this pass; slab_v, slab_i: [group nk][ntile][ndp].
// blockIdx.x = (g nk + j) ntile + tile.  Dynamic LDS: lds_bytes(nrec)
__global__ __launch_bounds__(kThreads) void wavecand_bootstrap_kernel(const float *__restrict__ slab, const int *__restrict__ rec_first,
                                                                      int nmis, int nrec, int nk, int ncand, int ntile,
                                                                      const int *__restrict__ failed, const double *__restrict__ rw,
                                                                      const double *__restrict__ ns, const double *__restrict__ cw,
                                                                      int ndraw, int d0, int nd, int ndp, int l2,
                                                                      double *__restrict__ slab_v, int *__restrict__ slab_i)
{
    extern __shared__ double lds[];
    double *sa = lds;                                       // [nrec][kThreads]
    const Walk wl(sa + (size_t)nrec * kThreads, nrec);
    const double *srw = wl.srw;
    const int tid = (int)threadIdx.x, tile = (int)(blockIdx.x % (unsigned)ntile);
    const size_t gj = blockIdx.x / (unsigned)ntile;
    const int g = (int)(gj / (unsigned)nk);
    const int cand = tile * kThreads + tid;
    const bool live = cand < ncand;
    wl.load_rw(rw + (size_t)g * nrec, nrec);
    __syncthreads();
    {
        const bool have = !failed[g];                       // (workgroup-uniform)
        const float *__restrict__ col = slab + gj * nmis * ncand + (live ? cand : 0);
        for (int r = 0; r < nrec; r++) {
            double M = 0.0;
            if (have)
                for (int k = rec_first[r]; k < rec_first[r + 1]; k++) {
                    const double mv = (double)col[(size_t)k * ncand];
                    if (l2) M = M + mv * mv;
                    else M = M + mv;
                }
            if (l2) M = sqrt(M);
            double av = M * srw[r];
            if (l2) av = av * av;
            sa[r * kThreads + tid] = av;
        }
    }
    candidates_bootstrap::draw_walk(wl, nrec, cw, ns + (size_t)g * ndraw, d0, nd, ndp, l2, live, cand, (size_t)gj * ntile + tile, slab_v, slab_i,
                                    [&](int r) { return sa[r * kThreads + tid]; });
}

// the scan's arrays that the caller of the bootstrap does not see: best_offset [group]; best_index, best_misfit [group][nk]
struct ScanArrays {
    std::vector<int> best_offset, best_index; std::vector<double> best_misfit;
    ScanArrays(size_t ngroup, size_t nk) : best_offset(ngroup, -1), best_index(ngroup * nk, -1), best_misfit(ngroup * nk, 0.0) {}
};
static waveform_candidates_timescan::Call scan_call(const Boot &bt, int *best_offset, int *best_index, double *best_misfit)
{
    return waveform_candidates_timescan::Call{ bt.x, bt.ncand, bt.outer_norm, best_offset, best_index, best_misfit, bt.status,
                                               nullptr, nullptr, nullptr, nullptr, nullptr, nullptr };
}

// what the call cannot do is refused before anything runs: everything the time scan refuses, and what the draws add
static void check_setup(kiwi_hip_ctx *c, int K, const timescan::Offsets &of, const double *receiver_weight, const Boot &bt)
{
    candidates_bootstrap::check_draws(kName, c, candidates_bootstrap::Extra::offset, kMaxRec, receiver_weight, bt, [&] {
        int idummy = 0; double ddummy = 0.0;               // (the parent's arrays: checked for null only)
        waveform_candidates_timescan::check_setup(c, K, of, scan_call(bt, &idummy, &idummy, &ddummy));
    });
}

// the bootstrap kernels of one chunk of the scan, on the run's device arrays; the spectral family's hook goes through this one
struct Hook : waveform_candidates_timescan::ChunkHook {
    kiwi_hip_ctx *c; int isrc0, K, nmis, anarchy, l2;
    candidates_bootstrap::Run st;
    DevBuf<double> w_d;
    DevBuf<int> first_d;
    // (the context is prepared: check_setup)
    Hook(kiwi_hip_ctx *ctx, const Boot &bt, int isrc0_, int K_, int nk, int anarchy_)
        : c(ctx), isrc0(isrc0_), K(K_), nmis(ctx->nmis), anarchy(anarchy_ ? 1 : 0), l2(bt.outer_norm == 2 ? 1 : 0),
          st(ctx, bt, (int)ctx->recv.size(), nk, (bt.ncand + kThreads - 1) / kThreads,
             candidates_bootstrap::draws_per_pass(ctx, bt.ndraw, nk, (bt.ncand + kThreads - 1) / kThreads))
    {
        per_group = st.per_group();
    }

    // the arrays of the run: the receiver weights, the slots of every receiver, and the run's own
    void begin(const double *receiver_weight)
    {
        const int nrec = st.nrec;
        const std::vector<double> w = receiver_weights(c, receiver_weight);
        std::vector<int> rec_first((size_t)nrec + 1, 0);       // (the slots of a receiver lie side by side, receivers ascending)
        for (int m = 0; m < nmis; m++) rec_first[(size_t)c->comps[(size_t)m].rec + 1]++;
        for (int r = 0; r < nrec; r++) rec_first[(size_t)r + 1] += rec_first[(size_t)r];
        w_d.alloc((size_t)std::max(nrec, 1), &c->dev_bytes);
        first_d.alloc((size_t)nrec + 1, &c->dev_bytes);
        HIPCHECK(hipMemcpyAsync(w_d.p, w.data(), (size_t)nrec * sizeof(double), hipMemcpyHostToDevice, c->stream));
        HIPCHECK(hipMemcpyAsync(first_d.p, rec_first.data(), rec_first.size() * sizeof(int), hipMemcpyHostToDevice, c->stream));
        st.begin();
    }

    void after_fold(int g0, int ng, const float *slab, const float *norm) override
    {
        const int ndraw = st.bt.ndraw, nrec = st.nrec, nk = st.nk;
        st.ensure(ng);
        st.mark_failed(isrc0 + g0 * K, ng, K);
        hipLaunchKernelGGL(wavecand_bootstrap_prepare_kernel, dim3((unsigned)ng), dim3(256), 0, c->stream, norm, first_d.p, nmis, nrec, nk,
                           w_d.p, anarchy, l2, st.cw.p, ndraw, st.rw.p, st.b.p, st.ns.p);
        HIPCHECK(hipGetLastError());
        if (!c->wavecand_boot_attr) {                      // (the attribute belongs to the function on this context's device)
            HIPCHECK(hipFuncSetAttribute(reinterpret_cast<const void *>(&wavecand_bootstrap_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                         kLdsBytes));
            c->wavecand_boot_attr = true;
        }
        for (int d0 = 0; d0 < ndraw; d0 += st.ndp) {
            const int nd = std::min(st.ndp, ndraw - d0);
            hipLaunchKernelGGL(wavecand_bootstrap_kernel, dim3((unsigned)((size_t)ng * nk * st.ntile)), dim3(kThreads), lds_bytes(nrec), c->stream,
                               slab, first_d.p, nmis, nrec, nk, st.bt.ncand, st.ntile, st.failed_d.p, st.rw.p, st.ns.p, st.cw.p, ndraw, d0, nd,
                               st.ndp, l2, st.slab_v.p, st.slab_i.p);
            HIPCHECK(hipGetLastError());
            st.fold(ng, d0, nd);
        }
        st.best(g0, ng);
        st.download_groups(g0, ng);                        // (with the scan's own downloads: the stream is drained behind them)
    }
};

// the groups [isrc0, isrc0 + ngroup K) of the uploaded batch: waveform_candidates_timescan::run's chunk loop with the bootstrap
// kernels behind its fold kernels.  Adds its HIP-event times to c->wavecand_boot_ms
static void run(kiwi_hip_ctx *c, int isrc0, int ngroup, int K, const timescan::Offsets &of, const double *receiver_weight, int anarchy,
                const Boot &bt)
{
    check_setup(c, K, of, receiver_weight, bt);
    check_group_range(kName, c, isrc0, ngroup, K);
    if (ngroup == 0) return;
    const int nk = of.nk;
    Hook h(c, bt, isrc0, K, nk, anarchy);
    if ((long long)nk * h.st.ntile > (1LL << 30))
        throw std::runtime_error(std::string(kName) + ": " + std::to_string(nk) + " offsets x " + std::to_string(h.st.ntile) + " candidate tiles exceed a launch");
    h.max_groups = (int)std::max<long long>((1LL << 30) / ((long long)nk * h.st.ntile), 1);    // (the candidate kernel's grid)
    float boot_ms = 0.f;
    h.ms = &boot_ms;

    h.begin(receiver_weight);

    float scan_ms[4];
    std::copy(c->wavecand_scan_ms, c->wavecand_scan_ms + 4, scan_ms);
    ScanArrays sa((size_t)ngroup, (size_t)nk);
    waveform_candidates_timescan::run(c, isrc0, ngroup, K, of, receiver_weight, anarchy,
                                      scan_call(bt, sa.best_offset.data(), sa.best_index.data(), sa.best_misfit.data()), &h);
    for (int i = 0; i < 3; i++) c->wavecand_boot_ms[i] += c->wavecand_scan_ms[i] - scan_ms[i];
    c->wavecand_boot_ms[3] += boot_ms;
    c->wavecand_boot_ms[4] += c->wavecand_scan_ms[3] - scan_ms[3];

    h.st.finish(c->wavecand_boot_ms + 4);
}

// kiwi_hip_waveform_candidates_bootstrap_params piece by piece
static PieceCall piece_call(int K, const timescan::Offsets &of, const double *receiver_weight, int anarchy, const Boot &bt)
{
    return candidates_bootstrap::piece_call(K, bt,
        [=](kiwi_hip_ctx *c, const Boot &b) { check_setup(c, K, of, receiver_weight, b); },
        [=](kiwi_hip_ctx *c, int ng, const Boot &b) { run(c, 0, ng, K, of, receiver_weight, anarchy, b); });
}

} // namespace waveform_candidates_bootstrap
