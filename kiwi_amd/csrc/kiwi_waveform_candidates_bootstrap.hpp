// kiwi_waveform_candidates_bootstrap.hpp -- the bootstrap over the receivers of a waveform candidate search (l1norm or l2norm
// inside), joint over group (location), origin time and candidate (mechanism), without the [candidate][slot] array ever leaving the
// device: kiwi_hip_waveform_candidates_bootstrap.  What it answers is DEFINED by two existing calls:
// kiwi_hip_waveform_candidates_time_scan writes slot_misfit [ngroup][nk][ncand][nmis] and slot_norm [ngroup][nmis] as floats,
// kiwi_hip_outer_misfits reads them as ngroup nk ncand sources of nmis slots (slot m belongs to receiver slot_receiver[m]; the norm
// row of group g repeated for each of its sources) and returns the best source of every draw.  Here the scan's slab stays where
// wavecand_scan_kernel wrote it, [(group nk + j)][slot][candidate], and the norm side of the fold -- rw, b and the denominator of
// every draw -- is made once per group, because it depends neither on the candidate nor on the offset.  Included by kiwi_hip.hip
// behind kiwi_waveform_candidates_timescan.hpp under the same -ffp-contract=off: every fp64 operation below is rounded on its own;
// tests/waveform_candidates_bootstrap_restatement.py composes the scan's slot arrays with tests/outer_restatement.py, and the GPU
// tests ask for bit identity with the host route.  Per chunk of whole groups, behind the unchanged rows, scan and fold kernels of
// the time scan (waveform_candidates_timescan::ChunkHook):
//   wavecand_bootstrap_prepare_kernel   one workgroup per group.  Per receiver r, its slots k ascending (outer_prepare_kernel):
//       nv = (double) norm[k];  N = N + nv (l1norm outside) | N = N + nv nv, N = sqrt(N) behind the slots (l2norm);  rw = w_r, under
//       anarchy q = rw / (N != 0 ? N : -1), rw = q > 0 or NaN ? q : 0;  b = N rw, squared under l2norm.  Per draw: ns = 0;
//       ns = ns + b_r c_dr, r ascending (outer_draw_kernel).  A receiver without slots has N = 0.
//   wavecand_bootstrap_kernel   one workgroup of kThreads lanes per ((g, j), tile of kThreads candidates), a lane owns ONE
//       candidate.  Phase 1 walks the slots of the slab ascending (a wavefront reads 64 consecutive floats of a slot) and folds them
//       per receiver: mv = (double) slab value;  M = M + mv | M = M + mv mv, M = sqrt(M);  a = M rw_r, squared under l2norm, to LDS
//       as sa[r][lane].  Phase 2 walks the draws of the pass in tiles of kTileD: the weight rows staged as cs[r][t], read as
//       broadcasts; ms_t = ms_t + a_r c_rt from zero, r ascending; v = ms / ns (root under l2norm), excluded (NaN) where not ns > 0
//       or not v >= 0.  (value, candidate) folded over wavefront and workgroup (linfit::wave_best, take_better); the tile's best of
//       every draw goes to slab_v, slab_i[(g, j)][tile][draw of the pass].  Nothing per candidate goes to global memory.
//   bootstrap_fold_kernel, bootstrap_best_kernel   kiwi_linfit_candidates_bootstrap.hpp's, unchanged: offsets and tiles per (group,
//       draw), then the chunk's groups into the running best of the run, which stays on the device until the last chunk.
// The order of "best" is total -- excluded last, then the smaller value, then the lowest (g, j, c) --, so no answer depends on
// tiles, draw passes, chunks (KIWI_HIP_CHUNK_MB), isrc0, pieces or devices.  No atomics, zero scratch
// (profiles/waveform_candidates_bootstrap_kernel_resources.json).  A draw with every source excluded: NaN, -1, -1, -1 -- the one
// difference from the host route, which answers NaN and index 0.  A group whose basis failed to discretise (status 2) or that no
// receiver counts for (status 1) has zero norms, so ns > 0 fails in every draw.  The kernels take slab, norms and the slot table as
// plain arguments: the floating and spectral families' slabs have the same layout.

namespace waveform_candidates_bootstrap {

using linfit_candidates_bootstrap::Boot;

constexpr int kThreads = 256;                       // candidates per workgroup, one per lane
constexpr int kTileD = 16;                          // draws per tile: 16 fp64 accumulators per lane
constexpr int kLdsBytes = 152 * 1024;               // of the 160 KiB a workgroup may hold
// LDS of the candidate kernel: the wavefronts' bests, and what one receiver adds (its column of a, its weight row of a draw tile,
// its rw)
constexpr int kLdsFixed = (kThreads / 64) * kTileD * 12;
constexpr int kLdsPerRec = kThreads * 8 + kTileD * 8 + 8;
constexpr int kMaxRec = (kLdsBytes - kLdsFixed) / kLdsPerRec;          // 70
static_assert(kMaxRec >= 64, "the layout must hold 64 receivers");
static size_t lds_bytes(int nrec) { return (size_t)kLdsFixed + (size_t)nrec * kLdsPerRec; }

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
        double rw = w[r];
        if (anarchy) {
            const double q = rw / (N != 0.0 ? N : -1.0);
            rw = (q > 0.0 || q != q) ? q : 0.0;
        }
        double bv = N * rw;
        if (l2) bv = bv * bv;
        rw_out[(size_t)g * nrec + r] = rw;
        b_out[(size_t)g * nrec + r] = bv;
    }
    __syncthreads();                                        // (b_out of this group: written by this workgroup, visible to it)
    const double *b = b_out + (size_t)g * nrec;
    for (int d = tid; d < ndraw; d += 256) {
        double s = 0.0;
        for (int r = 0; r < nrec; r++) s = s + b[r] * cw[(size_t)d * nrec + r];
        ns[(size_t)g * ndraw + d] = s;
    }
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
    constexpr int NW = kThreads / 64;
    extern __shared__ double lds[];
    double *sa = lds;                                       // [nrec][kThreads]
    double *srw = sa + (size_t)nrec * kThreads;             // [nrec]
    double *cs = srw + nrec;                                // [nrec][kTileD]
    double *red_v = cs + (size_t)nrec * kTileD;             // [NW][kTileD]
    int *red_i = (int *)(red_v + NW * kTileD);              // [NW][kTileD]
    const int tid = (int)threadIdx.x, tile = (int)(blockIdx.x % (unsigned)ntile);
    const size_t gj = blockIdx.x / (unsigned)ntile;
    const int g = (int)(gj / (unsigned)nk);
    const int cand = tile * kThreads + tid;
    const bool live = cand < ncand;
    const double nan = __longlong_as_double(0x7ff8000000000000LL);
    for (int r = tid; r < nrec; r += kThreads) srw[r] = rw[(size_t)g * nrec + r];
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
    const int lane = tid & 63, wave = tid >> 6;
    for (int t0 = 0; t0 < nd; t0 += kTileD) {
        __syncthreads();                                    // (the weight rows and the bests of the tile before)
        for (int i = tid; i < nrec * kTileD; i += kThreads) {
            const int t = i / nrec, r = i - t * nrec;
            cs[r * kTileD + t] = t0 + t < nd ? cw[(size_t)(d0 + t0 + t) * nrec + r] : 0.0;
        }
        __syncthreads();
        double ms[kTileD];
#pragma unroll
        for (int t = 0; t < kTileD; t++) ms[t] = 0.0;
        for (int r = 0; r < nrec; r++) {
            const double av = sa[r * kThreads + tid];
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
    refusing(kName, [&] {
        if (bt.ndraw < 1) throw std::runtime_error("ndraw = " + std::to_string(bt.ndraw) + "; at least one draw is needed");
        if (!bt.draw_weights || !bt.best_value || !bt.best_group || !bt.best_offset || !bt.best_cand || !bt.status)
            throw std::runtime_error("null draw_weights, best_value, best_group, best_offset, best_cand or status array");
        const int ngiven = (bt.group_value ? 1 : 0) + (bt.group_offset ? 1 : 0) + (bt.group_cand ? 1 : 0);
        if (ngiven != 0 && ngiven != 3) throw std::runtime_error("group_value, group_offset and group_cand are given all three or not at all");
        int idummy = 0; double ddummy = 0.0;               // (the parent's arrays: checked for null only)
        waveform_candidates_timescan::check_setup(c, K, of, scan_call(bt, &idummy, &idummy, &ddummy));
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

// the bootstrap kernels of one chunk of the scan, and the device arrays of the run
struct Hook : waveform_candidates_timescan::ChunkHook {
    kiwi_hip_ctx *c; const Boot &bt; int isrc0, K, nk, nrec, nmis, ntile, ndp, anarchy, l2;
    std::vector<int> failed;
    DevBuf<double> w_d, cw_d, rw_d, b_d, ns_d, slabv_d, grpv_d, runv_d;
    DevBuf<int> first_d, failed_d, slabi_d, grpj_d, grpc_d, rung_d, runj_d, runc_d;
    Hook(kiwi_hip_ctx *ctx, const Boot &b) : c(ctx), bt(b) {}

    // the arrays of the run: the receiver weights, the slots of every receiver, the draws, the running best (NaN, -1).  nrec, nmis
    // are set
    void begin(const double *receiver_weight)
    {
        const int ndraw = bt.ndraw;
        const std::vector<double> w = receiver_weights(c, receiver_weight);
        std::vector<int> rec_first((size_t)nrec + 1, 0);       // (the slots of a receiver lie side by side, receivers ascending)
        for (int m = 0; m < nmis; m++) rec_first[(size_t)c->comps[(size_t)m].rec + 1]++;
        for (int r = 0; r < nrec; r++) rec_first[(size_t)r + 1] += rec_first[(size_t)r];
        const std::vector<double> nanv((size_t)ndraw, std::numeric_limits<double>::quiet_NaN());
        const std::vector<int> nonev((size_t)ndraw, -1);
        w_d.alloc((size_t)std::max(nrec, 1), &c->dev_bytes);
        first_d.alloc((size_t)nrec + 1, &c->dev_bytes);
        cw_d.alloc((size_t)ndraw * std::max(nrec, 1), &c->dev_bytes);
        runv_d.alloc((size_t)ndraw, &c->dev_bytes); rung_d.alloc((size_t)ndraw, &c->dev_bytes);
        runj_d.alloc((size_t)ndraw, &c->dev_bytes); runc_d.alloc((size_t)ndraw, &c->dev_bytes);
        HIPCHECK(hipMemcpyAsync(w_d.p, w.data(), (size_t)nrec * sizeof(double), hipMemcpyHostToDevice, c->stream));
        HIPCHECK(hipMemcpyAsync(first_d.p, rec_first.data(), rec_first.size() * sizeof(int), hipMemcpyHostToDevice, c->stream));
        HIPCHECK(hipMemcpyAsync(cw_d.p, bt.draw_weights, (size_t)ndraw * nrec * sizeof(double), hipMemcpyHostToDevice, c->stream));
        HIPCHECK(hipMemcpyAsync(runv_d.p, nanv.data(), (size_t)ndraw * sizeof(double), hipMemcpyHostToDevice, c->stream));
        for (int *p : { rung_d.p, runj_d.p, runc_d.p })
            HIPCHECK(hipMemcpyAsync(p, nonev.data(), (size_t)ndraw * sizeof(int), hipMemcpyHostToDevice, c->stream));
        HIPCHECK(hipStreamSynchronize(c->stream));
    }

    // the running best of the run comes down and is folded into the bests of the call; the download's HIP-event time is added to
    // *down_ms
    void finish(float *down_ms)
    {
        const int ndraw = bt.ndraw;
        std::vector<double> rv((size_t)ndraw);
        std::vector<int> rg((size_t)ndraw), rj((size_t)ndraw), rc((size_t)ndraw);
        const PooledEvents<2> ev(c);
        HIPCHECK(hipEventRecord(ev[0], c->stream));
        HIPCHECK(hipMemcpyAsync(rv.data(), runv_d.p, (size_t)ndraw * sizeof(double), hipMemcpyDeviceToHost, c->stream));
        HIPCHECK(hipMemcpyAsync(rg.data(), rung_d.p, (size_t)ndraw * sizeof(int), hipMemcpyDeviceToHost, c->stream));
        HIPCHECK(hipMemcpyAsync(rj.data(), runj_d.p, (size_t)ndraw * sizeof(int), hipMemcpyDeviceToHost, c->stream));
        HIPCHECK(hipMemcpyAsync(rc.data(), runc_d.p, (size_t)ndraw * sizeof(int), hipMemcpyDeviceToHost, c->stream));
        HIPCHECK(hipEventRecord(ev[1], c->stream));
        HIPCHECK(hipStreamSynchronize(c->stream));
        ev.add_elapsed(down_ms, 0, 0, 1);
        linfit_candidates_bootstrap::merge(bt, rv.data(), rg.data(), rj.data(), rc.data());
    }

    void after_fold(int g0, int ng, const float *slab, const float *norm) override
    {
        const int ndraw = bt.ndraw;
        const size_t nsolve = (size_t)ng * nk;
        failed.assign((size_t)ng, 0);
        for_each_failed_group(c, isrc0 + g0 * K, ng, K, [&](int g) { failed[(size_t)g] = 1; });
        failed_d.ensure((size_t)ng, &c->dev_bytes);
        rw_d.ensure((size_t)ng * nrec, &c->dev_bytes); b_d.ensure((size_t)ng * nrec, &c->dev_bytes);
        ns_d.ensure((size_t)ng * ndraw, &c->dev_bytes);
        slabv_d.ensure(nsolve * ntile * ndp, &c->dev_bytes); slabi_d.ensure(nsolve * ntile * ndp, &c->dev_bytes);
        grpv_d.ensure((size_t)ng * ndraw, &c->dev_bytes); grpj_d.ensure((size_t)ng * ndraw, &c->dev_bytes);
        grpc_d.ensure((size_t)ng * ndraw, &c->dev_bytes);
        // (`failed` is read by this copy; the scan drains the stream at the end of the chunk, before the next call of this function)
        HIPCHECK(hipMemcpyAsync(failed_d.p, failed.data(), (size_t)ng * sizeof(int), hipMemcpyHostToDevice, c->stream));
        hipLaunchKernelGGL(wavecand_bootstrap_prepare_kernel, dim3((unsigned)ng), dim3(256), 0, c->stream, norm, first_d.p, nmis, nrec, nk,
                           w_d.p, anarchy, l2, cw_d.p, ndraw, rw_d.p, b_d.p, ns_d.p);
        HIPCHECK(hipGetLastError());
        if (!c->wavecand_boot_attr) {                      // (the attribute belongs to the function on this context's device)
            HIPCHECK(hipFuncSetAttribute(reinterpret_cast<const void *>(&wavecand_bootstrap_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                         kLdsBytes));
            c->wavecand_boot_attr = true;
        }
        for (int d0 = 0; d0 < ndraw; d0 += ndp) {
            const int nd = std::min(ndp, ndraw - d0);
            hipLaunchKernelGGL(wavecand_bootstrap_kernel, dim3((unsigned)(nsolve * ntile)), dim3(kThreads), lds_bytes(nrec), c->stream, slab,
                               first_d.p, nmis, nrec, nk, bt.ncand, ntile, failed_d.p, rw_d.p, ns_d.p, cw_d.p, ndraw, d0, nd, ndp, l2, slabv_d.p,
                               slabi_d.p);
            HIPCHECK(hipGetLastError());
            hipLaunchKernelGGL(linfit_candidates_bootstrap::bootstrap_fold_kernel, dim3((unsigned)((nd + 255) / 256), (unsigned)ng), dim3(256), 0,
                               c->stream, slabv_d.p, slabi_d.p, nk, ntile, ndp, d0, nd, ndraw, failed_d.p, grpv_d.p, grpj_d.p, grpc_d.p);
            HIPCHECK(hipGetLastError());
        }
        hipLaunchKernelGGL(linfit_candidates_bootstrap::bootstrap_best_kernel, dim3((unsigned)((ndraw + 255) / 256)), dim3(256), 0, c->stream,
                           grpv_d.p, grpj_d.p, grpc_d.p, ng, g0, ndraw, runv_d.p, rung_d.p, runj_d.p, runc_d.p);
        HIPCHECK(hipGetLastError());
        // (the group bests go down with the scan's own downloads: the stream is drained behind them)
        if (bt.group_value) {
            const Boot o = bt.at((size_t)g0);
            HIPCHECK(hipMemcpyAsync(o.group_value, grpv_d.p, (size_t)ng * ndraw * sizeof(double), hipMemcpyDeviceToHost, c->stream));
            HIPCHECK(hipMemcpyAsync(o.group_offset, grpj_d.p, (size_t)ng * ndraw * sizeof(int), hipMemcpyDeviceToHost, c->stream));
            HIPCHECK(hipMemcpyAsync(o.group_cand, grpc_d.p, (size_t)ng * ndraw * sizeof(int), hipMemcpyDeviceToHost, c->stream));
        }
    }
};

// the groups [isrc0, isrc0 + ngroup K) of the uploaded batch: waveform_candidates_timescan::run's chunk loop with the bootstrap
// kernels behind its fold kernels.  Adds its HIP-event times to c->wavecand_boot_ms
static void run(kiwi_hip_ctx *c, int isrc0, int ngroup, int K, const timescan::Offsets &of, const double *receiver_weight, int anarchy,
                const Boot &bt)
{
    waveform_candidates_bootstrap::check_setup(c, K, of, receiver_weight, bt);     // (qualified: Boot is the Gram sibling's)
    check_group_range(kName, c, isrc0, ngroup, K);
    if (ngroup == 0) return;
    const int nrec = (int)c->recv.size(), nmis = c->nmis, nk = of.nk, ndraw = bt.ndraw;
    const int ntile = (bt.ncand + kThreads - 1) / kThreads;
    // the draws of one pass: all of them, unless the slab of ONE group would exceed the chunk bound; then whole tiles of draws
    const size_t slab_per_draw = (size_t)nk * ntile * (sizeof(double) + sizeof(int));
    int ndp = ndraw;
    if (slab_per_draw * (size_t)ndraw > c->chunk_bytes_limit)
        ndp = (int)std::min<size_t>((size_t)ndraw, std::max<size_t>(c->chunk_bytes_limit / slab_per_draw / kTileD, 1) * kTileD);
    if ((long long)nk * ntile > (1LL << 30))
        throw std::runtime_error(std::string(kName) + ": " + std::to_string(nk) + " offsets x " + std::to_string(ntile) + " candidate tiles exceed a launch");

    Hook h(c, bt);
    h.isrc0 = isrc0; h.K = K; h.nk = nk; h.nrec = nrec; h.nmis = nmis; h.ntile = ntile; h.ndp = ndp;
    h.anarchy = anarchy ? 1 : 0; h.l2 = bt.outer_norm == 2 ? 1 : 0;
    // per group: the slab of one pass, ns and the group's bests per draw, rw and b, the flag
    h.per_group = slab_per_draw * (size_t)ndp + (size_t)ndraw * (2 * sizeof(double) + 2 * sizeof(int)) + (size_t)nrec * 2 * sizeof(double) + sizeof(int);
    h.max_groups = (int)std::max<long long>((1LL << 30) / ((long long)nk * ntile), 1);         // (the candidate kernel's grid)
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

    h.finish(c->wavecand_boot_ms + 4);
}

// kiwi_hip_waveform_candidates_bootstrap_params piece by piece: the Gram sibling's PieceCall with this header's check_setup and run
static PieceCall piece_call(int K, const timescan::Offsets &of, const double *receiver_weight, int anarchy, const Boot &bt)
{
    return linfit_candidates_bootstrap::piece_call(K, of, receiver_weight, anarchy, bt, &check_setup, &run);
}

} // namespace waveform_candidates_bootstrap
