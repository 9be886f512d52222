// kiwi_group_run.hpp -- the host steps that every call built on run_chunk repeats: the range check, the receiver weights, events
// from the context's pool, the greedy chunk of whole groups, what an evaluation leaves behind, the groups whose basis failed, the
// dispatch on the number of basis sources, what a _params call does with a piece of its list.  Host code only.  Included by
// kiwi_hip.hip in front of eval_impl and the call headers.

// f(std::integral_constant<int, k>{}) with k = K for K = 1 .. 7 and k = 8 for everything else (the callers have refused other K)
template <class F>
static void by_basis(int K, F &&f)
{
    switch (K) {
    case 1: f(std::integral_constant<int, 1>{}); break;
    case 2: f(std::integral_constant<int, 2>{}); break;
    case 3: f(std::integral_constant<int, 3>{}); break;
    case 4: f(std::integral_constant<int, 4>{}); break;
    case 5: f(std::integral_constant<int, 5>{}); break;
    case 6: f(std::integral_constant<int, 6>{}); break;
    case 7: f(std::integral_constant<int, 7>{}); break;
    default: f(std::integral_constant<int, 8>{}); break;
    }
}

// a refusal of one of the calls `call_name` is made of, under that call's name
template <class F>
static void refusing(const char *call_name, F &&f)
{
    try { f(); }
    catch (const std::runtime_error &e) {
        std::string m = e.what();
        const size_t colon = m.find(": ");
        if (colon != std::string::npos && m.find(' ') > colon) m = m.substr(colon + 2);       // (the other call's name in front)
        throw std::runtime_error(std::string(call_name) + ": " + m);
    }
}

// the groups [isrc0, isrc0 + ngroup K) lie inside the uploaded batch (K = 1: plain sources)
static void check_group_range(const char *call_name, const kiwi_hip_ctx *c, int isrc0, int ngroup, int K)
{
    const long long end = (long long)isrc0 + (long long)ngroup * K;
    if (isrc0 < 0 || ngroup < 0 || end > (long long)c->nsrc)
        throw std::runtime_error(std::string(call_name) + ": sources " + std::to_string(isrc0) + " .. " + std::to_string(end) +
                                 " are not inside the uploaded batch of " + std::to_string(c->nsrc));
}

// [nrec]: the caller's weight (1 without one) of a receiver that counts, 0 for one that is disabled or has no components
static std::vector<double> receiver_weights(const kiwi_hip_ctx *c, const double *receiver_weight)
{
    std::vector<double> w(c->recv.size(), 0.0);
    for (size_t r = 0; r < w.size(); r++)
        if (c->recv[r].enabled && c->recv[r].ncomp > 0) w[r] = receiver_weight ? receiver_weight[r] : 1.0;
    return w;
}

// N events of the context's pool for the length of a call
template <int N>
struct PooledEvents {
    kiwi_hip_ctx *c;
    hipEvent_t ev[N];
    explicit PooledEvents(kiwi_hip_ctx *ctx) : c(ctx) { for (int i = 0; i < N; i++) ev[i] = c->get_event(); }
    ~PooledEvents() { for (int i = 0; i < N; i++) c->event_pool.push_back(ev[i]); }
    PooledEvents(const PooledEvents &) = delete;
    PooledEvents &operator=(const PooledEvents &) = delete;
    hipEvent_t operator[](int i) const { return ev[i]; }
    // ms[i] += the time between two of them (both recorded, the stream drained)
    void add_elapsed(float *ms, int i, int from, int to) const
    {
        float t = 0.f;
        HIPCHECK(hipEventElapsedTime(&t, ev[from], ev[to]));
        ms[i] += t;
    }
};

// With a misfit filter the traces a call keeps come from the library transforms; the filtered references are made by the transform
// their trial sources go through (make_variants), so for the length of the call that is the library's for every length -- the way
// kiwi_hip_get_amp_spectrum forces it --, and the reference variants are made afresh before and after
struct LibraryTransforms {
    kiwi_hip_ctx *c; bool fused, touched;
    explicit LibraryTransforms(kiwi_hip_ctx *ctx) : c(ctx), fused(ctx->fused_fft), touched(ctx->fft_needed && ctx->fused_fft)
    {
        if (touched) { c->fused_fft = false; drop_variants(); }
    }
    ~LibraryTransforms() { if (touched) { c->fused_fft = fused; drop_variants(); } }
    LibraryTransforms(const LibraryTransforms &) = delete;
    LibraryTransforms &operator=(const LibraryTransforms &) = delete;
    void drop_variants() { c->variants.clear(); c->refamp_h.clear(); c->filtw_h.clear(); c->reffilt_h.clear(); }
};

// what source s adds to the workspace of a chunk of run_chunk whatever the call: geometry records, coefficient lines, plans.  The
// synthetic rows differ by call and are added by each
static size_t source_workspace_bytes(const kiwi_hip_ctx *c, int s, size_t nrec)
{
    const size_t nc = (size_t)(c->cent_ofs[s + 1] - c->cent_ofs[s]);
    return nc * nrec * (sizeof(GeoRec) + (c->accum_mode == 0 ? 512 + kCoefLine * sizeof(float) : 0)) + plan_bytes(c, s, nrec);
}

constexpr int kNoSourceCap = std::numeric_limits<int>::max();

// how many whole groups of K sources from group g0 on go into one chunk: the first always, then as many as keep the workspace --
// per source source_workspace_bytes and syn_rows rows of synthetics, per group per_group_bytes -- inside KIWI_HIP_CHUNK_MB, the
// sources inside a grid dimension, and the sources at or below cap_sources (the transform workspace's fft_cap, or kNoSourceCap)
static int next_group_chunk(const kiwi_hip_ctx *c, int isrc0, int g0, int ngroup, int K, int syn_rows, size_t per_group_bytes, int cap_sources)
{
    const size_t nrec = c->recv.size();
    size_t bytes = 0;
    int ng = 0;
    while (g0 + ng < ngroup) {
        size_t add = per_group_bytes;
        for (int s = isrc0 + (g0 + ng) * K; s < isrc0 + (g0 + ng + 1) * K; s++)
            add += source_workspace_bytes(c, s, nrec) + c->syn_stride * sizeof(float) * (size_t)syn_rows;
        if (ng > 0 && (bytes + add > c->chunk_bytes_limit || (ng + 1) * K > 65535)) break;
        if ((long long)(ng + 1) * K > (long long)cap_sources) break;
        bytes += add; ng++;
    }
    return ng;
}

// what an evaluation of the range leaves behind (eval_impl)
static void leave_evaluated(kiwi_hip_ctx *c, int isrc0, int nsrc, int proc_which)
{
    c->last_isrc0 = isrc0; c->last_nsrc = nsrc; c->last_proc_which = proc_which;
    c->evaluated.resize((size_t)c->nsrc, 0);
    std::fill(c->evaluated.begin() + isrc0, c->evaluated.begin() + isrc0 + nsrc, 1);
}

// f(g) for every group of the range with a basis source that failed to discretise: there is no answer for it
template <class F>
static void for_each_failed_group(const kiwi_hip_ctx *c, int isrc0, int ngroup, int K, F &&f)
{
    for (int g = 0; g < ngroup; g++) {
        bool bad = false;
        for (int i = 0; i < K; i++) if (c->src_status[(size_t)isrc0 + (size_t)g * K + i]) bad = true;
        if (bad) f(g);
    }
}

// What a kiwi_hip_*_params call does with a piece of its list; everything else -- shards, pieces, the discretiser ahead of the device,
// upload, download -- is for_params_impl's, which knows no call by name.  Each call header makes its own (piece_call), from the
// caller's arrays for the WHOLE list.  One object serves the threads of all shards: the callables change nothing but those arrays.
// s0 counts from the head of the caller's list, in every shard, so a callable forms call.at(s0 / unit, ...) once; the sizes at()
// takes -- nmis, the receivers, the bands -- are read from ctx, which is prepared and has every mate's settings.
struct PieceCall {
    int unit;                                                   // sources per group: shards and pieces are whole multiples of it
    std::function<void(kiwi_hip_ctx *ctx)> check;               // the call's check_setup, on every context the call reaches
    std::function<void(kiwi_hip_ctx *ctx, int s0, int n)> fill_failed;      // the answer for list sources [s0, s0 + n), none of which could be discretised
    std::function<void(kiwi_hip_ctx *ctx, int s0, int n)> run;  // evaluate list sources [s0, s0 + n): sources 0 .. n - 1 of ctx, just uploaded
};
