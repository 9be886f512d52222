// kiwi_candidates_bootstrap.hpp -- what the joint bootstraps of a candidate search have in common: kiwi_linfit_candidates_bootstrap.hpp
// (the Gram family), kiwi_linfit_candidates_floating_bootstrap.hpp, kiwi_waveform_candidates_bootstrap.hpp and
// kiwi_spectral_candidates_bootstrap.hpp keep only their own phase 1 -- how a candidate's misfit of a receiver is made -- and their own
// way to the norm N of a receiver.  Included by kiwi_hip.hip ahead of the four, under the same -ffp-contract=off: every fp64 operation
// below is rounded on its own, and the GPU tests of the four ask for bit identity with the host route (kiwi_hip_outer_misfits on the
// parent call's arrays).
//   norm_side, draw_norms   the tail of a family's prepare kernel (one workgroup of 256 per group), outer_prepare_kernel's and
//       outer_draw_kernel's expressions: rw = w_r, under anarchy q = rw / (N != 0 ? N : -1), rw = q > 0 or NaN ? q : 0;  b = N rw,
//       squared under l2norm.  Per draw, behind a barrier: ns = 0; ns = ns + b_r c_dr, r ascending.
//   draw_walk   phase 2 of a family's candidate kernel: a lane owns ONE candidate and has a_r of every receiver at hand (a callable:
//       the families keep a column of m or of a in LDS).  The draws of the pass in tiles of kTileD: the weight rows staged as cs[r][t]
//       and read as broadcasts; ms_t = ms_t + a_r c_rt from zero, r ascending; v = ms / ns (root under l2norm), excluded (NaN) where
//       not ns > 0 or not v >= 0.  (value, candidate) folded over wavefront and workgroup (linfit::wave_best, take_better, waves
//       ascending); the tile's best of every draw goes to slab_v, slab_i[row][draw of the pass].  Nothing per candidate goes to global
//       memory.  WalkLds is the walk's part of the kernel's dynamic LDS and the one description of its size.  The floating and the
//       waveform kernel call it; linfit_candidates_bootstrap_kernel<K> keeps a copy of the text, which is measurably faster there
//       (the head of kiwi_linfit_candidates_bootstrap.hpp): a change here is a change there.
//   bootstrap_fold_kernel   per (group, draw): the slab's offsets and tiles folded into grp_v, grp_j, grp_c[group][draw].
//   bootstrap_best_kernel   per draw: the chunk's groups folded into the running best of the run, which stays on the device until the
//       last chunk.
// The order of "best" is total -- excluded last, then the smaller value, then the lowest (g, j, c) --, so no answer depends on tiles,
// draw passes, chunks, pieces or devices.  No atomics.  A draw with every source excluded: NaN, -1, -1, -1.
// On the host: Boot (the caller's arrays), check_draws (what the draws add to a parent's refusals), draws_per_pass, Run (the device
// arrays of a run and the launches behind a family's candidate kernel) and piece_call.

namespace candidates_bootstrap {

constexpr int kTileD = 16;                          // draws per tile: 16 fp64 accumulators per lane
constexpr int kLdsBytes = 152 * 1024;               // of the 160 KiB a workgroup may hold

// the walk's part of the dynamic LDS of a candidate kernel of NT lanes, from `at` on: what does not grow with the receivers (the
// wavefronts' bests) and what one receiver adds (its weight row of a draw tile, its rw).  A kernel's own part -- its stages, its
// column of m or a per receiver -- lies in front of `at` or behind end()
template <int NT>
struct WalkLds {
    static constexpr int NW = NT / 64;
    static constexpr int kFixed = NW * kTileD * (8 + 4), kPerRec = kTileD * 8 + 8;
    double *srw;                                            // [nrec]
    double *cs;                                             // [nrec][kTileD]
    double *red_v;                                          // [NW][kTileD]
    int *red_i;                                             // [NW][kTileD]
    __device__ __forceinline__ WalkLds(double *at, int nrec) : srw(at), cs(at + nrec), red_v(cs + (size_t)nrec * kTileD), red_i((int *)(red_v + NW * kTileD)) {}
    __device__ __forceinline__ void *end() const { return red_i + NW * kTileD; }
    __device__ __forceinline__ void load_rw(const double *__restrict__ rw_g, int nrec) const        // (read behind the next barrier)
    {
        for (int r = (int)threadIdx.x; r < nrec; r += NT) srw[r] = rw_g[r];
    }
    // bytes of a kernel whose own part is own_fixed + nrec own_per_rec, and the receivers it holds
    static size_t bytes(int own_fixed, int own_per_rec, int nrec) { return (size_t)(own_fixed + kFixed) + (size_t)nrec * (own_per_rec + kPerRec); }
    static constexpr int max_rec(int own_fixed, int own_per_rec) { return (kLdsBytes - own_fixed - kFixed) / (own_per_rec + kPerRec); }
};

// a_r of the families that keep m as floats, sm[r][lane]: mv = (double) sm[r][lane] -- under l2norm the host route forms sqrt(mv mv),
// which IS mv for a float (tests) --, a = mv rw_r, squared under l2norm
template <int NT>
struct FloatColumn {
    const float *sm; const double *srw; int l2;
    __device__ __forceinline__ double operator()(int r) const
    {
        const double mv = (double)sm[r * NT + (int)threadIdx.x];
        double av = mv * srw[r];
        if (l2) av = av * av;
        return av;
    }
};

// cw: [ndraw][nrec]; ns_g: [ndraw], the group's; the draws [d0, d0 + nd) of this pass; slab_v, slab_i: [row][ndp], `row` the
// workgroup's; L.srw is loaded (load_rw; the first barrier below covers it).  Every lane of the workgroup comes here
template <int NT, class A>
__device__ __forceinline__ void draw_walk(const WalkLds<NT> &L, int nrec, const double *__restrict__ cw, const double *__restrict__ ns_g,
                                          int d0, int nd, int ndp, int l2, bool live, int cand, size_t row, double *__restrict__ slab_v,
                                          int *__restrict__ slab_i, A a_of)
{
    constexpr int NW = NT / 64;
    const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const double nan = __longlong_as_double(0x7ff8000000000000LL);
    double *cs = L.cs, *red_v = L.red_v;
    int *red_i = L.red_i;
    for (int t0 = 0; t0 < nd; t0 += kTileD) {
        __syncthreads();                                    // (srw; the weight rows and the bests of the tile before)
        for (int i = tid; i < nrec * kTileD; i += NT) {
            const int t = i / nrec, r = i - t * nrec;
            cs[r * kTileD + t] = t0 + t < nd ? cw[(size_t)(d0 + t0 + t) * nrec + r] : 0.0;
        }
        __syncthreads();
        double ms[kTileD];
#pragma unroll
        for (int t = 0; t < kTileD; t++) ms[t] = 0.0;
        for (int r = 0; r < nrec; r++) {
            const double av = a_of(r);
            const double *c = cs + r * kTileD;
#pragma unroll
            for (int t = 0; t < kTileD; t++) ms[t] = ms[t] + av * c[t];
        }
#pragma unroll
        for (int t = 0; t < kTileD; t++) {
            const double den = t0 + t < nd ? ns_g[d0 + t0 + t] : 0.0;
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
            const size_t at = row * ndp + t0 + tid;
            slab_v[at] = v;
            slab_i[at] = bi;
        }
    }
}

// the norm side of one receiver from its norm N and its weight w
__device__ __forceinline__ void norm_side(double N, double w, int anarchy, int l2, double &rw, double &b)
{
    rw = w;
    if (anarchy) {
        const double q = rw / (N != 0.0 ? N : -1.0);
        rw = (q > 0.0 || q != q) ? q : 0.0;
    }
    b = N * rw;
    if (l2) b = b * b;
}

// b_g: [nrec], the group's, written by THIS workgroup of 256 in front of the call; cw: [ndraw][nrec]; ns_g: [ndraw]
__device__ __forceinline__ void draw_norms(const double *b_g, const double *__restrict__ cw, int nrec, int ndraw, double *__restrict__ ns_g)
{
    __syncthreads();                                        // (b of this group: written by this workgroup, visible to it)
    for (int d = (int)threadIdx.x; d < ndraw; d += 256) {
        double s = 0.0;
        for (int r = 0; r < nrec; r++) s = s + b_g[r] * cw[(size_t)d * nrec + r];
        ns_g[d] = s;
    }
}

// slab_v, slab_i: [group nk][ntile][ndp] for the draws [d0, d0 + nd); grp_v, grp_j, grp_c: [group][ndraw].  blockIdx.y = group
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

// host arrays of the caller for the groups of ONE call of a family's run(): status [group]; group_value, group_cand [group][ndraw].
// best_value, best_group, best_cand [ndraw] belong to the WHOLE call: the caller fills them with NaN / -1 (begin), every run() folds its
// own bests into them with `group0` added to its group indices, under `mu` where runs of several devices share them.  A family with
// origin times has best_offset [ndraw] and group_offset [group][ndraw] beside them, a family with per-receiver shifts best_shift
// [ndraw][nrec] and group_shift [group][ndraw][nrec] (zeros without a winner); null where the family has none.  The group arrays are
// given all or none.  x [ncand][K] and draw_weights [ndraw][nrec] are shared by all groups
struct Boot {
    const double *x; int ncand, outer_norm, ndraw; const double *draw_weights;
    double *best_value; int *best_group, *best_cand;
    int *status;
    double *group_value; int *group_cand;
    int *best_offset, *group_offset;
    int *best_shift, *group_shift;
    int group0; std::mutex *mu;
    Boot at(size_t g, size_t nrec) const
    {
        Boot b = *this;
        b.status += g; b.group0 += (int)g;
        if (group_value) { b.group_value += g * (size_t)ndraw; b.group_cand += g * (size_t)ndraw; }
        if (group_offset) b.group_offset += g * (size_t)ndraw;
        if (group_shift) b.group_shift += g * (size_t)ndraw * nrec;
        return b;
    }
    void begin(size_t nrec) const
    {
        std::fill(best_value, best_value + ndraw, std::numeric_limits<double>::quiet_NaN());
        std::fill(best_group, best_group + ndraw, -1); std::fill(best_cand, best_cand + ndraw, -1);
        if (best_offset) std::fill(best_offset, best_offset + ndraw, -1);
        if (best_shift) std::fill(best_shift, best_shift + (size_t)ndraw * nrec, 0);
    }
    // groups whose basis sources could not be discretised at all (nothing was uploaded for them): status 2, no best in any draw
    void fill_failed(size_t ngroup, size_t nrec) const
    {
        std::fill(status, status + ngroup, 2);
        if (!group_value) return;
        std::fill(group_value, group_value + ngroup * (size_t)ndraw, std::numeric_limits<double>::quiet_NaN());
        std::fill(group_cand, group_cand + ngroup * (size_t)ndraw, -1);
        if (group_offset) std::fill(group_offset, group_offset + ngroup * (size_t)ndraw, -1);
        if (group_shift) std::fill(group_shift, group_shift + ngroup * (size_t)ndraw * nrec, 0);
    }
    // the bests of one run folded into those of the call, in the total order (j reads as 0 where there are no offsets), the winner's
    // row of shift [ndraw][nrec] with it where there are shifts; g: indices inside the run
    void merge(size_t nrec, const double *v, const int *g, const int *j, const int *cd, const int *shift) const
    {
        std::unique_lock<std::mutex> lk;
        if (mu) lk = std::unique_lock<std::mutex>(*mu);
        for (int d = 0; d < ndraw; d++) {
            if (cd[d] < 0) continue;
            const int g2 = group0 + g[d], j2 = best_offset ? j[d] : 0, j1 = best_offset ? best_offset[d] : 0;
            const double v1 = best_value[d];
            const bool better = best_cand[d] < 0 || v[d] < v1 ||
                                (v[d] == v1 && std::make_tuple(g2, j2, cd[d]) < std::make_tuple(best_group[d], j1, best_cand[d]));
            if (!better) continue;
            best_value[d] = v[d]; best_group[d] = g2; best_cand[d] = cd[d];
            if (best_offset) best_offset[d] = j2;
            if (best_shift) std::copy(shift + (size_t)d * nrec, shift + (size_t)(d + 1) * nrec, best_shift + (size_t)d * nrec);
        }
    }
};

// which arrays a family has beside value, group and candidate
enum class Extra { none, offset, shift };

// what the draws add to the refusals of the parent call, in the name of the family's call: the arrays in front of `parent` (the
// parent's own check_setup, which prepares the context), the receivers against the family's LDS layout and the weights behind it
template <class Parent>
static void check_draws(const char *name, kiwi_hip_ctx *c, Extra extra, int max_rec, const double *receiver_weight, const Boot &bt, Parent parent)
{
    refusing(name, [&] {
        if (bt.ndraw < 1) throw std::runtime_error("ndraw = " + std::to_string(bt.ndraw) + "; at least one draw is needed");
        const bool of = extra == Extra::offset, sh = extra == Extra::shift;
        if (!bt.draw_weights || !bt.best_value || !bt.best_group || !bt.best_cand || !bt.status || (of && !bt.best_offset) || (sh && !bt.best_shift))
            throw std::runtime_error(std::string("null draw_weights, best_value, best_group, ") + (of ? "best_offset, " : "") + "best_cand" +
                                     (sh ? ", best_shift" : "") + " or status array");
        const int ngiven = (bt.group_value ? 1 : 0) + (bt.group_cand ? 1 : 0) + (of && bt.group_offset ? 1 : 0) + (sh && bt.group_shift ? 1 : 0);
        if (ngiven != 0 && ngiven != (of || sh ? 3 : 2))
            throw std::runtime_error(of   ? "group_value, group_offset and group_cand are given all three or not at all"
                                     : sh ? "group_value, group_cand and group_shift are given all three or not at all"
                                          : "group_value and group_cand are given both or not at all");
        parent();
        const size_t nrec = c->recv.size();
        if (nrec > (size_t)max_rec)
            throw std::runtime_error(std::to_string(nrec) + " receivers; a candidate's misfits of all receivers stay in LDS, which holds at most " +
                                     std::to_string(max_rec));
        if (receiver_weight)
            for (size_t r = 0; r < nrec; r++)
                if (!std::isfinite(receiver_weight[r])) throw std::runtime_error("receiver_weight of receiver " + std::to_string(r + 1) + " is not finite");
        for (size_t p = 0; p < (size_t)bt.ndraw * nrec; p++)
            if (!std::isfinite(bt.draw_weights[p]))
                throw std::runtime_error("draw_weights of draw " + std::to_string(p / nrec) + ", receiver " + std::to_string(p % nrec + 1) + " is not finite");
    });
}

// bytes of slab_v, slab_i that one draw of one group takes, and the draws of one pass: all of them, unless the slab of ONE group would
// exceed the chunk bound; then whole tiles of draws
static size_t slab_per_draw(int nk, int ntile) { return (size_t)nk * ntile * (sizeof(double) + sizeof(int)); }
static int draws_per_pass(const kiwi_hip_ctx *c, int ndraw, int nk, int ntile)
{
    const size_t per_draw = slab_per_draw(nk, ntile);
    if (per_draw * (size_t)ndraw <= c->chunk_bytes_limit) return ndraw;
    return (int)std::min<size_t>((size_t)ndraw, std::max<size_t>(c->chunk_bytes_limit / per_draw / kTileD, 1) * kTileD);
}

// the device arrays of one run() behind a family's candidate kernel, and the launches that all families make on them.  Per chunk of ng
// groups: ensure, mark_failed, the family's prepare kernel (rw, b, ns), per draw pass the family's candidate kernel (slab_v, slab_i)
// and fold; then best and download_groups.  finish behind the last chunk
struct Run {
    kiwi_hip_ctx *c; const Boot &bt; int nrec, nk, ntile, ndp;
    std::vector<int> failed;
    DevBuf<double> cw, rw, b, ns, slab_v, grp_v, run_v;
    DevBuf<int> failed_d, slab_i, grp_j, grp_c, run_g, run_j, run_c;
    Run(kiwi_hip_ctx *ctx, const Boot &boot, int nrec_, int nk_, int ntile_, int ndp_)
        : c(ctx), bt(boot), nrec(nrec_), nk(nk_), ntile(ntile_), ndp(ndp_) {}
    // bytes per group of what ensure() allocates
    size_t per_group() const
    {
        return slab_per_draw(nk, ntile) * (size_t)ndp + (size_t)bt.ndraw * (2 * sizeof(double) + 2 * sizeof(int)) + (size_t)nrec * 2 * sizeof(double) + sizeof(int);
    }

    // the draws go up, the running best is NaN, -1; drains the stream, the caller's own uploads in front with it
    void begin()
    {
        const size_t ndraw = (size_t)bt.ndraw;
        const std::vector<double> nanv(ndraw, std::numeric_limits<double>::quiet_NaN());
        const std::vector<int> nonev(ndraw, -1);
        cw.alloc(ndraw * std::max(nrec, 1), &c->dev_bytes);
        run_v.alloc(ndraw, &c->dev_bytes); run_g.alloc(ndraw, &c->dev_bytes); run_j.alloc(ndraw, &c->dev_bytes); run_c.alloc(ndraw, &c->dev_bytes);
        HIPCHECK(hipMemcpyAsync(cw.p, bt.draw_weights, ndraw * nrec * sizeof(double), hipMemcpyHostToDevice, c->stream));
        HIPCHECK(hipMemcpyAsync(run_v.p, nanv.data(), ndraw * sizeof(double), hipMemcpyHostToDevice, c->stream));
        for (int *p : { run_g.p, run_j.p, run_c.p })
            HIPCHECK(hipMemcpyAsync(p, nonev.data(), ndraw * sizeof(int), hipMemcpyHostToDevice, c->stream));
        HIPCHECK(hipStreamSynchronize(c->stream));
    }

    void ensure(int ng)
    {
        const size_t ngr = (size_t)ng * nrec, ngd = (size_t)ng * bt.ndraw, nslab = (size_t)ng * nk * ntile * ndp;
        failed_d.ensure((size_t)ng, &c->dev_bytes);
        rw.ensure(ngr, &c->dev_bytes); b.ensure(ngr, &c->dev_bytes);
        ns.ensure(ngd, &c->dev_bytes);
        slab_v.ensure(nslab, &c->dev_bytes); slab_i.ensure(nslab, &c->dev_bytes);
        grp_v.ensure(ngd, &c->dev_bytes); grp_j.ensure(ngd, &c->dev_bytes); grp_c.ensure(ngd, &c->dev_bytes);
    }

    // failed_d [ng]: 1 for a group of the chunk (its sources from s0 on) with a basis source that failed to discretise.  (`failed` is
    // read by this copy: the stream is drained at the end of every chunk, before the next call)
    void mark_failed(int s0, int ng, int K)
    {
        failed.assign((size_t)ng, 0);
        for_each_failed_group(c, s0, ng, K, [&](int g) { failed[(size_t)g] = 1; });
        HIPCHECK(hipMemcpyAsync(failed_d.p, failed.data(), (size_t)ng * sizeof(int), hipMemcpyHostToDevice, c->stream));
    }

    // behind the candidate kernel of the draws [d0, d0 + nd)
    void fold(int ng, int d0, int nd)
    {
        hipLaunchKernelGGL(bootstrap_fold_kernel, dim3((unsigned)((nd + 255) / 256), (unsigned)ng), dim3(256), 0, c->stream, slab_v.p, slab_i.p,
                           nk, ntile, ndp, d0, nd, bt.ndraw, failed_d.p, grp_v.p, grp_j.p, grp_c.p);
        HIPCHECK(hipGetLastError());
    }

    // behind the last pass: the chunk's groups, the first of which is g0 of the run
    void best(int g0, int ng)
    {
        hipLaunchKernelGGL(bootstrap_best_kernel, dim3((unsigned)((bt.ndraw + 255) / 256)), dim3(256), 0, c->stream, grp_v.p, grp_j.p, grp_c.p,
                           ng, g0, bt.ndraw, run_v.p, run_g.p, run_j.p, run_c.p);
        HIPCHECK(hipGetLastError());
    }

    // the group bests to the caller's arrays, where there are any (on the stream: the caller drains it)
    void download_groups(int g0, int ng)
    {
        if (!bt.group_value) return;
        const Boot o = bt.at((size_t)g0, (size_t)nrec);
        const size_t ngd = (size_t)ng * bt.ndraw;
        HIPCHECK(hipMemcpyAsync(o.group_value, grp_v.p, ngd * sizeof(double), hipMemcpyDeviceToHost, c->stream));
        if (o.group_offset) HIPCHECK(hipMemcpyAsync(o.group_offset, grp_j.p, ngd * sizeof(int), hipMemcpyDeviceToHost, c->stream));
        HIPCHECK(hipMemcpyAsync(o.group_cand, grp_c.p, ngd * sizeof(int), hipMemcpyDeviceToHost, c->stream));
    }

    // the running best of the run comes down -- with run_shift [ndraw][nrec] on the device, where the family has shifts -- and is
    // folded into the bests of the call; the download's HIP-event time is added to *down_ms
    void finish(float *down_ms, const int *run_shift = nullptr)
    {
        const size_t ndraw = (size_t)bt.ndraw;
        std::vector<double> rv(ndraw);
        std::vector<int> rg(ndraw), rj(ndraw), rc(ndraw), rs(run_shift ? ndraw * nrec : 0);
        const PooledEvents<2> ev(c);
        HIPCHECK(hipEventRecord(ev[0], c->stream));
        HIPCHECK(hipMemcpyAsync(rv.data(), run_v.p, ndraw * sizeof(double), hipMemcpyDeviceToHost, c->stream));
        HIPCHECK(hipMemcpyAsync(rg.data(), run_g.p, ndraw * sizeof(int), hipMemcpyDeviceToHost, c->stream));
        if (bt.best_offset) HIPCHECK(hipMemcpyAsync(rj.data(), run_j.p, ndraw * sizeof(int), hipMemcpyDeviceToHost, c->stream));
        HIPCHECK(hipMemcpyAsync(rc.data(), run_c.p, ndraw * sizeof(int), hipMemcpyDeviceToHost, c->stream));
        if (run_shift) HIPCHECK(hipMemcpyAsync(rs.data(), run_shift, rs.size() * sizeof(int), hipMemcpyDeviceToHost, c->stream));
        HIPCHECK(hipEventRecord(ev[1], c->stream));
        HIPCHECK(hipStreamSynchronize(c->stream));
        ev.add_elapsed(down_ms, 0, 0, 1);
        bt.merge((size_t)nrec, rv.data(), rg.data(), rj.data(), rc.data(), rs.data());
    }
};

// a family's kiwi_hip_*_bootstrap_params piece by piece (PieceCall, kiwi_group_run.hpp): every piece's and device's run folds its bests
// into those of the call under bt.mu.  check(ctx, boot) and run(ctx, ngroup, boot) are the family's check_setup and its run() from
// source 0 of ctx, with the family's other arguments bound
template <class Check, class RunFn>
static PieceCall piece_call(int K, const Boot &bt, Check check, RunFn run)
{
    return PieceCall{ K,
        [=](kiwi_hip_ctx *c) { check(c, bt); },
        [=](kiwi_hip_ctx *c, int s0, int n) { bt.at((size_t)(s0 / K), c->recv.size()).fill_failed((size_t)(n / K), c->recv.size()); },
        [=](kiwi_hip_ctx *c, int s0, int n) { run(c, n / K, bt.at((size_t)(s0 / K), c->recv.size())); } };
}

} // namespace candidates_bootstrap
