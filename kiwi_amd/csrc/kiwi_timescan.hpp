// kiwi_timescan.hpp -- misfits at many origin times from ONE synthesis (kiwi_hip_time_scan).  A source moved by a whole number k of
// samples has the same synthetic, moved: for an uploaded source s and an integer offset k the scan's misfit is what the comparator
// gives when the raw synthetic row of s is read k samples earlier, syn_k[t] = syn_0[t - k] -- the source k dt later -- and everything
// else is as in a plain evaluation: rise-time fold, moment, synthetics factor, the receiver's taper at its fixed place, the
// receiver's filter, the context's misfit method, the references and their norm factors (which do not depend on k).
// Per chunk of trial sources: the rows are made `scan halo` = max |k| samples wider on either side (set_halo), run_chunk with the
// plain synthetics in memory (never the comparator inside the accumulate kernel, never shared synthetics), then ONE workgroup per
// (trial source, slot) pair that brings the folded, scaled, UNTAPERED row over the extended window into LDS once and answers every
// offset from it:
//   time-domain method, slot without filter   taper weight x shifted sample against the tapered reference in misfit_kernel's order,
//                                             kPerPass offsets per pass over the window (taper and reference read once per pass)
//   ampspec_*, or slot with a filter          per offset the tapered shifted row goes through fused_fft_forward (and filter,
//                                             fused_fft_inverse) and the loops of spec_fft_norm_kernel / spec_fft_filter_norm_kernel,
//                                             against the reference variants the plain evaluation of the chunk has just made
// Offset 0 is the plain evaluation bit for bit (KIWI_HIP_FUSE=0 for the unfiltered time-domain methods, as for the bands).
// Included by kiwi_hip.hip, so compiled under its -ffp-contract=off.

namespace timescan {

constexpr int kMaxShift = 1024;                         // |offset| at most, samples
constexpr int kMaxOffsets = 256;                        // offsets per call at most (= threads of time_scan_global_kernel)
constexpr int kPerPass = 4;                             // offsets per pass over the window (unfiltered time-domain methods)
constexpr int kMaxDynLds = 148 * 1024;                  // of the 160 KiB a workgroup may hold: 12 KiB stay for the kernel's static LDS

struct ScanArgs {
    SynRows sr;
    const float *reft;                  // tapered references over the windows
    const float *norm_slot;             // norm factor per slot ...
    const float *norm_src;              // ... or per (uploaded source, slot) where they follow the pair's transform length
    const FftPair *pairs;               // [chunk source][slot] of the plain evaluation; null: no slot goes through the transforms
    FusedFftTables tabs;
    const float *refamp, *filtw, *reffilt, *zmask;
    const int *status;                  // per uploaded source, or null: nobody failed
    int method, spectral, any_filter;
    int nmis, isrc0, k0, kstep, nk, shalo;
    int zf_floats;                      // floats of dynamic LDS in front of the row: the longest transform of the launch
    float dt, syn_factor;
    float *mis_out;                     // [chunk source][offset][slot]
    float *norm_out;                    // [chunk source][slot]
};

// unfiltered time-domain norm of kPerPass shifted rows at a time: row[i - k] x taper against the tapered reference, thread t takes
// samples t, t + 256, ...; fp64 accumulation and the tree of misfit_kernel, per offset
template <int METHOD>
__device__ __forceinline__ void scan_td(const ScanArgs &a, const float *row /* row[e]: extended sample e - shalo */, const float *__restrict__ tp,
                                        const float *__restrict__ rt, int wlen, double (*red)[256], float *__restrict__ out, int tid)
{
    const bool unit = (a.syn_factor == 1.f);
    for (int j0 = 0; j0 < a.nk; j0 += kPerPass) {
        const int nj = min(kPerPass, a.nk - j0);
        const float *rk[kPerPass];
        double acc[kPerPass];
#pragma unroll
        for (int j = 0; j < kPerPass; j++) {
            rk[j] = row + a.shalo - (a.k0 + (j0 + (j < nj ? j : 0)) * a.kstep);       // (past the last offset: the pass's first once more, dropped)
            acc[j] = 0.0;
        }
        for (int i = tid; i < wlen; i += 256) {
            const float w = tp[i], r = rt[i];
#pragma unroll
            for (int j = 0; j < kPerPass; j++) {
                const float vt = rk[j][i] * w;               // make_array_tapered, comparator.f90:1173-1184
                if (METHOD == 1) { const float d = unit ? (r - vt) : (1.f * r - a.syn_factor * vt); acc[j] = sq_acc(acc[j], d); }
                else if (METHOD == 2) { const float d = unit ? fabsf(r - vt) : fabsf(1.f * r - a.syn_factor * vt); acc[j] += (double)d; }
                else if (METHOD == 5) acc[j] += unit ? (double)(r * vt) : (double)(r * 1.f * vt * a.syn_factor);
                else { const double x = (double)(1.f * r), y = (double)(a.syn_factor * vt); acc[j] = fmax(acc[j], sqrt(x * x + y * y)); }
            }
        }
#pragma unroll
        for (int j = 0; j < kPerPass; j++) red[j][tid] = acc[j];
        __syncthreads();
        for (int st = 128; st > 0; st >>= 1) {
            if (tid < st) {
#pragma unroll
                for (int j = 0; j < kPerPass; j++) {
                    if (METHOD == 6) red[j][tid] = fmax(red[j][tid], red[j][tid + st]);
                    else red[j][tid] += red[j][tid + st];
                }
            }
            __syncthreads();
        }
        if (tid < nj) {
            const double tot = red[tid][0];
            float res;
            if (METHOD == 1) res = (float)sqrt((double)a.dt * tot);
            else if (METHOD == 2) res = (float)((double)a.dt * tot);
            else res = (float)tot;
            out[(size_t)(j0 + tid) * a.nmis] = res;
        }
        __syncthreads();                                     // (red is used again)
    }
}

__global__ __launch_bounds__(256) void time_scan_kernel(ScanArgs a)
{
    extern __shared__ __attribute__((aligned(16))) float2 zf[];
    __shared__ double red[kPerPass][256];
    __shared__ float fw[kMaxFold];
    __shared__ int fs[kMaxFold];
    __shared__ float fr[kMaxFold];
    __shared__ int nfold;
    const int tid = threadIdx.x, s = blockIdx.x, m = blockIdx.y;
    if (a.status && a.status[a.isrc0 + s]) return;          // a source the discretiser rejected: time_scan_global_kernel writes its zeros
    const CompDev cd = a.sr.comps[m];
    float *row = reinterpret_cast<float *>(zf) + a.zf_floats;
    const int S = a.shalo, ext = cd.wlen + 2 * S;
    const float mom = a.sr.moment[a.isrc0 + s];
    if (tid == 0) nfold = fold_setup(a.sr.risetime[a.isrc0 + s], a.dt, fw, fs, fr);
    __syncthreads();
    const int nf = nfold;
    const float *__restrict__ sy = a.sr.syn + (size_t)s * a.sr.syn_stride + cd.synofs + cd.halo;      // sy[i] = sample w0 + i; cd.halo = fold halo + S
    const float *__restrict__ tp = a.sr.taper + cd.refofs;
    // the folded, scaled, untapered row over [-S, wlen + S): folded_scaled_sample at every extended index
    for (int e = tid; e < ext; e += 256) row[e] = folded_scaled_sample(sy, e - S, nf, fw, fs, fr, mom);
    __syncthreads();
    const size_t pair = (size_t)s * a.nmis + m;
    if (tid == 0) a.norm_out[pair] = a.norm_src ? a.norm_src[(size_t)(a.isrc0 + s) * a.nmis + m] : a.norm_slot[m];
    float *__restrict__ out = a.mis_out + (size_t)s * a.nk * a.nmis + m;                               // offset j at out[j * nmis]
    if (!a.pairs || !(a.spectral || cd.has_filter)) {       // (workgroup-uniform)
        const float *__restrict__ rt = a.reft + cd.refofs;
        switch (a.method) {
        case 1: scan_td<1>(a, row, tp, rt, cd.wlen, red, out, tid); break;
        case 2: scan_td<2>(a, row, tp, rt, cd.wlen, red, out, tid); break;
        case 5: scan_td<5>(a, row, tp, rt, cd.wlen, red, out, tid); break;
        default: scan_td<6>(a, row, tp, rt, cd.wlen, red, out, tid); break;
        }
        return;
    }
    const FftPair pr = a.pairs[pair];
    const int N = pr.ntrans, M = N >> 1, lg = 31 - __clz(N), lgM = lg - 1;
    const float2 *__restrict__ tab = a.tabs.tab[lg];
    const float *__restrict__ fwt = a.filtw + pr.specofs;
    const bool unit = (a.syn_factor == 1.f);
    for (int j = 0; j < a.nk; j++) {
        const float *rk = row + S - (a.k0 + j * a.kstep);
        // the loaders of spec_fft_norm_kernel<2> / spec_fft_filter_norm_kernel<0>, the row read k samples earlier
#pragma unroll 4
        for (int n = tid; n < M; n += 256) {
            const int i = 2 * n;
            float2 x = make_float2(0.f, 0.f);
            if (i < cd.wlen) x.x = rk[i] * tp[i];           // make_array_tapered, comparator.f90:1173-1184
            if (i + 1 < cd.wlen) x.y = rk[i + 1] * tp[i + 1];
            zf[fused_fft_lds(n)] = x;
        }
        __syncthreads();
        const float2 *__restrict__ tw = fused_fft_forward(zf, tab, M, tid);
        if (a.spectral) {                                   // spec_fft_norm_kernel's bin loop
            const float *__restrict__ ra = a.refamp + pr.specofs;
            double acc = 0.0;
            auto bin = [&](int k, float re, float im) {
                float b = amp2f(re, im);                                         // amp_spectrum = abs(spectrum), comparator.f90:1213
                if (a.any_filter) b = b * fwt[k];                                // make_spectrum_filtered, :1226-1228
                const float r = ra[k];                                           // reference, already filtered
                if (a.method == 3) {
                    const float d = unit ? (r - b) : (1.f * r - a.syn_factor * b);
                    acc = sq_acc(acc, d);
                } else {
                    const float d = unit ? fabsf(r - b) : fabsf(1.f * r - a.syn_factor * b);
                    acc += (double)d;
                }
            };
#pragma unroll 2
            for (int k = tid; k <= (M >> 1); k += 256) {
                const float2 zk = zf[fused_fft_lds(fused_fft_pos(k, lgM))];
                float2 zm = zf[fused_fft_lds(fused_fft_pos((M - k) & (M - 1), lgM))];
                zm.y = -zm.y;                                                    // conj Z[M - k]
                const float2 e = make_float2(0.5f * (zk.x + zm.x), 0.5f * (zk.y + zm.y));
                const float2 o = make_float2(0.5f * (zk.y - zm.y), -0.5f * (zk.x - zm.x));
                const float2 w = tw[k];
                const float2 xp = cmaddf(e, w, o), xm = cmaddf(e, make_float2(-w.x, -w.y), o);
                bin(k, xp.x, xp.y);
                if (2 * k != M) bin(M - k, xm.x, xm.y);
            }
            const double tot = block_sum(acc, red[0]);
            if (tid == 0) {
                const float df = 1.f / ((float)N * a.dt);                        // comparator.f90:1215
                out[(size_t)j * a.nmis] = (a.method == 3) ? (float)sqrt((double)df * tot) : (float)((double)df * tot);
            }
            __syncthreads();                                                     // (red and the row in zf are used again)
            continue;
        }
        // spectrum x filter, packed for the way back (spec_fft_filter_norm_kernel)
#pragma unroll 2
        for (int k = tid; k <= (M >> 1); k += 256) {
            const int pk = fused_fft_lds(fused_fft_pos(k, lgM)), pm = fused_fft_lds(fused_fft_pos((M - k) & (M - 1), lgM));
            const float2 zk = zf[pk];
            float2 zm = zf[pm];
            zm.y = -zm.y;                                                        // conj Z[M - k]
            const float2 e = make_float2(0.5f * (zk.x + zm.x), 0.5f * (zk.y + zm.y));
            const float2 o = make_float2(0.5f * (zk.y - zm.y), -0.5f * (zk.x - zm.x));
            const float2 w = tw[k];
            const float2 xp = cmaddf(e, w, o), xm = cmaddf(e, make_float2(-w.x, -w.y), o);
            const float fk = fwt[k], fm = fwt[M - k];
            const float2 yk = make_float2(xp.x * fk, xp.y * fk);                              // spectrum * filter, comparator.f90:1224-1225
            const float2 ym = make_float2(xm.x * fm, xm.y * fm);                              // conj of bin M - k, filtered
            const float2 A = make_float2(yk.x + ym.x, yk.y + ym.y);
            const float2 B = cmulf(make_float2(yk.x - ym.x, yk.y - ym.y), make_float2(w.x, -w.y));
            zf[pk] = make_float2(A.x - B.y, A.y + B.x);                                       // A + i B
            if (pm != pk) zf[pm] = make_float2(A.x + B.y, B.x - A.y);                         // conj A + i conj B
        }
        __syncthreads();
        fused_fft_inverse(zf, tab, M, tid);
        const float res = bands::row_norm(zf, a.reffilt + pr.filtofs, a.zmask + cd.refofs, true, cd.wlen, N, a.method, a.syn_factor, a.dt, red[0], tid);
        if (tid == 0) out[(size_t)j * a.nmis] = res;
    }
}

// global misfit per (chunk source, offset): global_kernel's sums over the slots, and per source the index of the smallest one
// (lowest index among equal values, a NaN before any number: numpy's argmin).  One workgroup per source, thread j takes offset j;
// a source the discretiser rejected reads as zeros, best = -1
__global__ __launch_bounds__(kMaxOffsets) void time_scan_global_kernel(float *__restrict__ mis, float *__restrict__ norm, const int *__restrict__ rec_first,
                                                                       int nrec_en, int nmis, int nk, int isrc0, float *__restrict__ glob,
                                                                       int *__restrict__ best, const int *__restrict__ status)
{
    __shared__ float g[kMaxOffsets];
    const int s = blockIdx.x, j = threadIdx.x;
    float *n = norm + (size_t)s * nmis;
    if (status && status[isrc0 + s]) {
        float *mz = mis + (size_t)s * nk * nmis;
        for (int i = j; i < nk * nmis; i += kMaxOffsets) mz[i] = 0.f;
        for (int i = j; i < nmis; i += kMaxOffsets) n[i] = 0.f;
        if (j < nk) glob[(size_t)s * nk + j] = 0.f;
        if (j == 0) best[s] = -1;
        return;
    }
    if (j < nk) {
        const float *m = mis + ((size_t)s * nk + j) * nmis;
        float tm = 0.f, tn = 0.f;
        for (int r = 0; r < nrec_en; r++) {
            float x = 0.f, y = 0.f;
            for (int k = rec_first[r]; k < rec_first[r + 1]; k++) x = x + m[k] * m[k];
            for (int k = rec_first[r]; k < rec_first[r + 1]; k++) y = y + n[k] * n[k];
            tm = tm + x;
            tn = tn + y;
        }
        g[j] = sqrtf(tm) / sqrtf(tn);
        glob[(size_t)s * nk + j] = g[j];
    }
    __syncthreads();
    if (j == 0) {
        int b = 0;
        float v = g[0];
        for (int q = 1; q < nk; q++)
            if (g[q] < v || (g[q] != g[q] && v == v)) { v = g[q]; b = q; }
        best[s] = b;
    }
}

// host arrays of the caller for the sources of ONE call of run(); any may be null
struct Out {
    float *misfit, *norm, *global;
    int *best;
    Out at(size_t s0, size_t nk, size_t nmis) const
    {
        return Out{ misfit ? misfit + s0 * nk * nmis : nullptr, norm ? norm + s0 * nmis : nullptr, global ? global + s0 * nk : nullptr,
                    best ? best + s0 : nullptr };
    }
};

struct Offsets { int k0, kstep, nk; int max_abs() const { return std::max(std::abs(k0), std::abs(k0 + (nk - 1) * kstep)); } };

static void fill_failed(size_t nsrc, size_t nk, size_t nmis, const Out &out)
{
    if (out.misfit) std::memset(out.misfit, 0, nsrc * nk * nmis * sizeof(float));
    if (out.norm) std::memset(out.norm, 0, nsrc * nmis * sizeof(float));
    if (out.global) std::memset(out.global, 0, nsrc * nk * sizeof(float));
    if (out.best) std::fill(out.best, out.best + nsrc, -1);
}

// what the call cannot do is refused, nothing approximated.  Leaves the context prepared.
static void check_setup(kiwi_hip_ctx *c, int k0, int kstep, int nk)
{
    if (nk < 1) throw std::runtime_error("time_scan: nk = " + std::to_string(nk) + "; need at least one offset");
    if (nk > kMaxOffsets) throw std::runtime_error("time_scan: nk = " + std::to_string(nk) + " offsets; at most " + std::to_string(kMaxOffsets) + " are supported");
    if (kstep < 1) throw std::runtime_error("time_scan: kstep = " + std::to_string(kstep) + "; the step between offsets is at least one sample");
    const long long klast = (long long)k0 + (long long)(nk - 1) * kstep;
    if (k0 < -kMaxShift || k0 > kMaxShift || klast > kMaxShift)
        throw std::runtime_error("time_scan: offsets " + std::to_string(k0) + " .. " + std::to_string(klast) + " samples; the largest shift is " +
                                 std::to_string(kMaxShift) + " samples either way");
    if (c->method == KIWI_FLOATING_L2NORM || c->method == KIWI_FLOATING_L1NORM)
        throw std::runtime_error("time_scan: the context's misfit method is a floating norm, which already is a minimum over shifts; set another method");
    prepare(c);
    if (c->synth_only) throw std::runtime_error("time_scan: every enabled receiver component needs a reference seismogram");
    if (c->any_untapered)
        throw std::runtime_error("time_scan: an enabled receiver has no misfit taper (its comparison span follows the source, which the scan moves)");
}

// Rows of wlen + 2 halo samples per slot: the layout of prepare() for another halo.  Windows, references, tapers and every table laid
// over the windows stay; only where a slot's row begins inside a source's block, and how long it is, change.
static void set_halo(kiwi_hip_ctx *c, int halo)
{
    size_t synofs = 0;
    c->max_wlen = 0;
    for (RecvDev &d : c->recv_h) {
        if (!d.enabled) continue;
        d.wbeg = c->comps[(size_t)d.slot0].w0 - halo;
        d.wlen = c->comps[(size_t)d.slot0].wlen + 2 * halo;
        c->max_wlen = std::max(c->max_wlen, d.wlen);
        for (int k = 0; k < d.ncomp; k++) {
            CompDev &cd = c->comps[(size_t)d.slot0 + k];
            cd.synofs = (int)synofs; cd.halo = halo;
            d.synofs[k] = (int)synofs;
            synofs += ((size_t)d.wlen + 3) / 4 * 4;
        }
    }
    c->halo = halo;
    c->syn_stride = synofs;
    HIPCHECK(hipMemcpyAsync(c->recv_d.p, c->recv_h.data(), c->recv_h.size() * sizeof(RecvDev), hipMemcpyHostToDevice, c->stream));
    HIPCHECK(hipMemcpyAsync(c->comps_d.p, c->comps.data(), c->comps.size() * sizeof(CompDev), hipMemcpyHostToDevice, c->stream));
    HIPCHECK(hipStreamSynchronize(c->stream));
}

// for the length of a scan: the halo widened by `more` samples and every source synthesised with its own strip spans kept; both
// are put back on the way out, also where widen() itself threw
struct HaloScope {
    kiwi_hip_ctx *c; bool want; int halo;
    explicit HaloScope(kiwi_hip_ctx *ctx) : c(ctx), want(ctx->want_spansrc), halo(ctx->halo) {}
    void widen(int more)
    {
        c->want_spansrc = true;
        set_halo(c, halo + more);
    }
    ~HaloScope()
    {
        c->want_spansrc = want;
        try { HIPCHECK(hipSetDevice(c->device)); set_halo(c, halo); }
        catch (...) { c->prepared = false; }               // (the next call lays everything out again)
    }
    HaloScope(const HaloScope &) = delete;
    HaloScope &operator=(const HaloScope &) = delete;
};

// the sources [isrc0, isrc0 + nsrc) of the uploaded batch; adds its HIP-event times to c->timescan_ms
static void run(kiwi_hip_ctx *c, int isrc0, int nsrc, const Offsets &of, const Out &out)
{
    check_setup(c, of.k0, of.kstep, of.nk);
    check_group_range("time_scan", c, isrc0, nsrc, 1);
    if (nsrc == 0) return;
    TimeScanState &st = c->timescan_state;
    const int nmis = c->nmis, nk = of.nk;
    const bool spectral = c->method == KIWI_AMPSPEC_L2NORM || c->method == KIWI_AMPSPEC_L1NORM;
    if (c->fft_needed && !c->fused_fft)
        throw std::runtime_error("time_scan: slots with a frequency filter or an amplitude-spectrum method go through the in-LDS transforms, "
                                 "which KIWI_HIP_FUSED_FFT=0 switches off");
    c->misfit_d.ensure((size_t)c->nsrc * c->nmis, &c->dev_bytes);
    c->global_d.ensure((size_t)c->nsrc, &c->dev_bytes);
    if (c->fft_needed && !c->fft_ready) prepare_fft(c, c->reft_h);
    // the row in LDS beside the longest transform a slot of this batch can need (prepare_fft's bound: the same for every chunk)
    const int base = c->halo, shalo = of.max_abs();
    int max_w = 0, ntr_bound = 0;
    for (const CompDev &cd : c->comps) {
        max_w = std::max(max_w, cd.wlen);
        if (c->fft_needed && (spectral || cd.has_filter)) ntr_bound = std::max(ntr_bound, std::min(cd.ntrans_max, 1 << kFusedFftMaxLog2));
    }
    const int row_len = max_w + 2 * (base + shalo), row_limit = kMaxDynLds / 4 - ntr_bound;
    if (row_len > row_limit)
        throw std::runtime_error("time_scan: a row of " + std::to_string(row_len) + " samples (window " + std::to_string(max_w) + " + 2 x halo " +
                                 std::to_string(base + shalo) + ") does not fit in LDS" +
                                 (ntr_bound ? " beside a transform of " + std::to_string(ntr_bound) + " samples" : std::string()) + "; the limit is " +
                                 std::to_string(row_limit));
    c->fuse_now = false;                                   // the plain synthetics go to memory
    // every source is synthesised (run_chunk shares no synthetics between sources then), with its own strip spans kept
    HaloScope halo(c);
    halo.widen(shalo);
    if (!st.attr) {
        HIPCHECK(hipFuncSetAttribute(reinterpret_cast<const void *>(&time_scan_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, kMaxDynLds));
        st.attr = true;
    }

    const PooledEvents<4> ev(c);
    int s = isrc0;
    while (s < isrc0 + nsrc) {
        // a chunk of sources (groups of one), the outputs nk times those of a plain call
        const int n = next_group_chunk(c, isrc0, s - isrc0, nsrc, 1, 1, ((size_t)nk * nmis + nmis + nk + 1) * sizeof(float),
                                       c->fft_needed ? c->fft_cap : kNoSourceCap);
        HIPCHECK(hipEventRecord(ev[0], c->stream));
        run_chunk(c, s, n, 0);
        HIPCHECK(hipEventRecord(ev[1], c->stream));
        int longest = 0;
        if (c->fft_needed) {                               // (layout_fft_chunk has waited for the transform lengths of the chunk)
            for (size_t i = 0; i < (size_t)n * nmis; i++) {
                const int m = (int)(i % (size_t)nmis), nt = c->ntr_pin[i];
                if (!spectral && !c->comps[(size_t)m].has_filter) continue;
                if (nt < (1 << kFusedFftMinLog2) || nt > (1 << kFusedFftMaxLog2))
                    throw std::runtime_error("time_scan: source " + std::to_string(s + (int)(i / (size_t)nmis) + 1) + ", misfit slot " + std::to_string(m + 1) +
                                             " needs a transform of " + std::to_string(nt) + " samples; the in-LDS transforms take " +
                                             std::to_string(1 << kFusedFftMinLog2) + " to " + std::to_string(1 << kFusedFftMaxLog2));
                longest = std::max(longest, nt);
            }
        }
        const size_t nout = (size_t)n * nk * nmis;
        st.mis_d.ensure(nout, &c->dev_bytes); st.norm_d.ensure((size_t)n * nmis, &c->dev_bytes);
        st.glob_d.ensure((size_t)n * nk, &c->dev_bytes); st.best_d.ensure((size_t)n, &c->dev_bytes);
        ScanArgs a;
        a.sr = SynRows{ c->syn_d.p, c->syn_stride, c->comps_d.p, c->tw_d.p, c->moment_d.p, c->risetime_d.p, nullptr };
        a.reft = c->reft_d.p;
        a.norm_slot = c->norm_d.p;
        a.norm_src = c->fft_needed ? c->normsrc_d.p : nullptr;
        a.pairs = c->fft_needed ? c->pairs_d.p : nullptr;
        a.tabs = c->fft_needed ? fused_fft_tables(c) : FusedFftTables{};
        a.refamp = c->refamp_d.p; a.filtw = c->filtw_d.p; a.reffilt = c->reffilt_d.p; a.zmask = c->zmask_d.p;
        a.status = c->any_failed ? c->status_d.p : nullptr;
        a.method = c->method; a.spectral = spectral ? 1 : 0; a.any_filter = c->any_filter ? 1 : 0;
        a.nmis = nmis; a.isrc0 = s; a.k0 = of.k0; a.kstep = of.kstep; a.nk = nk; a.shalo = shalo;
        a.zf_floats = longest;
        a.dt = c->gm.dt; a.syn_factor = c->syn_factor;
        a.mis_out = st.mis_d.p; a.norm_out = st.norm_d.p;
        const size_t dyn = ((size_t)longest + (size_t)max_w + 2 * (size_t)shalo) * sizeof(float);      // <= kMaxDynLds: row_limit above
        hipLaunchKernelGGL(time_scan_kernel, dim3((unsigned)n, (unsigned)nmis), dim3(256), dyn, c->stream, a);
        hipLaunchKernelGGL(time_scan_global_kernel, dim3((unsigned)n), dim3(kMaxOffsets), 0, c->stream, st.mis_d.p, st.norm_d.p, c->recfirst_d.p,
                           c->nrec_en, nmis, nk, s, st.glob_d.p, st.best_d.p, c->any_failed ? c->status_d.p : (const int *)nullptr);
        HIPCHECK(hipGetLastError());
        HIPCHECK(hipEventRecord(ev[2], c->stream));
        const Out o = out.at((size_t)(s - isrc0), (size_t)nk, (size_t)nmis);
        if (o.misfit) HIPCHECK(hipMemcpyAsync(o.misfit, st.mis_d.p, nout * sizeof(float), hipMemcpyDeviceToHost, c->stream));
        if (o.norm) HIPCHECK(hipMemcpyAsync(o.norm, st.norm_d.p, (size_t)n * nmis * sizeof(float), hipMemcpyDeviceToHost, c->stream));
        if (o.global) HIPCHECK(hipMemcpyAsync(o.global, st.glob_d.p, (size_t)n * nk * sizeof(float), hipMemcpyDeviceToHost, c->stream));
        if (o.best) HIPCHECK(hipMemcpyAsync(o.best, st.best_d.p, (size_t)n * sizeof(int), hipMemcpyDeviceToHost, c->stream));
        HIPCHECK(hipEventRecord(ev[3], c->stream));
        HIPCHECK(hipStreamSynchronize(c->stream));
        for (int i = 0; i < 3; i++) ev.add_elapsed(c->timescan_ms, i, i, i + 1);
        s += n;
    }
    leave_evaluated(c, isrc0, nsrc, 0);                    // the plain evaluation -- offset 0 -- was made on the way
}

// kiwi_hip_time_scan_for_params piece by piece (PieceCall, kiwi_group_run.hpp): plain sources
static PieceCall piece_call(const Offsets &of, const Out &out)
{
    return PieceCall{ 1,
        [=](kiwi_hip_ctx *c) { check_setup(c, of.k0, of.kstep, of.nk); },
        [=](kiwi_hip_ctx *c, int s0, int n) { fill_failed((size_t)n, (size_t)of.nk, (size_t)c->nmis, out.at((size_t)s0, (size_t)of.nk, (size_t)c->nmis)); },
        [=](kiwi_hip_ctx *c, int s0, int n) { run(c, 0, n, of, out.at((size_t)s0, (size_t)of.nk, (size_t)c->nmis)); } };
}

} // namespace timescan
