// kiwi_bands.hpp -- misfits in several frequency bands and norms from ONE synthesis (kiwi_hip_band_misfits).  A band is a misfit
// method (ids 1 to 6) plus an optional frequency filter, the same for every receiver (what kiwi_hip_set_filter(ctx, 0, ...) means).
// Per chunk of trial sources: run_chunk with the plain synthetics in memory (never the comparator inside the accumulate kernel, never
// shared synthetics), then ONE workgroup per (trial source, slot) pair that
// brings the pair's row into LDS once -- rise-time fold, moment and taper on the way in, exactly the loaders of
// spec_fft_norm_kernel<2> / spec_fft_filter_norm_kernel<0> -- and answers every band from it:
//   time-domain method, no filter    reduced straight from the tapered samples in misfit_kernel's order
//   ampspec_*                        one fused_fft_forward; every such band is a weighted sum over the bins of that one spectrum
//                                    (spec_fft_norm_kernel's bin loop), up to four bands per pass over the bins
//   time-domain method with filter   spectrum x filter, repacked, fused_fft_inverse, / N, zero mask, norm: the loops of
//                                    spec_fft_filter_norm_kernel<0>.  The inverse overwrites the spectrum; with two or more such
//                                    bands it is kept in a second LDS copy where 2 x (N / 2) x 8 bytes fit beside the kernel's
//                                    static LDS (N <= 16384), else the row is loaded and transformed again
// The reference side of a band -- refamp, reffilt, filtw per (band, slot, transform length), zero mask, norm factors -- is made by
// the existing mode-1 kernels and host loops, so band b is bit for bit what kiwi_hip_get_misfits returns after
// kiwi_hip_set_filter(ctx, 0, band b's filter) + kiwi_hip_set_misfit_method(ctx, band b's method) + kiwi_hip_eval.  Included by
// kiwi_hip.hip, so compiled under its -ffp-contract=off.

namespace bands {

constexpr int kMaxBands = 16;
constexpr int kLg = 16;                                 // entries per (band, slot) of the variant tables: log2 of the transform length
constexpr int kMaxDynLds = 152 * 1024;                  // of the 160 KiB a workgroup may hold: 8 KiB stay for the kernel's static LDS

static inline bool is_spectral(int method) { return method == KIWI_AMPSPEC_L2NORM || method == KIWI_AMPSPEC_L1NORM; }

// which bands go which way, made on the host (the kernel reads it with scalar loads)
struct BandTab {
    int ntd, nfilt, nspec, nband;
    int td[kMaxBands], filt[kMaxBands], spec[kMaxBands];      // band indices: unfiltered time-domain, filtered time-domain, spectral
    int method[kMaxBands], has_filter[kMaxBands];
};

struct BandArgs {
    SynRows sr;
    const float *reft;                  // tapered references over the windows
    const int *ntr;                     // transform length per (chunk source, slot); null: no band needs the spectrum
    FusedFftTables tabs;
    const BandTab *bt;
    const int2 *vtab;                   // [(band * nmis + slot) * kLg + log2 N]: (specofs, filtofs) of the reference variant
    const float *normtab;               // same index: norm factor
    const float *refamp, *filtw, *reffilt, *zmask;
    int nband, nmis, isrc0, dyn_bytes;
    float dt, syn_factor;
    float *mis_out, *norm_out;          // [chunk source][band][slot]
};

// time-domain norm of the row in LDS against `ref` over the window; thread t takes samples t, t + 256, ...; fp64 accumulation
// (misfit_kernel).  filtered: the row is the unnormalised inverse transform -- / N and the zero mask first
// (spec_fft_filter_norm_kernel).  The result is valid in thread 0; ends with a barrier.
__device__ __forceinline__ float row_norm(const float2 *zf, const float *__restrict__ ref, const float *__restrict__ zm, bool filtered, int wlen,
                                          int N, int method, float syn_factor, float dt, double *red, int tid)
{
    const bool unit = (syn_factor == 1.f);
    double acc = 0.0, peak = 0.0;
    for (int i = tid; i < wlen; i += 256) {
        const float2 z = zf[fused_fft_lds(i >> 1)];
        float v = (i & 1) ? z.y : z.x;
        if (filtered) {
            v = v / (float)N;                                            // normalize result, comparator.f90:1251
            v = v * zm[i];                                               // :1254-1258
        }
        const float a = ref[i];
        switch (method) {
        case 1: { const float d = unit ? (a - v) : (1.f * a - syn_factor * v); acc = sq_acc(acc, d); break; }
        case 2: { const float d = unit ? fabsf(a - v) : fabsf(1.f * a - syn_factor * v); acc += (double)d; break; }
        case 5: acc += unit ? (double)(a * v) : (double)(a * 1.f * v * syn_factor); break;
        default: { const double x = (double)(1.f * a), y = (double)(syn_factor * v); peak = fmax(peak, sqrt(x * x + y * y)); break; }
        }
    }
    red[tid] = (method == 6) ? peak : acc;
    __syncthreads();
    for (int st = 128; st > 0; st >>= 1) {
        if (tid < st) {
            if (method == 6) red[tid] = fmax(red[tid], red[tid + st]);
            else red[tid] += red[tid + st];
        }
        __syncthreads();
    }
    const double tot = red[0];
    __syncthreads();                                                     // (red is used again)
    switch (method) {
    case 1: return (float)sqrt((double)dt * tot);
    case 2: return (float)((double)dt * tot);
    default: return (float)tot;
    }
}

__global__ __launch_bounds__(256) void band_kernel(BandArgs a)
{
    extern __shared__ __attribute__((aligned(16))) float2 zf[];
    __shared__ double red[256];
    __shared__ float fw[kMaxFold];
    __shared__ int fs[kMaxFold];
    __shared__ float fr[kMaxFold];
    __shared__ int nfold;
    const int tid = threadIdx.x, s = blockIdx.x, m = blockIdx.y;
    const BandTab *__restrict__ bt = a.bt;
    const CompDev cd = a.sr.comps[m];
    int N;
    if (a.ntr) N = a.ntr[(size_t)s * a.nmis + m];
    else { N = 1 << kFusedFftMinLog2; while (N < cd.wlen) N <<= 1; }     // no transform: the row only has to hold the window
    const int M = N >> 1, lg = 31 - __clz(N);
    const int ntd = bt->ntd, nfilt = bt->nfilt, nspec = bt->nspec;
    const bool use_copy = nfilt >= 2 && 8 * N <= a.dyn_bytes;            // (workgroup-uniform)
    float2 *zc = zf + M;
    const float mom = a.sr.moment[a.isrc0 + s];
    if (tid == 0) nfold = fold_setup(a.sr.risetime[a.isrc0 + s], a.dt, fw, fs, fr);
    __syncthreads();
    const int nf = nfold;
    const float *__restrict__ sy = a.sr.syn + (size_t)(a.sr.synrow ? a.sr.synrow[s] : s) * a.sr.syn_stride + cd.synofs + cd.halo;
    const float *__restrict__ tp = a.sr.taper + cd.refofs;
    const float *__restrict__ rt = a.reft + cd.refofs;
    const float *__restrict__ zm_ = a.zmask + cd.refofs;
    const size_t orow = (size_t)s * a.nband * a.nmis + m;
    if (tid < a.nband) a.norm_out[orow + (size_t)tid * a.nmis] = a.normtab[(((size_t)tid * a.nmis + m) << 4) + lg];
    const float2 *__restrict__ tab = a.ntr ? a.tabs.tab[lg] : nullptr;
    const float2 *__restrict__ tw = nullptr;
    const bool unit = (a.syn_factor == 1.f);
    const int lgM = lg - 1;
    for (int pass = 0; pass == 0 || pass < nfilt; pass++) {
        if (pass == 0 || !use_copy) {
#pragma unroll 4
            for (int n = tid; n < M; n += 256) {
                const int i = 2 * n;
                float2 x = make_float2(0.f, 0.f);
                if (i < cd.wlen) x.x = folded_scaled_sample(sy, i, nf, fw, fs, fr, mom) * tp[i];           // make_array_tapered, comparator.f90:1173-1184
                if (i + 1 < cd.wlen) x.y = folded_scaled_sample(sy, i + 1, nf, fw, fs, fr, mom) * tp[i + 1];
                zf[fused_fft_lds(n)] = x;
            }
            __syncthreads();
            if (pass == 0)
                for (int j = 0; j < ntd; j++) {
                    const int b = bt->td[j];
                    const float res = row_norm(zf, rt, zm_, false, cd.wlen, N, bt->method[b], a.syn_factor, a.dt, red, tid);
                    if (tid == 0) a.mis_out[orow + (size_t)b * a.nmis] = res;
                }
            if (a.ntr) {
                tw = fused_fft_forward(zf, tab, M, tid);
                if (pass == 0) {
                    for (int g0 = 0; g0 < nspec; g0 += 4) {              // up to four spectral bands per pass over the bins
                        int bb[4], meth[4], hf[4];
                        const float *ra[4], *fwt[4];
                        double acc[4];
#pragma unroll
                        for (int j = 0; j < 4; j++) {
                            bb[j] = g0 + j < nspec ? bt->spec[g0 + j] : -1;
                            const int b = bb[j] < 0 ? 0 : bb[j];
                            const int2 v = a.vtab[(((size_t)b * a.nmis + m) << 4) + lg];
                            meth[j] = bt->method[b]; hf[j] = bt->has_filter[b];
                            ra[j] = a.refamp + v.x; fwt[j] = a.filtw + v.x;
                            acc[j] = 0.0;
                        }
                        auto bin = [&](int k, float re, float im) {
                            const float amp = amp2f(re, im);                             // amp_spectrum = abs(spectrum), comparator.f90:1213
#pragma unroll
                            for (int j = 0; j < 4; j++) {
                                if (bb[j] < 0) continue;
                                float b = amp;
                                if (hf[j]) b = b * fwt[j][k];                            // make_spectrum_filtered, :1226-1228
                                const float r = ra[j][k];                                // reference, already filtered
                                if (meth[j] == 3) {
                                    const float d = unit ? (r - b) : (1.f * r - a.syn_factor * b);
                                    acc[j] = sq_acc(acc[j], d);
                                } else {
                                    const float d = unit ? fabsf(r - b) : fabsf(1.f * r - a.syn_factor * b);
                                    acc[j] += (double)d;
                                }
                            }
                        };
#pragma unroll 2
                        for (int k = tid; k <= (M >> 1); k += 256) {
                            const float2 zk = zf[fused_fft_lds(fused_fft_pos(k, lgM))];
                            float2 zm = zf[fused_fft_lds(fused_fft_pos((M - k) & (M - 1), lgM))];
                            zm.y = -zm.y;                                                // conj Z[M - k]
                            const float2 e = make_float2(0.5f * (zk.x + zm.x), 0.5f * (zk.y + zm.y));
                            const float2 o = make_float2(0.5f * (zk.y - zm.y), -0.5f * (zk.x - zm.x));
                            const float2 w = tw[k];
                            const float2 xp = cmaddf(e, w, o), xm = cmaddf(e, make_float2(-w.x, -w.y), o);
                            bin(k, xp.x, xp.y);
                            if (2 * k != M) bin(M - k, xm.x, xm.y);
                        }
#pragma unroll
                        for (int j = 0; j < 4; j++) {
                            if (bb[j] < 0) continue;                                     // (uniform)
                            const double tot = block_sum(acc[j], red);
                            if (tid == 0) {
                                const float df = 1.f / ((float)N * a.dt);                // comparator.f90:1215
                                a.mis_out[orow + (size_t)bb[j] * a.nmis] = (meth[j] == 3) ? (float)sqrt((double)df * tot) : (float)((double)df * tot);
                            }
                            __syncthreads();                                             // (red is used again)
                        }
                    }
                    if (use_copy) {
                        for (int n = tid; n < M; n += 256) zc[n] = zf[n];
                        __syncthreads();
                    }
                }
            }
        }
        if (nfilt == 0) break;
        // the pass-th filtered time-domain band: spectrum x filter, packed for the way back (spec_fft_filter_norm_kernel)
        const int b = bt->filt[pass];
        const int2 vo = a.vtab[(((size_t)b * a.nmis + m) << 4) + lg];
        const float *__restrict__ fwt = a.filtw + vo.x;
        const float2 *src = use_copy ? zc : zf;
#pragma unroll 2
        for (int k = tid; k <= (M >> 1); k += 256) {
            const int pk = fused_fft_lds(fused_fft_pos(k, lgM)), pm = fused_fft_lds(fused_fft_pos((M - k) & (M - 1), lgM));
            const float2 zk = src[pk];
            float2 zm = src[pm];
            zm.y = -zm.y;                                                    // conj Z[M - k]
            const float2 e = make_float2(0.5f * (zk.x + zm.x), 0.5f * (zk.y + zm.y));
            const float2 o = make_float2(0.5f * (zk.y - zm.y), -0.5f * (zk.x - zm.x));
            const float2 w = tw[k];
            const float2 xp = cmaddf(e, w, o), xm = cmaddf(e, make_float2(-w.x, -w.y), o);
            const float fk = fwt[k], fm = fwt[M - k];
            const float2 yk = make_float2(xp.x * fk, xp.y * fk);                          // spectrum * filter, comparator.f90:1224-1225
            const float2 ym = make_float2(xm.x * fm, xm.y * fm);                          // conj of bin M - k, filtered
            const float2 A = make_float2(yk.x + ym.x, yk.y + ym.y);
            const float2 B = cmulf(make_float2(yk.x - ym.x, yk.y - ym.y), make_float2(w.x, -w.y));
            zf[pk] = make_float2(A.x - B.y, A.y + B.x);                                   // A + i B
            if (pm != pk) zf[pm] = make_float2(A.x + B.y, B.x - A.y);                     // conj A + i conj B
        }
        __syncthreads();
        fused_fft_inverse(zf, tab, M, tid);
        const float res = row_norm(zf, a.reffilt + vo.y, zm_, true, cd.wlen, N, bt->method[b], a.syn_factor, a.dt, red, tid);
        if (tid == 0) a.mis_out[orow + (size_t)b * a.nmis] = res;
    }
}

// global misfit per (chunk source, band): global_kernel's sums over the band's slots; a source the discretiser rejected reads as zeros
__global__ void band_global_kernel(float *__restrict__ mis, float *__restrict__ norm, const int *__restrict__ rec_first, int nrec_en, int nmis,
                                   int nband, int isrc0, int nsrc, float *__restrict__ glob, const int *__restrict__ status)
{
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= nsrc * nband) return;
    const int s = idx / nband;
    float *m = mis + (size_t)idx * nmis, *n = norm + (size_t)idx * nmis;
    if (status && status[isrc0 + s]) {
        for (int k = 0; k < nmis; k++) { m[k] = 0.f; n[k] = 0.f; }
        glob[idx] = 0.f;
        return;
    }
    float tm = 0.f, tn = 0.f;
    for (int r = 0; r < nrec_en; r++) {
        float x = 0.f, y = 0.f;
        for (int k = rec_first[r]; k < rec_first[r + 1]; k++) x = x + m[k] * m[k];
        for (int k = rec_first[r]; k < rec_first[r + 1]; k++) y = y + n[k] * n[k];
        tm = tm + x;
        tn = tn + y;
    }
    glob[idx] = sqrtf(tm) / sqrtf(tn);
}

// host arrays of the caller for the sources of ONE call of run(); any may be null
struct Out {
    float *misfit, *norm, *global;
    Out at(size_t s0, size_t nband, size_t nmis) const
    {
        return Out{ misfit ? misfit + s0 * nband * nmis : nullptr, norm ? norm + s0 * nband * nmis : nullptr, global ? global + s0 * nband : nullptr };
    }
};

static void fill_failed(size_t nsrc, size_t nband, size_t nmis, const Out &out)
{
    if (out.misfit) std::memset(out.misfit, 0, nsrc * nband * nmis * sizeof(float));
    if (out.norm) std::memset(out.norm, 0, nsrc * nband * nmis * sizeof(float));
    if (out.global) std::memset(out.global, 0, nsrc * nband * sizeof(float));
}

// what the call cannot do is refused, nothing approximated.  Leaves the context prepared.
static void check_setup(kiwi_hip_ctx *c)
{
    if (c->bands.empty()) throw std::runtime_error("band_misfits: no misfit bands set (kiwi_hip_set_misfit_bands)");
    if (c->method == KIWI_FLOATING_L2NORM || c->method == KIWI_FLOATING_L1NORM)
        throw std::runtime_error("band_misfits: the context's misfit method is a floating norm, which the band call does not evaluate; set another method");
    prepare(c);
    if (c->synth_only) throw std::runtime_error("band_misfits: every enabled receiver component needs a reference seismogram");
    if (c->any_untapered)
        throw std::runtime_error("band_misfits: an enabled receiver has no misfit taper (its transform length and comparison span follow the source and the reference, "
                                 "not a window the bands could share)");
}

// reference side of the bands: tables per (band, slot, transform length), kept while the context's prepared state and the bands stay
static void reset_cache(kiwi_hip_ctx *c)
{
    BandState &st = c->band_state;
    st.prepare_gen = c->prepare_gen; st.valid = true;
    st.refamp_h.clear(); st.filtw_h.clear(); st.reffilt_h.clear();
    const int nband = (int)c->bands.size(), nmis = c->nmis;
    st.vtab_h.assign((size_t)nband * nmis * kLg, make_int2(-1, -1));
    st.normtab_h.assign((size_t)nband * nmis * kLg, 0.f);
    const float dt = c->gm.dt;
    BandTab bt;
    std::memset(&bt, 0, sizeof(bt));
    bt.nband = nband;
    for (int b = 0; b < nband; b++) {
        const BandDef &bd = c->bands[(size_t)b];
        bt.method[b] = bd.method; bt.has_filter[b] = bd.filter.defined() ? 1 : 0;
        if (is_spectral(bd.method)) bt.spec[bt.nspec++] = b;
        else if (bd.filter.defined()) bt.filt[bt.nfilt++] = b;
        else {
            bt.td[bt.ntd++] = b;
            // norm factor of a time-domain band without filter: probe_norm over the tapered reference (the host loop of prepare())
            for (int m = 0; m < nmis; m++) {
                const CompDev &cd = c->comps[(size_t)m];
                double sum = 0.0, pk = 0.0;
                for (int i = 0; i < cd.wlen; i++) {
                    const float v = c->reft_h[(size_t)cd.refofs + i];
                    switch (bd.method) {
                    case KIWI_L2NORM: sum += (double)v * (double)v; break;
                    case KIWI_L1NORM: sum += (double)std::fabs(v); break;
                    case KIWI_SCALAR_PRODUCT: sum += (double)(v * v); break;
                    default: pk = std::max(pk, (double)std::fabs(v)); break;
                    }
                }
                float nf;
                switch (bd.method) {
                case KIWI_L2NORM: nf = 1.f * (float)std::sqrt((double)dt * sum); break;
                case KIWI_L1NORM: nf = 1.f * (float)((double)dt * sum); break;
                case KIWI_SCALAR_PRODUCT: nf = (1.f * 1.f) * (float)sum; break;
                default: nf = 1.f * (float)pk; break;
                }
                for (int lg = 0; lg < kLg; lg++) st.normtab_h[((size_t)b * nmis + m) * kLg + lg] = nf;
            }
        }
    }
    st.need_spec = bt.nspec + bt.nfilt > 0;
    st.nfilt = bt.nfilt;
    // slot records that say "filtered" (the mode-1 kernel of the filtered references asks), zero/one mask of the tapers (prepare_fft)
    std::vector<CompDev> comps = c->comps;
    for (auto &cd : comps) cd.has_filter = 1;
    std::vector<float> zm(c->reft_h.size(), 1.f);
    for (const CompDev &cd : c->comps)
        plf_taper_array(c->recv[(size_t)cd.rec].taper, zm.data() + cd.refofs, cd.w0, cd.w0 + cd.wlen - 1, dt, IP_ZERO_ONE);
    st.comps_d.ensure(comps.size(), &c->dev_bytes);
    st.zmask_d.ensure(zm.size(), &c->dev_bytes);
    st.bt_d.ensure(sizeof(BandTab) / sizeof(int), &c->dev_bytes);
    st.vtab_d.ensure(st.vtab_h.size(), &c->dev_bytes);
    st.normtab_d.ensure(st.normtab_h.size(), &c->dev_bytes);
    HIPCHECK(hipMemcpyAsync(st.comps_d.p, comps.data(), comps.size() * sizeof(CompDev), hipMemcpyHostToDevice, c->stream));
    HIPCHECK(hipMemcpyAsync(st.zmask_d.p, zm.data(), zm.size() * sizeof(float), hipMemcpyHostToDevice, c->stream));
    HIPCHECK(hipMemcpyAsync(st.bt_d.p, &bt, sizeof(BandTab), hipMemcpyHostToDevice, c->stream));
    HIPCHECK(hipMemcpyAsync(st.vtab_d.p, st.vtab_h.data(), st.vtab_h.size() * sizeof(int2), hipMemcpyHostToDevice, c->stream));
    HIPCHECK(hipMemcpyAsync(st.normtab_d.p, st.normtab_h.data(), st.normtab_h.size() * sizeof(float), hipMemcpyHostToDevice, c->stream));
    HIPCHECK(hipStreamSynchronize(c->stream));      // host vectors go out of scope
}

// The reference probes of the (slot, length) pairs in `want` that no band has seen yet, for every band that needs the spectrum,
// through the in-LDS mode-1 kernels of the plain comparator (make_variants): |X| x filter for the spectral bands, the filtered
// trace for the filtered time-domain bands; norm factors on the host (probe_norm, comparator.f90:954-996).
static void make_variants(kiwi_hip_ctx *c, const std::vector<std::pair<int, int>> &want)
{
    BandState &st = c->band_state;
    const int nband = (int)c->bands.size(), nmis = c->nmis;
    const float dt = c->gm.dt;
    auto lg_of = [](int n) { int lg = 0; while ((1 << lg) < n) lg++; return lg; };
    struct Fresh { int b; FftPair pr; };
    std::vector<Fresh> fresh;
    long long fofs = 0;
    int longest = 0;
    for (auto &w : want) {
        const int m = w.first, ntr = w.second, nb = ntr / 2 + 1, lg = lg_of(ntr);
        for (int b = 0; b < nband; b++) {
            const BandDef &bd = c->bands[(size_t)b];
            if (!is_spectral(bd.method) && !bd.filter.defined()) continue;
            const size_t vi = ((size_t)b * nmis + m) * kLg + lg;
            if (st.vtab_h[vi].x >= 0) continue;
            const CompDev &cd = c->comps[(size_t)m];
            FftPair pr;
            pr.fft_ofs = fofs; pr.spec_ofs = 0; pr.ntrans = ntr; pr.slot = m;
            pr.specofs = (int)st.refamp_h.size(); pr.filtofs = (int)st.reffilt_h.size();
            st.refamp_h.resize(st.refamp_h.size() + nb, 0.f);
            st.filtw_h.resize(st.filtw_h.size() + nb, 1.f);
            st.reffilt_h.resize(st.reffilt_h.size() + cd.wlen, 0.f);
            if (bd.filter.defined()) {                       // filter weights per bin: abscissa j * df (comparator.f90:1224-1228)
                const float df = 1.f / ((float)ntr * dt);
                plf_taper_array(bd.filter, st.filtw_h.data() + pr.specofs, 0, nb - 1, df, IP_COS);
            }
            st.vtab_h[vi] = make_int2(pr.specofs, pr.filtofs);
            fresh.push_back(Fresh{ b, pr });
            fofs += ntr;
            longest = std::max(longest, ntr);
            fused_fft_table(c, ntr);
        }
    }
    if (fresh.empty()) return;
    // rows: the tapered reference over the window, zero padded
    std::vector<float> rows((size_t)fofs, 0.f);
    std::vector<FftPair> spec_prs, filt_prs;
    for (auto &f : fresh) {
        const CompDev &cd = c->comps[(size_t)f.pr.slot];
        std::memcpy(rows.data() + f.pr.fft_ofs, c->reft_h.data() + cd.refofs, (size_t)cd.wlen * sizeof(float));
        (is_spectral(c->bands[(size_t)f.b].method) ? spec_prs : filt_prs).push_back(f.pr);
    }
    st.rows_d.ensure(rows.size(), &c->dev_bytes);
    st.refamp_d.ensure(st.refamp_h.size(), &c->dev_bytes);
    st.filtw_d.ensure(st.filtw_h.size(), &c->dev_bytes);
    st.reffilt_d.ensure(st.reffilt_h.size(), &c->dev_bytes);
    st.prs_d.ensure(fresh.size(), &c->dev_bytes);
    std::vector<FftPair> prs(spec_prs);
    prs.insert(prs.end(), filt_prs.begin(), filt_prs.end());
    HIPCHECK(hipMemcpyAsync(st.rows_d.p, rows.data(), rows.size() * sizeof(float), hipMemcpyHostToDevice, c->stream));
    HIPCHECK(hipMemcpyAsync(st.prs_d.p, prs.data(), prs.size() * sizeof(FftPair), hipMemcpyHostToDevice, c->stream));
    HIPCHECK(hipMemcpyAsync(st.filtw_d.p, st.filtw_h.data(), st.filtw_h.size() * sizeof(float), hipMemcpyHostToDevice, c->stream));
    SpecParams sp{ KIWI_L2NORM, dt, c->syn_factor, nmis, 0, 1 };
    sp.lds_lo = 1 << kFusedFftMinLog2; sp.lds_hi = 1 << kFusedFftMaxLog2;
    const FusedFftTables tabs = fused_fft_tables(c);
    if (!spec_prs.empty())
        hipLaunchKernelGGL(spec_fft_norm_kernel<1>, dim3((unsigned)spec_prs.size()), dim3(256), (size_t)longest * 4, c->stream, st.rows_d.p, st.prs_d.p, tabs,
                           (const float *)nullptr, st.filtw_d.p, sp, (float *)nullptr, st.refamp_d.p, SynRows{});
    if (!filt_prs.empty())
        hipLaunchKernelGGL(spec_fft_filter_norm_kernel<1>, dim3((unsigned)filt_prs.size()), dim3(256), (size_t)longest * 4, c->stream, st.rows_d.p,
                           st.prs_d.p + spec_prs.size(), tabs, st.comps_d.p, st.filtw_d.p, (const float *)nullptr, st.zmask_d.p, sp, (float *)nullptr,
                           st.reffilt_d.p, SynRows{});
    HIPCHECK(hipGetLastError());
    // the fresh results down to the host mirrors, which are the master copy (the device arrays were re-allocated if they grew)
    for (auto &f : fresh) {
        const CompDev &cd = c->comps[(size_t)f.pr.slot];
        if (is_spectral(c->bands[(size_t)f.b].method))
            HIPCHECK(hipMemcpyAsync(st.refamp_h.data() + f.pr.specofs, st.refamp_d.p + f.pr.specofs, (size_t)(f.pr.ntrans / 2 + 1) * sizeof(float),
                                    hipMemcpyDeviceToHost, c->stream));
        else
            HIPCHECK(hipMemcpyAsync(st.reffilt_h.data() + f.pr.filtofs, st.reffilt_d.p + f.pr.filtofs, (size_t)cd.wlen * sizeof(float),
                                    hipMemcpyDeviceToHost, c->stream));
    }
    HIPCHECK(hipStreamSynchronize(c->stream));
    for (auto &f : fresh) {
        const CompDev &cd = c->comps[(size_t)f.pr.slot];
        const int method = c->bands[(size_t)f.b].method;
        double sum = 0.0, pk = 0.0;
        float nf;
        if (is_spectral(method)) {
            const int nb = f.pr.ntrans / 2 + 1;
            const float df = 1.f / ((float)f.pr.ntrans * dt);
            for (int k = 0; k < nb; k++) {
                const float v = st.refamp_h[(size_t)f.pr.specofs + k];
                sum += (method == KIWI_AMPSPEC_L2NORM) ? (double)v * (double)v : (double)std::fabs(v);
            }
            nf = (method == KIWI_AMPSPEC_L2NORM) ? 1.f * (float)std::sqrt((double)df * sum) : 1.f * (float)((double)df * sum);
        } else {
            for (int i = 0; i < cd.wlen; i++) {
                const float v = st.reffilt_h[(size_t)f.pr.filtofs + i];
                switch (method) {
                case KIWI_L2NORM: sum += (double)v * (double)v; break;
                case KIWI_L1NORM: sum += (double)std::fabs(v); break;
                case KIWI_SCALAR_PRODUCT: sum += (double)(v * v); break;
                default: pk = std::max(pk, (double)std::fabs(v)); break;
                }
            }
            switch (method) {
            case KIWI_L2NORM: nf = 1.f * (float)std::sqrt((double)dt * sum); break;
            case KIWI_L1NORM: nf = 1.f * (float)((double)dt * sum); break;
            case KIWI_SCALAR_PRODUCT: nf = (1.f * 1.f) * (float)sum; break;
            default: nf = 1.f * (float)pk; break;
            }
        }
        st.normtab_h[((size_t)f.b * nmis + f.pr.slot) * kLg + lg_of(f.pr.ntrans)] = nf;
    }
    HIPCHECK(hipMemcpyAsync(st.refamp_d.p, st.refamp_h.data(), st.refamp_h.size() * sizeof(float), hipMemcpyHostToDevice, c->stream));
    HIPCHECK(hipMemcpyAsync(st.reffilt_d.p, st.reffilt_h.data(), st.reffilt_h.size() * sizeof(float), hipMemcpyHostToDevice, c->stream));
    HIPCHECK(hipMemcpyAsync(st.vtab_d.p, st.vtab_h.data(), st.vtab_h.size() * sizeof(int2), hipMemcpyHostToDevice, c->stream));
    HIPCHECK(hipMemcpyAsync(st.normtab_d.p, st.normtab_h.data(), st.normtab_h.size() * sizeof(float), hipMemcpyHostToDevice, c->stream));
    HIPCHECK(hipStreamSynchronize(c->stream));
}

// the sources [isrc0, isrc0 + nsrc) of the uploaded batch; adds its HIP-event times to c->bands_ms
static void run(kiwi_hip_ctx *c, int isrc0, int nsrc, const Out &out)
{
    check_setup(c);
    check_group_range("band_misfits", c, isrc0, nsrc, 1);
    if (nsrc == 0) return;
    BandState &st = c->band_state;
    if (!st.valid || st.prepare_gen != c->prepare_gen) reset_cache(c);
    const int nrec = (int)c->recv.size(), nband = (int)c->bands.size(), nmis = c->nmis;
    if (st.need_spec && !c->fused_fft)
        throw std::runtime_error("band_misfits: bands with a frequency filter or an amplitude-spectrum method go through the in-LDS transforms, "
                                 "which KIWI_HIP_FUSED_FFT=0 switches off");
    int wlen_pow2 = 1 << kFusedFftMinLog2;
    while (wlen_pow2 < c->max_wlen) wlen_pow2 <<= 1;
    if (wlen_pow2 > (1 << kFusedFftMaxLog2))
        throw std::runtime_error("band_misfits: a misfit window of " + std::to_string(c->max_wlen) + " samples does not fit the in-LDS row of " +
                                 std::to_string(1 << kFusedFftMaxLog2) + " samples");
    c->misfit_d.ensure((size_t)c->nsrc * c->nmis, &c->dev_bytes);
    c->global_d.ensure((size_t)c->nsrc, &c->dev_bytes);
    if (c->fft_needed && !c->fft_ready) prepare_fft(c, c->reft_h);
    c->fuse_now = false;                                   // the plain synthetics go to memory
    // the sources' own strip spans are kept: the transform lengths follow them (fft_size_kernel), and every source is synthesised
    // (run_chunk shares no synthetics between sources then)
    struct Restore { kiwi_hip_ctx *c; bool want; ~Restore() { c->want_spansrc = want; } } restore{ c, c->want_spansrc };
    c->want_spansrc = true;
    if (!st.attr) {
        HIPCHECK(hipFuncSetAttribute(reinterpret_cast<const void *>(&band_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, kMaxDynLds));
        st.attr = true;
    }

    const PooledEvents<4> ev(c);
    std::vector<int> ntr_h;
    int s = isrc0;
    while (s < isrc0 + nsrc) {
        // a chunk of sources (groups of one) with their misfits and norms per band
        const int n = next_group_chunk(c, isrc0, s - isrc0, nsrc, 1, 1, (size_t)nband * nmis * 2 * sizeof(float),
                                       c->fft_needed ? c->fft_cap : kNoSourceCap);
        HIPCHECK(hipEventRecord(ev[0], c->stream));
        run_chunk(c, s, n, 0);
        HIPCHECK(hipEventRecord(ev[1], c->stream));
        const size_t np = (size_t)n * nmis;
        int longest = wlen_pow2;
        if (st.need_spec) {
            st.ntr_d.ensure(np, &c->dev_bytes);
            hipLaunchKernelGGL(fft_size_kernel, dim3((unsigned)((np + 255) / 256)), dim3(256), 0, c->stream, c->spansrc_d.p, c->comps_d.p, nmis, n, nrec,
                               c->risetime_d.p + s, c->gm.dt, st.ntr_d.p, (const int *)nullptr);
            ntr_h.resize(np);
            HIPCHECK(hipMemcpyAsync(ntr_h.data(), st.ntr_d.p, np * sizeof(int), hipMemcpyDeviceToHost, c->stream));
            HIPCHECK(hipStreamSynchronize(c->stream));
            std::vector<std::pair<int, int>> want;
            std::vector<int> seen((size_t)nmis, 0);
            longest = 0;
            for (size_t i = 0; i < np; i++) {
                const int m = (int)(i % (size_t)nmis), nt = ntr_h[i];
                if (nt < (1 << kFusedFftMinLog2) || nt > (1 << kFusedFftMaxLog2))
                    throw std::runtime_error("band_misfits: source " + std::to_string(s + (int)(i / (size_t)nmis) + 1) + ", misfit slot " + std::to_string(m + 1) +
                                             " needs a transform of " + std::to_string(nt) + " samples; the in-LDS transforms take " +
                                             std::to_string(1 << kFusedFftMinLog2) + " to " + std::to_string(1 << kFusedFftMaxLog2));
                longest = std::max(longest, nt);
                if (seen[(size_t)m] != nt) { seen[(size_t)m] = nt; want.emplace_back(m, nt); }
            }
            std::sort(want.begin(), want.end());
            want.erase(std::unique(want.begin(), want.end()), want.end());
            make_variants(c, want);
        }
        const size_t nout = (size_t)n * nband * nmis;
        st.mis_d.ensure(nout, &c->dev_bytes); st.norm_d.ensure(nout, &c->dev_bytes); st.glob_d.ensure((size_t)n * nband, &c->dev_bytes);
        // dynamic LDS: the longest row, twice where a copy of the spectrum serves two or more filtered bands and fits
        const int dyn = st.nfilt >= 2 ? std::max(4 * longest, std::min(8 * longest, kMaxDynLds)) : 4 * longest;
        BandArgs a;
        a.sr = SynRows{ c->syn_d.p, c->syn_stride, c->comps_d.p, c->tw_d.p, c->moment_d.p, c->risetime_d.p, nullptr };
        a.reft = c->reft_d.p;
        a.ntr = st.need_spec ? st.ntr_d.p : nullptr;
        a.tabs = fused_fft_tables(c);
        a.bt = reinterpret_cast<const BandTab *>(st.bt_d.p);
        a.vtab = st.vtab_d.p; a.normtab = st.normtab_d.p;
        a.refamp = st.refamp_d.p; a.filtw = st.filtw_d.p; a.reffilt = st.reffilt_d.p; a.zmask = st.zmask_d.p;
        a.nband = nband; a.nmis = nmis; a.isrc0 = s; a.dyn_bytes = dyn;
        a.dt = c->gm.dt; a.syn_factor = c->syn_factor;
        a.mis_out = st.mis_d.p; a.norm_out = st.norm_d.p;
        hipLaunchKernelGGL(band_kernel, dim3((unsigned)n, (unsigned)nmis), dim3(256), (size_t)dyn, c->stream, a);
        hipLaunchKernelGGL(band_global_kernel, dim3((unsigned)(((size_t)n * nband + 127) / 128)), dim3(128), 0, c->stream, st.mis_d.p, st.norm_d.p,
                           c->recfirst_d.p, c->nrec_en, nmis, nband, s, n, st.glob_d.p, c->any_failed ? c->status_d.p : (const int *)nullptr);
        HIPCHECK(hipGetLastError());
        HIPCHECK(hipEventRecord(ev[2], c->stream));
        const Out o = out.at((size_t)(s - isrc0), (size_t)nband, (size_t)nmis);
        if (o.misfit) HIPCHECK(hipMemcpyAsync(o.misfit, st.mis_d.p, nout * sizeof(float), hipMemcpyDeviceToHost, c->stream));
        if (o.norm) HIPCHECK(hipMemcpyAsync(o.norm, st.norm_d.p, nout * sizeof(float), hipMemcpyDeviceToHost, c->stream));
        if (o.global) HIPCHECK(hipMemcpyAsync(o.global, st.glob_d.p, (size_t)n * nband * sizeof(float), hipMemcpyDeviceToHost, c->stream));
        HIPCHECK(hipEventRecord(ev[3], c->stream));
        HIPCHECK(hipStreamSynchronize(c->stream));
        for (int i = 0; i < 3; i++) ev.add_elapsed(c->bands_ms, i, i, i + 1);
        s += n;
    }
    leave_evaluated(c, isrc0, nsrc, 0);                    // the context's own method and filters were evaluated on the way
}

// kiwi_hip_band_misfits_for_params piece by piece (PieceCall, kiwi_group_run.hpp): plain sources
static PieceCall piece_call(const Out &out)
{
    return PieceCall{ 1,
        [](kiwi_hip_ctx *c) { check_setup(c); },
        [=](kiwi_hip_ctx *c, int s0, int n) { fill_failed((size_t)n, c->bands.size(), (size_t)c->nmis, out.at((size_t)s0, c->bands.size(), (size_t)c->nmis)); },
        [=](kiwi_hip_ctx *c, int s0, int n) { run(c, 0, n, out.at((size_t)s0, c->bands.size(), (size_t)c->nmis)); } };
}

} // namespace bands
