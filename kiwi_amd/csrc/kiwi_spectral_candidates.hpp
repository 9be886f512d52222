// kiwi_spectral_candidates.hpp -- misfits of many GIVEN coefficient vectors per group under the amplitude-spectrum norms
// (ampspec_l2norm, ampspec_l1norm).  The amplitude spectrum is not quadratic in the coefficients, but the complex spectrum is
// linear in them: a candidate x at a location is X(f) = sum_a x_a S_a(f) with S_a the spectra of the K basis sources' kept traces,
// so the K transforms are paid once per location and a candidate costs K complex multiply-adds and a root per kept bin.  Included
// by kiwi_hip.hip behind the other candidate headers, under the same -ffp-contract=off: every fp32 and fp64 operation below is
// rounded on its own, and tests/spectral_candidates_restatement.py restates each in the same order (the GPU tests ask for bit
// identity of the candidate kernels with that restatement fed with the device's own spectra).
//
// Sources [isrc0, isrc0 + ngroup K) are ngroup groups of K <= 8 consecutive basis sources, as for kiwi_hip_linear_fit.  Per chunk
// of whole groups:
//   evaluate    run_chunk with the tapered, folded, moment-scaled rows kept in proc_d (keep 2): misfits, norm factors and global
//               misfits of the basis sources are left exactly as kiwi_hip_eval leaves them
//   spectra     speccand_spectra_kernel, one workgroup of 256 per (basis source, slot): the kept row of wlen samples, zero-padded
//               to the pair's transform length, through fused_fft_forward and the unpacking X[k] = E + w O, X[M-k] = conj(E - w O)
//               of spec_fft_norm_kernel, operation for operation; the bins klo .. khi of the slot go, as float2, to
//               spec[(group, slot)][k - klo][a], basis index innermost.  No filter weight and no syn_factor here.  klo .. khi is
//               the smallest range that holds every bin with a non-zero filter weight (host, from filtw_h; 0 .. ntrans / 2 without a
//               filter).  A skipped bin adds exactly nothing: its reference amplitude is |Xref| x 0 -- checked on the host when
//               the table is made, a non-zero one is refused.
//   candidates  speccand_kernel<K, FREE>, one workgroup of kThreads lanes per (group, tile of kThreads candidates); a lane owns ONE
//               candidate with xf = (float) x in registers.  Slots ascend; per slot kStage bins of spec, refamp and filtw at a time
//               are staged in LDS and read as broadcasts, bins ascending from klo to khi into ONE fp64 accumulator per lane:
//                   re = xf_0 S_0.re; re = re + xf_a S_a.re (a ascending); im the same;  b = amp_rn(re, im)  (amp2f's power-of-two
//                   scaling with a correctly rounded root);  b = b fw[k] where the receiver has a filter;
//                   d = unit ? a - b : 1.f a - syn_factor b  (a = refamp[k]);  acc = sq_acc(acc, d)  |  acc += (double) fabsf(d)
//               slot misfit m = (float) sqrt((double) df acc) | (float) ((double) df acc), df = 1.f / ((float) ntrans dt); slot norm
//               factor n = normsrc of the group's FIRST source (under a taper the same for all of them).
//               Outer fold, the expression sequence of outer_prepare_kernel and outer_draw_kernel (kiwi_outer.hpp) for ONE draw
//               of weights 1, per SLOT as make_global_misfits has it: per receiver r (ascending) M, N = sums (l2norm: roots of sums
//               of squares) of its slots' m, n in fp64; rw = w_r, anarchy: q = rw / (N != 0 ? N : -1), rw = q > 0 or NaN ? q : 0;
//               av = M rw, bv = N rw (squared under l2norm); ms = ms + av 1.0; ns = ns + bv 1.0;  misfit = ms / ns (root under
//               l2norm) where ns > 0, else NaN; a negative or NaN quotient is NaN.
//     FREE      (method 3, outer l2norm) the candidate is a direction.  Per slot P = P + a bs, Q = Q + bs bs, A = A + a a in fp64
//               (bs = unit ? b : syn_factor b; the products of fp32 values are exact in fp64).  Per receiver: N and rw as above,
//               W = rw rw;  p = p + (double) df P, q and a the same over its slots;  SP = SP + W p, SQ, SA the same;
//               SD = SD + (N rw)(N rw).  s = SP / SQ (NaN unless SQ > 0);  misfit = sqrt(max((SA - 2 s SP) + (s s) SQ, 0) / SD)
//               (NaN unless SD > 0).  scale[g][c] = s.
//               A tile's best (NaN passed over, then value, then lowest index) goes to a slab.
//   fold        speccand_fold_kernel, one wavefront per group: the tiles' bests in the same order.  No atomics.
// Status of a group: 0 evaluated; 1 no receiver counts (the denominator of the fold is not positive): NaN, best_index -1; 2 a basis
// source failed to discretise (set on the host).

namespace spectral_candidates {

constexpr int kThreads = 256;                   // candidates per workgroup
constexpr int kStage = 128;                     // bins per LDS stage: 128 x (8 K + 8) bytes = 9 KiB at K = 8
constexpr int kMaxBasis = linfit::kMaxBasis;

struct SlotRec {                                // per (group of the chunk, slot)
    long long sofs;                             // bins in front of this row in spec (a bin is K float2)
    int ntrans;                                 // 0: the group is not evaluated (a basis source failed to discretise)
    int klo, khi;                               // kept bins (khi < klo: none)
    int specofs;                                // refamp / filtw of (slot, ntrans)
    float df, norm;                             // 1.f / ((float) ntrans dt); norm factor of the group's first source
};
static_assert(sizeof(SlotRec) == 32, "SlotRec layout");
struct SlotInfo { int rec, last, has_filter, pad; };     // per slot: its receiver, whether it is the receiver's last slot

// |x + i y| as amp2f scales it, with a correctly rounded root (the argument of the root lies in [1/4, 2)): numpy restates its bits
__device__ __forceinline__ float amp_rn(float x, float y)
{
    const float m = fmaxf(fabsf(x), fabsf(y));
    if (!(m > 0.f) || m > 3.0e38f) return m != m ? m : fabsf(x) + fabsf(y);     // 0, inf, nan
    const int e = __builtin_amdgcn_frexp_expf(m);
    const float sx = ldexpf(x, -e), sy = ldexpf(y, -e);
    return ldexpf(sqrtf(sx * sx + sy * sy), e);          // (sqrtf is correctly rounded: the unit is compiled without fast-math)
}

// blockIdx.x = slot, blockIdx.y = basis source of the chunk.  proc: the kept rows (run_chunk, keep 2)
__global__ __launch_bounds__(256) void speccand_spectra_kernel(const float *__restrict__ proc, size_t syn_stride,
                                                               const CompDev *__restrict__ comps, const SlotRec *__restrict__ slots,
                                                               FusedFftTables tabs, int nmis, int K, float2 *__restrict__ spec)
{
    extern __shared__ __attribute__((aligned(16))) float2 zf[];
    const int tid = (int)threadIdx.x, m = (int)blockIdx.x, s = (int)blockIdx.y;
    const int g = s / K, a = s - g * K;
    const SlotRec sl = slots[(size_t)g * nmis + m];
    if (sl.ntrans == 0 || sl.khi < sl.klo) return;       // (workgroup-uniform)
    const CompDev cd = comps[m];
    const int N = sl.ntrans, M = N >> 1;
    const float2 *__restrict__ tw = tabs.tab[31 - __clz(N)];
    const float *__restrict__ row = proc + (size_t)s * syn_stride + cd.synofs + cd.halo;
#pragma unroll 4
    for (int n = tid; n < M; n += 256) {
        const int i = 2 * n;
        float2 x = make_float2(0.f, 0.f);
        if (i < cd.wlen) x.x = row[i];
        if (i + 1 < cd.wlen) x.y = row[i + 1];
        zf[fused_fft_lds(n)] = x;
    }
    __syncthreads();
    tw = fused_fft_forward(zf, tw, M, tid);
    const int lgM = 31 - __clz(M);
    float2 *__restrict__ out = spec + (size_t)sl.sofs * K + a;
    auto bin = [&](int k, float re, float im) {
        if (k >= sl.klo && k <= sl.khi) out[(size_t)(k - sl.klo) * K] = make_float2(re, im);
    };
    // (as spec_fft_norm_kernel: bins k and M - k come from the same two points)
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
}

// spec: the chunk's rows; slots: [group][nmis]; info: [nmis]; w: [nrec] (0 for a disabled receiver); x: [ncand][K] fp32.
// misfit, scale: [group][ncand] or null; smis: [group][ncand][nmis] or null; tile_v, tile_i: [group][gridDim.x]; status: [group].
// blockIdx.x = tile of candidates, blockIdx.y = group
template <int K, bool FREE>
__global__ __launch_bounds__(kThreads) void speccand_kernel(const float2 *__restrict__ spec, const SlotRec *__restrict__ slots,
                                                            const SlotInfo *__restrict__ info, const float *__restrict__ refamp,
                                                            const float *__restrict__ filtw, const double *__restrict__ w, int nmis,
                                                            int method, int l2, int anarchy, float syn_factor,
                                                            const float *__restrict__ x, int ncand, double *__restrict__ misfit,
                                                            double *__restrict__ scale, float *__restrict__ smis,
                                                            double *__restrict__ tile_v, int *__restrict__ tile_i,
                                                            int *__restrict__ status)
{
    __shared__ float2 sS[kStage * K];
    __shared__ float sA[kStage], sF[kStage];
    __shared__ double best_v[kThreads / 64];
    __shared__ int best_i[kThreads / 64];
    const int g = (int)blockIdx.y, tid = (int)threadIdx.x;
    const int cand = (int)blockIdx.x * kThreads + tid;
    const bool live = cand < ncand;
    const size_t cslot = (size_t)g * ncand + (live ? cand : 0);
    const double nan = __longlong_as_double(0x7ff8000000000000LL);
    const bool unit = (syn_factor == 1.f);
    float xf[K];
#pragma unroll
    for (int a = 0; a < K; a++) xf[a] = live ? x[(size_t)cand * K + a] : 0.f;
    double ms = 0.0, ns = 0.0;                  // the fold's sums over the receivers (FREE: ns is SD)
    double SP = 0.0, SQ = 0.0, SA = 0.0;        // FREE
    double Mr = 0.0, Nr = 0.0;                  // the receiver being folded
    double pr = 0.0, qr = 0.0, ar = 0.0;        // FREE
    const bool evaluated = nmis > 0 && slots[(size_t)g * nmis].ntrans != 0;
    for (int m = 0; evaluated && m < nmis; m++) {
        const SlotRec sl = slots[(size_t)g * nmis + m];
        const SlotInfo si = info[m];
        const int nb = sl.khi - sl.klo + 1;
        double acc = 0.0, P = 0.0, Q = 0.0, A = 0.0;
        for (int k0 = 0; k0 < nb; k0 += kStage) {
            const int nst = nb - k0 < kStage ? nb - k0 : kStage;
            __syncthreads();
            const float2 *__restrict__ src = spec + ((size_t)sl.sofs + k0) * K;
            for (int p = tid; p < nst * K; p += kThreads) sS[p] = src[p];
            if (tid < nst) {
                sA[tid] = refamp[sl.specofs + sl.klo + k0 + tid];
                sF[tid] = filtw[sl.specofs + sl.klo + k0 + tid];
            }
            __syncthreads();
            for (int j = 0; j < nst; j++) {
                const float2 *sv = sS + j * K;
                float re = xf[0] * sv[0].x, im = xf[0] * sv[0].y;
#pragma unroll
                for (int a = 1; a < K; a++) { re = re + xf[a] * sv[a].x; im = im + xf[a] * sv[a].y; }
                float b = amp_rn(re, im);
                if (si.has_filter) b = b * sF[j];
                const float av = sA[j];
                if (FREE) {
                    const double bs = (double)(unit ? b : syn_factor * b), ad = (double)av;
                    P = P + ad * bs;
                    Q = Q + bs * bs;
                    A = A + ad * ad;
                } else {
                    const float d = unit ? (av - b) : (1.f * av - syn_factor * b);
                    if (method == 3) acc = sq_acc(acc, d);
                    else acc += (double)fabsf(d);
                }
            }
        }
        const double nv = (double)sl.norm;
        if (FREE) {
            pr = pr + (double)sl.df * P; qr = qr + (double)sl.df * Q; ar = ar + (double)sl.df * A;
            Nr = Nr + nv * nv;
        } else {
            const float mf = method == 3 ? (float)sqrt((double)sl.df * acc) : (float)((double)sl.df * acc);
            if (smis && live) smis[cslot * nmis + m] = mf;
            const double mv = (double)mf;
            if (l2) { Mr = Mr + mv * mv; Nr = Nr + nv * nv; }
            else { Mr = Mr + mv; Nr = Nr + nv; }
        }
        if (!si.last) continue;
        if (l2) { Mr = sqrt(Mr); Nr = sqrt(Nr); }
        double rw = w[si.rec];
        if (anarchy) {
            const double q = rw / (Nr != 0.0 ? Nr : -1.0);
            rw = (q > 0.0 || q != q) ? q : 0.0;
        }
        double bv = Nr * rw;
        if (FREE) {
            const double W = rw * rw;
            SP = SP + W * pr; SQ = SQ + W * qr; SA = SA + W * ar;
            ns = ns + bv * bv;
        } else {
            double av = Mr * rw;
            if (l2) { av = av * av; bv = bv * bv; }
            ms = ms + av * 1.0;
            ns = ns + bv * 1.0;
        }
        Mr = 0.0; Nr = 0.0; pr = 0.0; qr = 0.0; ar = 0.0;
    }
    double mf = nan, sc = nan;
    if (evaluated) {
        if (FREE) {
            if (SQ > 0.0) sc = SP / SQ;
            if (ns > 0.0) {
                double val = (SA - 2.0 * sc * SP) + (sc * sc) * SQ;
                val = val > 0.0 ? val : (val == val ? 0.0 : val);
                mf = sqrt(val / ns);
            }
        } else if (ns > 0.0) {
            mf = ms / ns;
            if (l2) mf = sqrt(mf);
            if (!(mf >= 0.0)) mf = nan;
        }
    }
    if (live) {
        if (misfit) misfit[cslot] = mf;
        if (scale) scale[cslot] = sc;
    }
    if (blockIdx.x == 0 && tid == 0) status[g] = (evaluated && ns > 0.0) ? 0 : 1;
    double bv = mf;
    int bi = (live && mf == mf) ? cand : -1;
    linfit::wave_best(bv, bi);
    if ((tid & 63) == 0) { best_v[tid >> 6] = bv; best_i[tid >> 6] = bi; }
    __syncthreads();
    if (tid == 0) {
        for (int k = 1; k < kThreads / 64; k++) linfit::take_better(bv, bi, best_v[k], best_i[k]);
        tile_v[(size_t)g * gridDim.x + blockIdx.x] = bv;
        tile_i[(size_t)g * gridDim.x + blockIdx.x] = bi;
    }
}

// blockIdx.x = group
__global__ __launch_bounds__(64) void speccand_fold_kernel(const double *__restrict__ tile_v, const int *__restrict__ tile_i, int ntile,
                                                           int *__restrict__ best_index, double *__restrict__ best_misfit)
{
    const int g = (int)blockIdx.x, lane = (int)threadIdx.x;
    double bv = 0.0;
    int bi = -1;
    for (int t = lane; t < ntile; t += 64) linfit::take_better(bv, bi, tile_v[(size_t)g * ntile + t], tile_i[(size_t)g * ntile + t]);
    linfit::wave_best(bv, bi);
    if (lane == 0) {
        best_index[g] = bi;
        best_misfit[g] = bi >= 0 ? bv : __longlong_as_double(0x7ff8000000000000LL);
    }
}

// host arrays of the caller for the groups of ONE call of run().  x [ncand][K], shared by all groups.  best_index, best_misfit,
// status [group]; the others may be null: misfit, scale [group][ncand]; slot_misfit [group][ncand][nmis], slot_norm [group][nmis];
// spectra [group][nmis][spectra_bins][K] float2 (the kept bins of a slot from index 0), spectra_range [group][nmis][3] (klo, khi,
// ntrans), spectra_ref [group][nmis][spectra_bins][2] (refamp, filtw of the kept bins)
struct Call {
    const double *x; int ncand, outer_norm, free_scale;
    int *best_index; double *best_misfit; int *status;
    double *misfit, *scale;
    float *slot_misfit, *slot_norm;
    int spectra_bins; float *spectra; int *spectra_range; float *spectra_ref;
    Call at(int g, int nmis, int K) const
    {
        Call c = *this;
        c.best_index += g; c.best_misfit += g; c.status += g;
        if (misfit) c.misfit += (size_t)g * ncand;
        if (scale) c.scale += (size_t)g * ncand;
        if (slot_misfit) c.slot_misfit += (size_t)g * ncand * nmis;
        if (slot_norm) c.slot_norm += (size_t)g * nmis;
        if (spectra) c.spectra += (size_t)g * nmis * spectra_bins * K * 2;
        if (spectra_range) c.spectra_range += (size_t)g * nmis * 3;
        if (spectra_ref) c.spectra_ref += (size_t)g * nmis * spectra_bins * 2;
        return c;
    }
};

// what the call cannot do is refused before anything runs, nothing approximated.  Leaves the context prepared
static void check_setup(kiwi_hip_ctx *c, int K, const Call &cl)
{
    if (K < 1 || K > kMaxBasis)
        throw std::runtime_error("spectral_candidates: K = " + std::to_string(K) + " basis sources per group; 1 to " + std::to_string(kMaxBasis) + " are supported");
    if (cl.ncand < 1) throw std::runtime_error("spectral_candidates: ncand = " + std::to_string(cl.ncand) + "; at least one candidate is needed");
    if (!cl.x || !cl.best_index || !cl.best_misfit || !cl.status)
        throw std::runtime_error("spectral_candidates: null candidates, best_index, best_misfit or status array");
    if (c->method != KIWI_AMPSPEC_L2NORM && c->method != KIWI_AMPSPEC_L1NORM)
        throw std::runtime_error("spectral_candidates: the misfit method must be ampspec_l2norm or ampspec_l1norm (the quadratic norms go through linear_fit_candidates)");
    if (cl.outer_norm != 1 && cl.outer_norm != 2) throw std::runtime_error("spectral_candidates: outer_norm must be 1 (l1norm) or 2 (l2norm)");
    if (cl.free_scale != 0 && cl.free_scale != 1)
        throw std::runtime_error("spectral_candidates: free_scale = " + std::to_string(cl.free_scale) + " must be 0 or 1");
    if (cl.free_scale && (c->method != KIWI_AMPSPEC_L2NORM || cl.outer_norm != 2))
        throw std::runtime_error("spectral_candidates: free_scale needs ampspec_l2norm and the outer l2norm (elsewhere the best scale of a direction has no closed form)");
    if (cl.free_scale && (cl.slot_misfit || cl.slot_norm))
        throw std::runtime_error("spectral_candidates: free_scale together with slot_misfit is refused (the scale belongs to the whole fold, not to a slot)");
    if (cl.scale && !cl.free_scale) throw std::runtime_error("spectral_candidates: a scale array without free_scale");
    if ((cl.slot_misfit == nullptr) != (cl.slot_norm == nullptr)) throw std::runtime_error("spectral_candidates: slot_misfit and slot_norm come together");
    if ((cl.spectra || cl.spectra_ref) && (!cl.spectra_range || cl.spectra_bins < 1))
        throw std::runtime_error("spectral_candidates: spectra need spectra_range and spectra_bins (kiwi_hip_spectral_candidates_shape)");
    for (size_t p = 0; p < (size_t)cl.ncand * K; p++)
        if (!std::isfinite(cl.x[p]))
            throw std::runtime_error("spectral_candidates: entry " + std::to_string(p % K) + " of candidate " + std::to_string(p / K) + " is not finite");
    if (!c->fused_fft) throw std::runtime_error("spectral_candidates: KIWI_HIP_FUSED_FFT=0 leaves no in-LDS transform to take the spectra from");
    prepare(c);
    if (c->synth_only) throw std::runtime_error("spectral_candidates: every enabled receiver component needs a reference seismogram");
    if (c->any_untapered)
        throw std::runtime_error("spectral_candidates: an enabled receiver has no misfit taper (its transform follows the source, so the basis traces have no common spectrum)");
}

// bins per (group, slot) of the spectra arrays in this context: the longest transform any slot can need
static int spectra_bins(kiwi_hip_ctx *c)
{
    prepare(c);
    if (c->fft_needed && !c->fft_ready) prepare_fft(c, c->reft_h);
    int nb = 1;
    for (const CompDev &cd : c->comps) nb = std::max(nb, cd.ntrans_max / 2 + 1);
    return nb;
}

static void fill_failed(int ngroup, int nmis, int K, const Call &cl)
{
    const double nan = std::numeric_limits<double>::quiet_NaN();
    for (int g = 0; g < ngroup; g++) { cl.status[g] = 2; cl.best_index[g] = -1; cl.best_misfit[g] = nan; }
    const size_t nc = (size_t)ngroup * cl.ncand;
    if (cl.misfit) std::fill(cl.misfit, cl.misfit + nc, nan);
    if (cl.scale) std::fill(cl.scale, cl.scale + nc, nan);
    if (cl.slot_misfit) std::fill(cl.slot_misfit, cl.slot_misfit + nc * nmis, 0.f);
    if (cl.slot_norm) std::fill(cl.slot_norm, cl.slot_norm + (size_t)ngroup * nmis, 0.f);
    if (cl.spectra) std::fill(cl.spectra, cl.spectra + (size_t)ngroup * nmis * cl.spectra_bins * K * 2, 0.f);
    if (cl.spectra_ref) std::fill(cl.spectra_ref, cl.spectra_ref + (size_t)ngroup * nmis * cl.spectra_bins * 2, 0.f);
    if (cl.spectra_range)
        for (size_t i = 0; i < (size_t)ngroup * nmis; i++) { cl.spectra_range[3 * i] = 0; cl.spectra_range[3 * i + 1] = -1; cl.spectra_range[3 * i + 2] = 0; }
}

struct Args {
    const float2 *spec; const SlotRec *slots; const SlotInfo *info; const double *w; const float *x;
    int ng, method, l2, anarchy, ncand;
    double *misfit, *scale; float *smis; double *tile_v; int *tile_i; int *status;
};

template <int K>
static void launch(kiwi_hip_ctx *c, const Args &a, bool free_scale)
{
    const int ntile = (a.ncand + kThreads - 1) / kThreads;
    const dim3 grid((unsigned)ntile, (unsigned)a.ng);
    if (free_scale)
        hipLaunchKernelGGL((speccand_kernel<K, true>), grid, dim3(kThreads), 0, c->stream, a.spec, a.slots, a.info, c->refamp_d.p, c->filtw_d.p, a.w,
                           c->nmis, a.method, a.l2, a.anarchy, c->syn_factor, a.x, a.ncand, a.misfit, a.scale, a.smis, a.tile_v, a.tile_i, a.status);
    else
        hipLaunchKernelGGL((speccand_kernel<K, false>), grid, dim3(kThreads), 0, c->stream, a.spec, a.slots, a.info, c->refamp_d.p, c->filtw_d.p, a.w,
                           c->nmis, a.method, a.l2, a.anarchy, c->syn_factor, a.x, a.ncand, a.misfit, a.scale, a.smis, a.tile_v, a.tile_i, a.status);
    HIPCHECK(hipGetLastError());
}

static void launch_any(kiwi_hip_ctx *c, int K, const Args &a, bool free_scale)
{
    by_basis(K, [&](auto k) { launch<k.value>(c, a, free_scale); });
}

// what a call built on this one (kiwi_spectral_candidates_bootstrap.hpp) puts in the place of the candidate and fold kernels of every
// chunk: its device bytes per group; its own candidate kernel on the chunk's spectra, slot table [group][nmis], slot info and fp32
// candidates; and behind it its kernels on what that one wrote, which also write status [group] (0 or 1).  sl: the host's copy of
// the slot table.  With a hook speccand_kernel and speccand_fold_kernel are not launched, best_index and best_misfit stay as the
// caller made them, and the third time of c->speccand_ms is the hook's candidate kernel; the time of its other kernels goes to ms[0]
struct ChunkHook {
    size_t per_group = 0;
    float *ms = nullptr;
    virtual void candidates(int ng, const float2 *spec, const SlotRec *slots, const SlotInfo *info, const float *x) = 0;
    virtual void after_candidates(int g0, int ng, const std::vector<SlotRec> &sl, int *status) = 0;
    virtual ~ChunkHook() = default;
};

// the groups [isrc0, isrc0 + ngroup K) of the uploaded batch; adds its HIP-event times to c->speccand_ms: evaluation (run_chunk),
// the spectra kernel alone, the candidate and fold kernels, the downloads
static void run(kiwi_hip_ctx *c, int isrc0, int ngroup, int K, const double *receiver_weight, int anarchy, const Call &cl,
                ChunkHook *hook = nullptr)
{
    check_setup(c, K, cl);
    check_group_range("spectral_candidates", c, isrc0, ngroup, K);
    if (ngroup == 0) return;
    const int nrec = (int)c->recv.size(), nmis = c->nmis;
    c->misfit_d.ensure((size_t)c->nsrc * c->nmis, &c->dev_bytes);
    c->global_d.ensure((size_t)c->nsrc, &c->dev_bytes);
    if (c->fft_needed && !c->fft_ready) prepare_fft(c, c->reft_h);
    const int proc_which = 2;
    c->fuse_now = can_fuse(c, proc_which, isrc0, ngroup * K);
    if (c->fft_cap < K) throw std::runtime_error("spectral_candidates: the transform workspace (KIWI_HIP_CHUNK_MB) does not hold one group");

    const std::vector<double> w = receiver_weights(c, receiver_weight);
    std::vector<SlotInfo> info((size_t)nmis);
    for (int m = 0; m < nmis; m++)
        info[(size_t)m] = SlotInfo{ c->comps[(size_t)m].rec, (m + 1 == nmis || c->comps[(size_t)m + 1].rec != c->comps[(size_t)m].rec) ? 1 : 0,
                                    c->comps[(size_t)m].has_filter, 0 };
    std::vector<float> xf((size_t)cl.ncand * K);
    for (size_t p = 0; p < xf.size(); p++) xf[p] = (float)cl.x[p];
    const size_t ntile = (size_t)(cl.ncand + kThreads - 1) / kThreads;
    // device buffers of the call: kept on the context and grown only, like the evaluation's workspaces (no allocation, and so no
    // device-wide wait, in a call whose sizes the context has seen)
    auto &B = c->speccand_bufs;
    DevBuf<double> &w_d = B.w, &mis_d = B.misfit, &sc_d = B.scale, &tile_v = B.tile_v, &bestv_d = B.best_misfit;
    DevBuf<float> &x_d = B.x, &smis_d = B.smis;
    DevBuf<float2> &spec_d = B.spec;
    DevBuf<int> &tile_i = B.tile_i, &besti_d = B.best_index, &st_d = B.status, &slots_d = B.slots, &info_d = B.info;
    constexpr size_t kRecInts = sizeof(SlotRec) / sizeof(int), kInfoInts = sizeof(SlotInfo) / sizeof(int);
    w_d.ensure((size_t)std::max(nrec, 1), &c->dev_bytes);
    x_d.ensure(xf.size(), &c->dev_bytes);
    info_d.ensure((size_t)std::max(nmis, 1) * kInfoInts, &c->dev_bytes);
    // (w, info and xf are read by these copies: nothing leaves this function, by return or by exception, before the stream is drained)
    struct Drain { hipStream_t s; ~Drain() { (void)hipStreamSynchronize(s); } } drain{ c->stream };
    HIPCHECK(hipMemcpyAsync(w_d.p, w.data(), (size_t)nrec * sizeof(double), hipMemcpyHostToDevice, c->stream));
    HIPCHECK(hipMemcpyAsync(x_d.p, xf.data(), xf.size() * sizeof(float), hipMemcpyHostToDevice, c->stream));
    if (nmis > 0) HIPCHECK(hipMemcpyAsync(info_d.p, info.data(), (size_t)nmis * sizeof(SlotInfo), hipMemcpyHostToDevice, c->stream));
    if (!c->speccand_attr) {          // more than 64 KB of dynamic LDS per workgroup has to be asked for
        HIPCHECK(hipFuncSetAttribute(reinterpret_cast<const void *>(&speccand_spectra_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, 4 << kFusedFftMaxLog2));
        c->speccand_attr = true;
    }

    const PooledEvents<7> ev(c);                           // (ev[5]: immediately in front of the spectra kernel; ev[6]: behind the hook)
    // the kept bins of (slot, variant): from the host mirror of the filter weights, made once per variant and call
    std::map<std::pair<int, int>, std::pair<int, int>> kept;
    auto kept_range = [&](int m, int ntrans, int specofs) {
        const auto key = std::make_pair(m, ntrans);
        const auto it = kept.find(key);
        if (it != kept.end()) return it->second;
        const int nb = ntrans / 2 + 1;
        int klo = 0, khi = nb - 1;
        if (c->comps[(size_t)m].has_filter) {
            const float *fw = c->filtw_h.data() + specofs, *ra = c->refamp_h.data() + specofs;
            while (klo <= khi && fw[klo] == 0.f) klo++;
            while (khi >= klo && fw[khi] == 0.f) khi--;
            for (int k = 0; k < nb; k++)
                if ((k < klo || k > khi) && ra[k] != 0.f)
                    throw std::runtime_error("spectral_candidates: bin " + std::to_string(k) + " of slot " + std::to_string(m + 1) +
                                             " has the filter weight 0 and a reference amplitude that is not 0");
        }
        return kept[key] = std::make_pair(klo, khi);
    };
    std::vector<SlotRec> sl;
    std::vector<float2> spec_h;
    // per group: the spectra of the basis, the slot table, the candidate outputs
    const size_t per_group = c->spec_cplx_per_src * K * sizeof(float2) + (size_t)nmis * sizeof(SlotRec) + ntile * (sizeof(double) + sizeof(int)) +
                             (size_t)cl.ncand * ((cl.misfit ? sizeof(double) : 0) + (cl.scale ? sizeof(double) : 0) + (cl.slot_misfit ? (size_t)nmis * sizeof(float) : 0)) +
                             (hook ? hook->per_group : 0);
    int g0 = 0;
    while (g0 < ngroup) {
        const int ng = next_group_chunk(c, isrc0, g0, ngroup, K, 2, per_group, c->fft_cap);
        const int s0 = isrc0 + g0 * K;
        HIPCHECK(hipEventRecord(ev[0], c->stream));
        run_chunk(c, s0, ng * K, proc_which);
        HIPCHECK(hipEventRecord(ev[1], c->stream));
        // the slot table of the chunk from its pair table (host side of run_chunk: complete when it returns)
        sl.assign((size_t)ng * nmis, SlotRec{});
        long long nbins = 0;
        int longest = 0;
        for (int g = 0; g < ng; g++) {
            bool bad = false;
            for (int i = 0; i < K; i++) if (c->src_status[(size_t)s0 + (size_t)g * K + i]) bad = true;
            for (int m = 0; m < nmis; m++) {
                SlotRec &r = sl[(size_t)g * nmis + m];
                r.sofs = nbins; r.ntrans = 0; r.klo = 0; r.khi = -1; r.specofs = 0; r.df = 0.f; r.norm = 0.f;
                if (bad) continue;
                const FftPair &p0 = c->last_pairs[((size_t)g * K) * nmis + m];
                for (int i = 1; i < K; i++)
                    if (c->last_pairs[((size_t)g * K + i) * nmis + m].ntrans != p0.ntrans)
                        throw std::runtime_error("spectral_candidates: the basis sources of group " + std::to_string(g0 + g) + " need transforms of " +
                                                 std::to_string(p0.ntrans) + " and " + std::to_string(c->last_pairs[((size_t)g * K + i) * nmis + m].ntrans) +
                                                 " samples at slot " + std::to_string(m + 1) + "; their spectra have no common bins");
                if (p0.ntrans < (1 << kFusedFftMinLog2) || p0.ntrans > (1 << kFusedFftMaxLog2) || (p0.ntrans & (p0.ntrans - 1)))
                    throw std::runtime_error("spectral_candidates: slot " + std::to_string(m + 1) + " needs a transform of " + std::to_string(p0.ntrans) +
                                             " samples; " + std::to_string(1 << kFusedFftMinLog2) + " to " + std::to_string(1 << kFusedFftMaxLog2) + " are supported");
                const std::pair<int, int> kr = kept_range(m, p0.ntrans, p0.specofs);
                r.ntrans = p0.ntrans; r.klo = kr.first; r.khi = kr.second; r.specofs = p0.specofs;
                r.df = 1.f / ((float)p0.ntrans * c->gm.dt);
                r.norm = c->norm_src_h[(size_t)s0 * nmis + ((size_t)g * K) * nmis + m];
                nbins += kr.second - kr.first + 1;
                longest = std::max(longest, p0.ntrans);
                fused_fft_table(c, p0.ntrans);
                if ((cl.spectra || cl.spectra_ref) && kr.second - kr.first + 1 > cl.spectra_bins)
                    throw std::runtime_error("spectral_candidates: slot " + std::to_string(m + 1) + " keeps " + std::to_string(kr.second - kr.first + 1) +
                                             " bins; spectra_bins = " + std::to_string(cl.spectra_bins) + " does not hold them");
            }
        }
        const size_t nc = (size_t)ng * cl.ncand;
        slots_d.ensure(std::max<size_t>(1, sl.size()) * kRecInts, &c->dev_bytes);
        spec_d.ensure(std::max<size_t>(1, (size_t)nbins * K), &c->dev_bytes);
        tile_v.ensure((size_t)ng * ntile, &c->dev_bytes); tile_i.ensure((size_t)ng * ntile, &c->dev_bytes);
        besti_d.ensure((size_t)ng, &c->dev_bytes); bestv_d.ensure((size_t)ng, &c->dev_bytes); st_d.ensure((size_t)ng, &c->dev_bytes);
        if (cl.misfit) mis_d.ensure(nc, &c->dev_bytes);
        if (cl.scale) sc_d.ensure(nc, &c->dev_bytes);
        if (cl.slot_misfit) smis_d.ensure(nc * nmis, &c->dev_bytes);
        if (!sl.empty()) HIPCHECK(hipMemcpyAsync(slots_d.p, sl.data(), sl.size() * sizeof(SlotRec), hipMemcpyHostToDevice, c->stream));
        if (cl.slot_misfit) HIPCHECK(hipMemsetAsync(smis_d.p, 0, nc * nmis * sizeof(float), c->stream));
        HIPCHECK(hipEventRecord(ev[5], c->stream));
        if (longest > 0) {
            FusedFftTables ft;
            for (int i = 0; i <= kFusedFftMaxLog2; i++) ft.tab[i] = c->fused_tab[i].p;
            hipLaunchKernelGGL(speccand_spectra_kernel, dim3((unsigned)nmis, (unsigned)(ng * K)), dim3(256), (size_t)longest * 4, c->stream,
                               c->proc_d.p, c->syn_stride, c->comps_d.p, (const SlotRec *)slots_d.p, ft, nmis, K, spec_d.p);
            HIPCHECK(hipGetLastError());
        }
        HIPCHECK(hipEventRecord(ev[2], c->stream));
        const Args a{ spec_d.p, (const SlotRec *)slots_d.p, (const SlotInfo *)info_d.p, w_d.p, x_d.p, ng, c->method, cl.outer_norm == 2 ? 1 : 0, anarchy ? 1 : 0, cl.ncand,
                      cl.misfit ? mis_d.p : (double *)nullptr, cl.scale ? sc_d.p : (double *)nullptr, cl.slot_misfit ? smis_d.p : (float *)nullptr,
                      tile_v.p, tile_i.p, st_d.p };
        if (hook) {
            hook->candidates(ng, a.spec, a.slots, a.info, a.x);
            HIPCHECK(hipEventRecord(ev[3], c->stream));
            hook->after_candidates(g0, ng, sl, st_d.p);
            HIPCHECK(hipEventRecord(ev[6], c->stream));
        } else {
            launch_any(c, K, a, cl.free_scale != 0);
            hipLaunchKernelGGL(speccand_fold_kernel, dim3((unsigned)ng), dim3(64), 0, c->stream, tile_v.p, tile_i.p, (int)ntile, besti_d.p, bestv_d.p);
            HIPCHECK(hipGetLastError());
            HIPCHECK(hipEventRecord(ev[3], c->stream));
        }
        const Call o = cl.at(g0, nmis, K);
        if (!hook) {
            HIPCHECK(hipMemcpyAsync(o.best_index, besti_d.p, (size_t)ng * sizeof(int), hipMemcpyDeviceToHost, c->stream));
            HIPCHECK(hipMemcpyAsync(o.best_misfit, bestv_d.p, (size_t)ng * sizeof(double), hipMemcpyDeviceToHost, c->stream));
        }
        HIPCHECK(hipMemcpyAsync(o.status, st_d.p, (size_t)ng * sizeof(int), hipMemcpyDeviceToHost, c->stream));
        if (cl.misfit) HIPCHECK(hipMemcpyAsync(o.misfit, mis_d.p, nc * sizeof(double), hipMemcpyDeviceToHost, c->stream));
        if (cl.scale) HIPCHECK(hipMemcpyAsync(o.scale, sc_d.p, nc * sizeof(double), hipMemcpyDeviceToHost, c->stream));
        if (cl.slot_misfit) HIPCHECK(hipMemcpyAsync(o.slot_misfit, smis_d.p, nc * nmis * sizeof(float), hipMemcpyDeviceToHost, c->stream));
        if (cl.spectra && nbins > 0) {
            spec_h.resize((size_t)nbins * K);
            HIPCHECK(hipMemcpyAsync(spec_h.data(), spec_d.p, spec_h.size() * sizeof(float2), hipMemcpyDeviceToHost, c->stream));
        }
        HIPCHECK(hipEventRecord(ev[4], c->stream));
        HIPCHECK(hipStreamSynchronize(c->stream));
        for (int g = 0; g < ng; g++)
            for (int m = 0; m < nmis; m++) {
                const SlotRec &r = sl[(size_t)g * nmis + m];
                const size_t gm = (size_t)g * nmis + m, nk = (size_t)(r.khi - r.klo + 1);
                if (o.slot_norm) o.slot_norm[gm] = r.norm;
                if (o.spectra_range) { o.spectra_range[3 * gm] = r.klo; o.spectra_range[3 * gm + 1] = r.khi; o.spectra_range[3 * gm + 2] = r.ntrans; }
                if (o.spectra) {
                    float *dst = o.spectra + gm * cl.spectra_bins * K * 2;
                    std::fill(dst, dst + (size_t)cl.spectra_bins * K * 2, 0.f);
                    if (r.ntrans) std::memcpy(dst, spec_h.data() + (size_t)r.sofs * K, nk * K * sizeof(float2));
                }
                if (o.spectra_ref) {
                    float *dst = o.spectra_ref + gm * cl.spectra_bins * 2;
                    std::fill(dst, dst + (size_t)cl.spectra_bins * 2, 0.f);
                    for (size_t k = 0; r.ntrans && k < nk; k++) {
                        dst[2 * k] = c->refamp_h[(size_t)r.specofs + r.klo + k];
                        dst[2 * k + 1] = c->filtw_h[(size_t)r.specofs + r.klo + k];
                    }
                }
            }
        // (the host's slot table, the twiddle tables of lengths seen for the first time and the table's upload lie between ev[1] and
        // ev[5]: in none of the four)
        ev.add_elapsed(c->speccand_ms, 0, 0, 1);
        ev.add_elapsed(c->speccand_ms, 1, 5, 2);
        ev.add_elapsed(c->speccand_ms, 2, 2, 3);
        ev.add_elapsed(c->speccand_ms, 3, hook ? 6 : 3, 4);
        if (hook) ev.add_elapsed(hook->ms, 0, 3, 6);
        g0 += ng;
    }
    leave_evaluated(c, isrc0, ngroup * K, proc_which);
    for_each_failed_group(c, isrc0, ngroup, K, [&](int g) { fill_failed(1, nmis, K, cl.at(g, nmis, K)); });
}

// kiwi_hip_spectral_candidates_params piece by piece (PieceCall, kiwi_group_run.hpp)
static PieceCall piece_call(int K, const double *receiver_weight, int anarchy, const Call &cl)
{
    return PieceCall{ K,
        [=](kiwi_hip_ctx *c) { check_setup(c, K, cl); },
        [=](kiwi_hip_ctx *c, int s0, int n) { fill_failed(n / K, c->nmis, K, cl.at(s0 / K, c->nmis, K)); },
        [=](kiwi_hip_ctx *c, int s0, int n) { run(c, 0, n / K, K, receiver_weight, anarchy, cl.at(s0 / K, c->nmis, K)); } };
}

} // namespace spectral_candidates
