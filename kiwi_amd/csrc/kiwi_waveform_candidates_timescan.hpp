// kiwi_waveform_candidates_timescan.hpp -- misfits of many GIVEN coefficient vectors per group at MANY origin times under the
// time-domain norms l1norm (the point of the call) and l2norm, from ONE synthesis of the basis
// (kiwi_hip_waveform_candidates_time_scan): kiwi_waveform_candidates.hpp with the time scan of kiwi_timescan.hpp inside.  A source
// moved by a whole number k of samples has the same synthetic, moved; the receiver's taper and reference stay where they are.  The
// shift is common to all receivers and the taper stays with the REFERENCE side of the window, so -- unlike
// kiwi_waveform_candidates_floating.hpp, where the taper stays with the synthetic -- the candidate's combined trace is formed from the
// UNTAPERED rows, once per extended sample, and a further offset costs one taper product, a subtraction, a |.| and one fp64 add.
// Included by kiwi_hip.hip behind kiwi_waveform_candidates_floating.hpp under the same -ffp-contract=off: every fp32 and fp64
// operation below is rounded on its own, and tests/waveform_candidates_timescan_restatement.py restates each in the same order (the
// GPU tests ask for bit identity of the kernels with that restatement fed with the device's own rows).
//
// Sources [isrc0, isrc0 + ngroup K) are ngroup groups of K <= 8 consecutive basis sources.  Offsets k_j = k0 + j kstep, j < nk,
// S = max |k_j| (kiwi_hip_time_scan's, with its limits).  Per chunk of whole groups:
//   evaluate    timescan::HaloScope::widen(S) and run_chunk(..., 0) with the plain synthetics in memory, as linfit_timescan::run:
//               misfits, norm factors and global misfits of the basis sources are left as kiwi_hip_eval leaves them (offset 0's
//               plain evaluation); halo and want_spansrc are put back on the way out
//   rows        wavecand_scan_rows_kernel, one workgroup per (chunk source, slot): row_a[e] = folded_scaled_sample at extended
//               sample e = -S .. wlen + S - 1 -- folded, moment-scaled, UNTAPERED, the rows linfit_scan_gram_kernel and
//               time_scan_kernel work on -- to rows[chunk source][row_stride], slot m at row_offset[m] (the slots' wlen + 2 S side by
//               side), so that no workgroup of the scan folds again.  A group with a failed basis source reads as zeros.
//   scan        wavecand_scan_kernel<K, METHOD> (METHOD 1 l2 inside, 2 l1 inside), one workgroup of kThreads lanes per (tile of
//               kThreads candidates, slot, (group, pass of J = offsets_per_pass(K) consecutive offsets)); a lane owns ONE candidate
//               with xf = (float) x in registers.  Extended samples e ascending over [-k_last, wlen - 1 - k_first] of the pass,
//               kStage at a time in LDS: a staged sample carries the K row values and per offset of the pass the pair
//               (taper[e + k_j], ref[e + k_j]) (ref: the tapered reference; zeros outside the window), read as 16-byte broadcasts:
//                   u = xf_0 row_0[e]; u = u + xf_a row_a[e] (a ascending, fp32)                      (once per sample)
//                   i = e + k_j inside [0, wlen):   vt = u * taper[i]                                 (one fp32 product)
//                   d = unit ? ref[i] - vt : 1.f ref[i] - syn_factor vt                               (misfit_kernel's expressions)
//                   l2: acc_j = sq_acc(acc_j, d)  |  l1: acc_j += (double) fabsf(d)                   (ONE fp64 accumulator per offset)
//               A sample outside the window contributes nothing, also where u is not finite; whether it lies inside is
//               workgroup-uniform (the head and the tail of the range, at most k_last - k_first samples each, are walked with the
//               test, the body without).  m = (float) sqrt((double) dt acc_j) | (float) ((double) dt acc_j) to
//               slab[(group nk + j)][slot][candidate].  An accumulator sees its window samples i ascending whatever the pass.
//   fold        wavecand_fold_kernel and speccand_fold_kernel unchanged over ngroup x nk "groups" (the norm row and `ok` of group g
//               repeated per offset: the norm factors do not depend on k); wavecand_scan_best_kernel then gives per (group,
//               candidate) the first smallest misfit over the offsets and its index -- NaN passed over, then the value, then the
//               lowest index: linfit::take_better's total order --, and per group the best offset the same way from the offsets'
//               best misfits and the status (that of offset 0: the denominator of the fold does not depend on k).
// No atomics, zero scratch (profiles/waveform_candidates_time_scan_kernel_resources.json).  The answer does not depend on tiles,
// passes, chunking (KIWI_HIP_CHUNK_MB), isrc0, the piece or the device count.  A unit candidate e_a gives u = row_a exactly (the
// other products are +-0): its slot misfit at offset k is kiwi_hip_time_scan's for basis source a up to the order of the fp64 sum.
// Offset 0 is NOT kiwi_hip_waveform_candidates bit for bit: that call tapers every basis trace before combining
// (x_a fl(row_a taper)), this one combines first (fl(sum_a x_a row_a) taper); the two differ by rounding.
// Status of a group: 0 evaluated; 1 no receiver counts: NaN, best_index -1, best_offset -1; 2 a basis source failed to discretise
// (host).

namespace waveform_candidates_timescan {

using waveform_candidates::kMaxBasis;
using waveform_candidates::kStage;
using waveform_candidates::kThreads;
using spectral_candidates::SlotInfo;

// floats per staged sample: the K rows and J (taper, reference) pairs in whole 16-byte reads, J at least 8: 8 or 9 offsets, 20 or
// 24 floats (24 KiB per stage at K = 8); per lane 2 J registers of accumulators, no scratch
__host__ __device__ constexpr int row_floats(int K) { return (K + 16 + 3) / 4 * 4; }
__host__ __device__ constexpr int offsets_per_pass(int K) { return (row_floats(K) - K) / 2; }

// floats of one source's rows: the slots' wlen + 2 S side by side (no padding); ofs (or null): [nmis + 1] where each slot begins
static size_t row_stride(const kiwi_hip_ctx *c, int S, std::vector<int> *ofs = nullptr)
{
    size_t n = 0;
    if (ofs) ofs->clear();
    for (const CompDev &cd : c->comps) {
        if (ofs) ofs->push_back((int)n);
        n += (size_t)cd.wlen + 2 * (size_t)S;
    }
    if (ofs) ofs->push_back((int)n);
    return n;
}

// sr: the plain synthetics of the chunk, rows with the scan halo; ok: [group nk] (read at group nk); rofs: [nmis + 1].
// blockIdx.x = chunk source, blockIdx.y = slot
__global__ __launch_bounds__(256) void wavecand_scan_rows_kernel(SynRows sr, const int *__restrict__ ok, const int *__restrict__ rofs, int K,
                                                                 int nk, int isrc0, int S, size_t rstride, float dt, float *__restrict__ rows)
{
    __shared__ float fw[kMaxFold];
    __shared__ int fs[kMaxFold];
    __shared__ float fr[kMaxFold];
    __shared__ int nfold;
    const int tid = (int)threadIdx.x, s = (int)blockIdx.x, m = (int)blockIdx.y;
    const CompDev cd = sr.comps[m];
    const int ext = cd.wlen + 2 * S;
    float *__restrict__ out = rows + (size_t)s * rstride + rofs[m];
    if (!ok[(size_t)(s / K) * nk]) {                       // (workgroup-uniform)
        for (int e = tid; e < ext; e += 256) out[e] = 0.f;
        return;
    }
    if (tid == 0) nfold = fold_setup(sr.risetime[isrc0 + s], dt, fw, fs, fr);
    __syncthreads();
    const int nf = nfold;
    const float mom = sr.moment[isrc0 + s];
    const float *__restrict__ sy = sr.syn + (size_t)s * sr.syn_stride + cd.synofs + cd.halo;      // sy[i] = window sample i; cd.halo = fold halo + S
    for (int e = tid; e < ext; e += 256) out[e] = folded_scaled_sample(sy, e - S, nf, fw, fs, fr, mom);
}

struct ScanArgs {
    const float *rows; size_t rstride;  // wavecand_scan_rows_kernel's
    const int *rofs;                    // [nmis + 1]
    const CompDev *comps;
    const float *taper, *reft;          // taper weights and tapered references over the windows, [refofs + i]
    const int *ok;                      // [group nk] (read at group nk)
    const float *x;                     // [ncand][K]
    int nmis, ncand, k0, kstep, nk, S;
    float syn_factor, dt;
    float *slab;                        // [(group nk + offset)][slot][ncand]
};

// staged samples [n_from, n_to) of a stage whose sample 0 puts offset 0 of the pass at window sample i_first; CHECK: some offset's
// sample may lie outside the window [0, wlen)
template <int K, int J, int METHOD, bool CHECK>
__device__ __forceinline__ void scan_samples(const float *sS, int n_from, int n_to, int i_first, int kstep, int nj, int wlen, const float (&xf)[K],
                                             bool unit, float syn_factor, double (&acc)[J])
{
    constexpr int R = row_floats(K);
#pragma unroll 2
    for (int n = n_from; n < n_to; n++) {
        float s[R];
#pragma unroll
        for (int p = 0; p < R; p += 4) {
            const float4 t = *reinterpret_cast<const float4 *>(sS + n * R + p);
            s[p] = t.x; s[p + 1] = t.y; s[p + 2] = t.z; s[p + 3] = t.w;
        }
        float u = xf[0] * s[0];
#pragma unroll
        for (int a = 1; a < K; a++) u = u + xf[a] * s[a];
#pragma unroll
        for (int j = 0; j < J; j++) {
            if (CHECK) {                                 // (workgroup-uniform)
                const int i = i_first + n + j * kstep;
                if (j >= nj || i < 0 || i >= wlen) continue;
            }
            const float vt = u * s[K + 2 * j];           // make_array_tapered, comparator.f90:1173-1184
            const float rv = s[K + 2 * j + 1];
            const float d = unit ? (rv - vt) : (1.f * rv - syn_factor * vt);
            if (METHOD == 1) acc[j] = sq_acc(acc[j], d);
            else acc[j] += (double)fabsf(d);
        }
    }
}

// blockIdx.x = tile of candidates, blockIdx.y = slot, blockIdx.z = group x passes + pass
template <int K, int METHOD>
__global__ __launch_bounds__(kThreads) void wavecand_scan_kernel(ScanArgs a)
{
    constexpr int R = row_floats(K), J = offsets_per_pass(K);
    static_assert(kStage == kThreads, "a staging thread forms one sample of a stage");
    static_assert(K + 2 * J <= R && R % 4 == 0 && J >= 8, "a staged sample is whole 16-byte reads");
    __shared__ __attribute__((aligned(16))) float sS[kStage * R];
    const int tid = (int)threadIdx.x, m = (int)blockIdx.y;
    const int npass = (a.nk + J - 1) / J, g = (int)blockIdx.z / npass, j0 = ((int)blockIdx.z - g * npass) * J;
    if (!a.ok[(size_t)g * a.nk]) return;                 // (workgroup-uniform, as every branch on cd, nj and the offsets below)
    const int cand = (int)blockIdx.x * kThreads + tid;
    const bool live = cand < a.ncand;
    const bool unit = (a.syn_factor == 1.f);
    const CompDev cd = a.comps[m];
    const int nj = a.nk - j0 < J ? a.nk - j0 : J;
    const int kf = a.k0 + j0 * a.kstep, kl = kf + (nj - 1) * a.kstep;       // first and last offset of the pass
    // rw[a rstride + e] = row_a[e], e in [-S, wlen + S); the pass reads e in [-kl, wlen - kf), inside it as |kf|, |kl| <= S
    const float *__restrict__ rw = a.rows + (size_t)g * K * a.rstride + a.rofs[m] + a.S;
    const float *__restrict__ tp = a.taper + cd.refofs;
    const float *__restrict__ rt = a.reft + cd.refofs;
    float xf[K];
#pragma unroll
    for (int b = 0; b < K; b++) xf[b] = live ? a.x[(size_t)cand * K + b] : 0.f;
    double acc[J];
#pragma unroll
    for (int j = 0; j < J; j++) acc[j] = 0.0;
    const int e_lo = -kl, e_hi = cd.wlen > 0 ? cd.wlen - kf : e_lo;         // the pass's extended samples [e_lo, e_hi)
    const int b_lo = -kf, b_hi = cd.wlen - kl;                              // [b_lo, b_hi): every offset's sample is inside the window
    for (int e0 = e_lo; e0 < e_hi; e0 += kStage) {
        const int nst = e_hi - e0 < kStage ? e_hi - e0 : kStage;
        __syncthreads();                                 // the stage before this one has been read by every wavefront
        if (tid < nst) {                                 // (the rows are contiguous in e: coalesced loads)
            const int e = e0 + tid;
            float t[R];
#pragma unroll
            for (int b = 0; b < K; b++) t[b] = rw[(size_t)b * a.rstride + e];
#pragma unroll
            for (int j = 0; j < J; j++) {
                const int i = e + kf + j * a.kstep;
                const bool in = j < nj && i >= 0 && i < cd.wlen;
                const int ic = i < 0 ? 0 : (i < cd.wlen ? i : cd.wlen - 1);             // (never read outside the window's tables)
                const float tv = tp[ic], rv = rt[ic];
                t[K + 2 * j] = in ? tv : 0.f;
                t[K + 2 * j + 1] = in ? rv : 0.f;
            }
#pragma unroll
            for (int p = K + 2 * J; p < R; p++) t[p] = 0.f;
#pragma unroll
            for (int p = 0; p < R; p += 4)
                *reinterpret_cast<float4 *>(sS + tid * R + p) = make_float4(t[p], t[p + 1], t[p + 2], t[p + 3]);
        }
        __syncthreads();
        int n1 = b_lo - e0, n2 = b_hi - e0;
        n1 = n1 < 0 ? 0 : (n1 < nst ? n1 : nst);
        n2 = n2 < n1 ? n1 : (n2 < nst ? n2 : nst);
        scan_samples<K, J, METHOD, true>(sS, 0, n1, e0 + kf, a.kstep, nj, cd.wlen, xf, unit, a.syn_factor, acc);
        scan_samples<K, J, METHOD, false>(sS, n1, n2, e0 + kf, a.kstep, nj, cd.wlen, xf, unit, a.syn_factor, acc);
        scan_samples<K, J, METHOD, true>(sS, n2, nst, e0 + kf, a.kstep, nj, cd.wlen, xf, unit, a.syn_factor, acc);
    }
    if (!live) return;
#pragma unroll
    for (int j = 0; j < J; j++)
        if (j < nj) {
            const float mf = METHOD == 1 ? (float)sqrt((double)a.dt * acc[j]) : (float)((double)a.dt * acc[j]);
            a.slab[(((size_t)g * a.nk + j0 + j) * a.nmis + m) * a.ncand + cand] = mf;
        }
}

// misfit: [group][nk][ncand] (read only with cand_misfit); best_misfit_j, best_index_j, status_j: [group][nk], the fold kernels';
// cand_misfit, cand_offset: [group][ncand] or null; best_offset, status: [group].  blockIdx.y = group.  The LAST block of a group
// walks the offsets' bests; with cand_misfit the blocks in front of it walk the offsets of a candidate per thread
__global__ __launch_bounds__(kThreads) void wavecand_scan_best_kernel(const double *__restrict__ misfit, const double *__restrict__ best_misfit_j,
                                                                      const int *__restrict__ best_index_j, const int *__restrict__ status_j,
                                                                      int nk, int ncand, double *__restrict__ cand_misfit,
                                                                      int *__restrict__ cand_offset, int *__restrict__ best_offset,
                                                                      int *__restrict__ status)
{
    const int g = (int)blockIdx.y, tid = (int)threadIdx.x;
    double v = 0.0;
    int o = -1;
    if (blockIdx.x + 1 == gridDim.x) {
        if (tid != 0) return;
        for (int j = 0; j < nk; j++) linfit::take_better(v, o, best_misfit_j[(size_t)g * nk + j], best_index_j[(size_t)g * nk + j] >= 0 ? j : -1);
        best_offset[g] = o;
        status[g] = status_j[(size_t)g * nk];
        return;
    }
    const int cand = (int)blockIdx.x * kThreads + tid;
    if (cand >= ncand) return;
    for (int j = 0; j < nk; j++) {
        const double mv = misfit[((size_t)g * nk + j) * ncand + cand];
        linfit::take_better(v, o, mv, mv == mv ? j : -1);
    }
    cand_misfit[(size_t)g * ncand + cand] = o >= 0 ? v : __longlong_as_double(0x7ff8000000000000LL);
    if (cand_offset) cand_offset[(size_t)g * ncand + cand] = o;
}

// host arrays of the caller for the groups of ONE call of run().  x [ncand][K], shared by all groups.  best_offset, status [group];
// best_index, best_misfit [group][nk]; the others may be null: cand_misfit, cand_offset [group][ncand] (the offset: an index j, -1
// where every offset is NaN); misfit [group][nk][ncand]; slot_misfit [group][nk][ncand][nmis] and slot_norm [group][nmis] (both or
// neither: with nk x ncand read as sources, the pair kiwi_hip_outer_misfits takes); rows [group][K][row_stride]
struct Call {
    const double *x; int ncand, outer_norm;
    int *best_offset, *best_index; double *best_misfit; int *status;
    double *cand_misfit; int *cand_offset;
    double *misfit;
    float *slot_misfit, *slot_norm, *rows;
    Call at(size_t g, size_t nmis, size_t nk, size_t K, size_t rstride) const
    {
        Call c = *this;
        c.best_offset += g; c.best_index += g * nk; c.best_misfit += g * nk; c.status += g;
        if (cand_misfit) c.cand_misfit += g * ncand;
        if (cand_offset) c.cand_offset += g * ncand;
        if (misfit) c.misfit += g * nk * ncand;
        if (slot_misfit) c.slot_misfit += g * nk * ncand * nmis;
        if (slot_norm) c.slot_norm += g * nmis;
        if (rows) c.rows += g * K * rstride;
        return c;
    }
};

// what the call cannot do is refused before anything runs, nothing approximated: what kiwi_hip_waveform_candidates refuses, what
// kiwi_hip_time_scan refuses of the offsets, and a misfit filter.  Leaves the context prepared
static void check_setup(kiwi_hip_ctx *c, int K, const timescan::Offsets &of, const Call &cl)
{
    refusing("waveform_candidates_time_scan", [&] {
        if (!cl.best_offset) throw std::runtime_error("null best_offset array");
        if (cl.cand_offset && !cl.cand_misfit) throw std::runtime_error("a cand_offset array without cand_misfit");
        if (cl.slot_misfit && !cl.slot_norm) throw std::runtime_error("a slot_misfit array without slot_norm");
        waveform_candidates::check_setup(c, K, waveform_candidates::Call{ cl.x, cl.ncand, cl.outer_norm, cl.best_index, cl.best_misfit, cl.status,
                                                                          nullptr, cl.slot_misfit, cl.slot_norm });
        timescan::check_setup(c, of.k0, of.kstep, of.nk);
        if (c->any_filter)                                 // (prepare(): a filter on an enabled receiver with components)
            throw std::runtime_error("an enabled receiver has a misfit filter; the taper sits in front of the filter, so every candidate and "
                                     "offset would need a transform of its own, which is not supported");
        if (row_stride(c, of.max_abs()) > 0x7fffffffULL)   // (the slots' offsets inside a source's rows are ints, here as in the rows query)
            throw std::runtime_error("a source's rows do not fit an int");
    });
}

static void fill_failed(size_t ngroup, size_t nmis, size_t nk, size_t K, size_t rstride, const Call &cl)
{
    const double nan = std::numeric_limits<double>::quiet_NaN();
    const size_t nj = ngroup * nk, nc = ngroup * (size_t)cl.ncand, njc = nj * (size_t)cl.ncand;
    std::fill(cl.status, cl.status + ngroup, 2);
    std::fill(cl.best_offset, cl.best_offset + ngroup, -1);
    std::fill(cl.best_index, cl.best_index + nj, -1);
    std::fill(cl.best_misfit, cl.best_misfit + nj, nan);
    if (cl.cand_misfit) std::fill(cl.cand_misfit, cl.cand_misfit + nc, nan);
    if (cl.cand_offset) std::fill(cl.cand_offset, cl.cand_offset + nc, -1);
    if (cl.misfit) std::fill(cl.misfit, cl.misfit + njc, nan);
    if (cl.slot_misfit) std::fill(cl.slot_misfit, cl.slot_misfit + njc * nmis, 0.f);
    if (cl.slot_norm) std::fill(cl.slot_norm, cl.slot_norm + ngroup * nmis, 0.f);
    if (cl.rows) std::fill(cl.rows, cl.rows + ngroup * K * rstride, 0.f);
}

template <int K>
static void launch(kiwi_hip_ctx *c, const ScanArgs &a, int ng)
{
    constexpr int J = offsets_per_pass(K);
    const int ntile = (a.ncand + kThreads - 1) / kThreads, npass = (a.nk + J - 1) / J;
    const dim3 grid((unsigned)ntile, (unsigned)a.nmis, (unsigned)(ng * npass));
    if (c->method == KIWI_L2NORM) hipLaunchKernelGGL((wavecand_scan_kernel<K, 1>), grid, dim3(kThreads), 0, c->stream, a);
    else hipLaunchKernelGGL((wavecand_scan_kernel<K, 2>), grid, dim3(kThreads), 0, c->stream, a);
    HIPCHECK(hipGetLastError());
}

// what a call built on this one (kiwi_waveform_candidates_bootstrap.hpp) adds to every chunk: its device bytes per group, its bound
// on the groups of a chunk, and its kernels on the chunk's slab and norm rows [(group nk + j)][slot], launched behind the fold kernels
// and in front of the downloads; their HIP-event time is added to ms[0]
struct ChunkHook {
    size_t per_group = 0;
    int max_groups = std::numeric_limits<int>::max();
    float *ms = nullptr;
    virtual void after_fold(int g0, int ng, const float *slab, const float *norm) = 0;
    virtual ~ChunkHook() = default;
};

// the groups [isrc0, isrc0 + ngroup K) of the uploaded batch, on waveform_candidates::run's skeleton inside linfit_timescan::run's
// halo; adds its HIP-event times to c->wavecand_scan_ms: evaluation (run_chunk), rows + scan kernel, the fold kernels, the downloads
static void run(kiwi_hip_ctx *c, int isrc0, int ngroup, int K, const timescan::Offsets &of, const double *receiver_weight, int anarchy,
                const Call &cl, ChunkHook *hook = nullptr)
{
    check_setup(c, K, of, cl);
    check_group_range("waveform_candidates_time_scan", c, isrc0, ngroup, K);
    if (ngroup == 0) return;
    const int nrec = (int)c->recv.size(), nmis = c->nmis, nk = of.nk, S = of.max_abs();
    c->misfit_d.ensure((size_t)c->nsrc * c->nmis, &c->dev_bytes);
    c->global_d.ensure((size_t)c->nsrc, &c->dev_bytes);
    c->fuse_now = false;                                   // the plain synthetics go to memory
    // every source is synthesised (run_chunk shares no synthetics between sources then), as in timescan::run
    timescan::HaloScope halo(c);
    halo.widen(S);

    const std::vector<double> w = receiver_weights(c, receiver_weight);
    std::vector<SlotInfo> info((size_t)nmis);
    for (int m = 0; m < nmis; m++)
        info[(size_t)m] = SlotInfo{ c->comps[(size_t)m].rec, (m + 1 == nmis || c->comps[(size_t)m + 1].rec != c->comps[(size_t)m].rec) ? 1 : 0, 0, 0 };
    std::vector<float> xf((size_t)cl.ncand * K);
    for (size_t p = 0; p < xf.size(); p++) xf[p] = (float)cl.x[p];
    std::vector<int> rofs;
    const size_t rstride = row_stride(c, S, &rofs);
    const size_t ntile = (size_t)(cl.ncand + kThreads - 1) / kThreads;
    const bool want_misfit = cl.misfit || cl.cand_misfit;
    // device buffers of the call: kept on the context and grown only
    auto &B = c->wavecand_scan_bufs;
    constexpr size_t kInfoInts = sizeof(SlotInfo) / sizeof(int);
    B.w.ensure((size_t)std::max(nrec, 1), &c->dev_bytes);
    B.x.ensure(xf.size(), &c->dev_bytes);
    B.info.ensure((size_t)std::max(nmis, 1) * kInfoInts, &c->dev_bytes);
    B.rofs.ensure(rofs.size(), &c->dev_bytes);
    // (w, info, xf, rofs and the tables of a chunk are read by these copies: nothing leaves this function, by return or by exception,
    // before the stream is drained)
    struct Drain { hipStream_t s; ~Drain() { (void)hipStreamSynchronize(s); } } drain{ c->stream };
    HIPCHECK(hipMemcpyAsync(B.w.p, w.data(), (size_t)nrec * sizeof(double), hipMemcpyHostToDevice, c->stream));
    HIPCHECK(hipMemcpyAsync(B.x.p, xf.data(), xf.size() * sizeof(float), hipMemcpyHostToDevice, c->stream));
    if (nmis > 0) HIPCHECK(hipMemcpyAsync(B.info.p, info.data(), (size_t)nmis * sizeof(SlotInfo), hipMemcpyHostToDevice, c->stream));
    HIPCHECK(hipMemcpyAsync(B.rofs.p, rofs.data(), rofs.size() * sizeof(int), hipMemcpyHostToDevice, c->stream));

    const PooledEvents<7> ev(c);                           // (ev[5]: immediately in front of the rows kernel; ev[6]: behind the hook)
    std::vector<float> norm_h;
    std::vector<int> ok_h;
    // per group: the rows, and at every offset the slab of slot misfits, the norm factors, the tiles' bests, the outputs
    const size_t per_group = (size_t)K * rstride * sizeof(float) +
                             (size_t)nk * ((size_t)nmis * cl.ncand * sizeof(float) + (size_t)nmis * sizeof(float) + 2 * sizeof(int) +
                                           ntile * (sizeof(double) + sizeof(int)) + sizeof(double) + sizeof(int) +
                                           (size_t)cl.ncand * ((want_misfit ? sizeof(double) : 0) + (cl.slot_misfit ? (size_t)nmis * sizeof(float) : 0))) +
                             (size_t)cl.ncand * ((cl.cand_misfit ? sizeof(double) : 0) + (cl.cand_offset ? sizeof(int) : 0)) + 2 * sizeof(int) +
                             (hook ? hook->per_group : 0);
    int g0 = 0;
    while (g0 < ngroup) {
        // (at most 65535 / nk groups: groups x offsets is a grid dimension of the fold, groups x passes one of the scan)
        const int ng = next_group_chunk(c, isrc0, g0, ngroup, K, 1, per_group, K * std::min(65535 / nk, hook ? hook->max_groups : 65535));
        const int s0 = isrc0 + g0 * K;
        HIPCHECK(hipEventRecord(ev[0], c->stream));
        run_chunk(c, s0, ng * K, 0);
        HIPCHECK(hipEventRecord(ev[1], c->stream));
        // the norm factors of the chunk's slots, the same at every offset, and which of its groups are evaluated at all
        const size_t nj = (size_t)ng * nk, njc = nj * cl.ncand, nc = (size_t)ng * cl.ncand;
        norm_h.assign(nj * nmis, 0.f);
        ok_h.assign(nj, 1);
        for (int g = 0; g < ng; g++) {
            bool ok = true;
            for (int i = 0; i < K; i++) if (c->src_status[(size_t)s0 + (size_t)g * K + i]) ok = false;
            for (int j = 0; j < nk; j++) {
                ok_h[(size_t)g * nk + j] = ok ? 1 : 0;
                if (ok) std::copy(c->norm_h.begin(), c->norm_h.begin() + nmis, norm_h.begin() + ((size_t)g * nk + j) * nmis);
            }
        }
        B.rows.ensure(std::max<size_t>(1, (size_t)ng * K * rstride), &c->dev_bytes);
        B.slab.ensure(std::max<size_t>(1, njc * nmis), &c->dev_bytes);
        B.norm.ensure(std::max<size_t>(1, norm_h.size()), &c->dev_bytes);
        B.ok.ensure(nj, &c->dev_bytes);
        B.tile_v.ensure(nj * ntile, &c->dev_bytes); B.tile_i.ensure(nj * ntile, &c->dev_bytes);
        B.best_index.ensure(nj, &c->dev_bytes); B.best_misfit.ensure(nj, &c->dev_bytes); B.status_j.ensure(nj, &c->dev_bytes);
        B.status.ensure((size_t)ng, &c->dev_bytes); B.best_offset.ensure((size_t)ng, &c->dev_bytes);
        if (want_misfit) B.misfit.ensure(njc, &c->dev_bytes);
        if (cl.cand_misfit) B.cand_misfit.ensure(nc, &c->dev_bytes);
        if (cl.cand_offset) B.cand_offset.ensure(nc, &c->dev_bytes);
        if (cl.slot_misfit) B.smis.ensure(std::max<size_t>(1, njc * nmis), &c->dev_bytes);
        if (!norm_h.empty()) HIPCHECK(hipMemcpyAsync(B.norm.p, norm_h.data(), norm_h.size() * sizeof(float), hipMemcpyHostToDevice, c->stream));
        HIPCHECK(hipMemcpyAsync(B.ok.p, ok_h.data(), ok_h.size() * sizeof(int), hipMemcpyHostToDevice, c->stream));
        if (cl.slot_misfit && nmis > 0) HIPCHECK(hipMemsetAsync(B.smis.p, 0, njc * nmis * sizeof(float), c->stream));
        HIPCHECK(hipEventRecord(ev[5], c->stream));
        if (nmis > 0) {
            const SynRows sr{ c->syn_d.p, c->syn_stride, c->comps_d.p, c->tw_d.p, c->moment_d.p, c->risetime_d.p, nullptr };
            hipLaunchKernelGGL(wavecand_scan_rows_kernel, dim3((unsigned)(ng * K), (unsigned)nmis), dim3(256), 0, c->stream, sr, B.ok.p, B.rofs.p, K, nk,
                               s0, S, rstride, c->gm.dt, B.rows.p);
            HIPCHECK(hipGetLastError());
            const ScanArgs a{ B.rows.p, rstride, B.rofs.p, c->comps_d.p, c->tw_d.p, c->reft_d.p, B.ok.p, B.x.p, nmis, cl.ncand, of.k0, of.kstep, nk, S,
                              c->syn_factor, c->gm.dt, B.slab.p };
            by_basis(K, [&](auto k) { launch<k.value>(c, a, ng); });
        }
        HIPCHECK(hipEventRecord(ev[2], c->stream));
        hipLaunchKernelGGL(waveform_candidates::wavecand_fold_kernel, dim3((unsigned)ntile, (unsigned)nj), dim3(kThreads), 0, c->stream, B.slab.p,
                           B.norm.p, B.ok.p, (const SlotInfo *)B.info.p, B.w.p, nmis, cl.outer_norm == 2 ? 1 : 0, anarchy ? 1 : 0, cl.ncand,
                           want_misfit ? B.misfit.p : (double *)nullptr, cl.slot_misfit ? B.smis.p : (float *)nullptr, B.tile_v.p, B.tile_i.p, B.status_j.p);
        HIPCHECK(hipGetLastError());
        hipLaunchKernelGGL(spectral_candidates::speccand_fold_kernel, dim3((unsigned)nj), dim3(64), 0, c->stream, B.tile_v.p, B.tile_i.p, (int)ntile,
                           B.best_index.p, B.best_misfit.p);
        HIPCHECK(hipGetLastError());
        hipLaunchKernelGGL(wavecand_scan_best_kernel, dim3((unsigned)((cl.cand_misfit ? ntile : 0) + 1), (unsigned)ng), dim3(kThreads), 0, c->stream,
                           want_misfit ? B.misfit.p : (const double *)nullptr, B.best_misfit.p, B.best_index.p, B.status_j.p, nk, cl.ncand,
                           cl.cand_misfit ? B.cand_misfit.p : (double *)nullptr, cl.cand_offset ? B.cand_offset.p : (int *)nullptr, B.best_offset.p,
                           B.status.p);
        HIPCHECK(hipGetLastError());
        HIPCHECK(hipEventRecord(ev[3], c->stream));
        if (hook) hook->after_fold(g0, ng, B.slab.p, B.norm.p);
        HIPCHECK(hipEventRecord(ev[6], c->stream));
        const Call o = cl.at((size_t)g0, (size_t)nmis, (size_t)nk, (size_t)K, rstride);
        auto down = [&](void *dst, const void *src, size_t bytes) { if (dst && bytes) HIPCHECK(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, c->stream)); };
        down(o.best_offset, B.best_offset.p, (size_t)ng * sizeof(int));
        down(o.status, B.status.p, (size_t)ng * sizeof(int));
        down(o.best_index, B.best_index.p, nj * sizeof(int));
        down(o.best_misfit, B.best_misfit.p, nj * sizeof(double));
        down(o.cand_misfit, B.cand_misfit.p, nc * sizeof(double));
        down(o.cand_offset, B.cand_offset.p, nc * sizeof(int));
        down(o.misfit, B.misfit.p, njc * sizeof(double));
        down(o.slot_misfit, B.smis.p, njc * nmis * sizeof(float));
        if (nmis > 0) down(o.rows, B.rows.p, (size_t)ng * K * rstride * sizeof(float));
        HIPCHECK(hipEventRecord(ev[4], c->stream));
        HIPCHECK(hipStreamSynchronize(c->stream));
        if (o.slot_norm)
            for (int g = 0; g < ng; g++) std::copy(norm_h.begin() + (size_t)g * nk * nmis, norm_h.begin() + ((size_t)g * nk + 1) * nmis, o.slot_norm + (size_t)g * nmis);
        // (the host's tables of the chunk and their upload lie between ev[1] and ev[5]: in none of the four)
        ev.add_elapsed(c->wavecand_scan_ms, 0, 0, 1);
        ev.add_elapsed(c->wavecand_scan_ms, 1, 5, 2);
        ev.add_elapsed(c->wavecand_scan_ms, 2, 2, 3);
        ev.add_elapsed(c->wavecand_scan_ms, 3, 6, 4);
        if (hook) ev.add_elapsed(hook->ms, 0, 3, 6);
        g0 += ng;
    }
    leave_evaluated(c, isrc0, ngroup * K, 0);              // the plain evaluation of the basis sources -- offset 0 -- was made on the way
    for_each_failed_group(c, isrc0, ngroup, K, [&](int g) {
        fill_failed(1, (size_t)nmis, (size_t)nk, (size_t)K, rstride, cl.at((size_t)g, (size_t)nmis, (size_t)nk, (size_t)K, rstride));
    });
}

// kiwi_hip_waveform_candidates_time_scan_params piece by piece (PieceCall, kiwi_group_run.hpp); the rows have the same layout on
// every device and in every piece
static PieceCall piece_call(int K, const timescan::Offsets &of, const double *receiver_weight, int anarchy, const Call &cl)
{
    const size_t nk = (size_t)of.nk;
    auto mine = [=](const kiwi_hip_ctx *c, int s0) { return cl.at((size_t)(s0 / K), (size_t)c->nmis, nk, (size_t)K, row_stride(c, of.max_abs())); };
    return PieceCall{ K,
        [=](kiwi_hip_ctx *c) { check_setup(c, K, of, cl); },
        [=](kiwi_hip_ctx *c, int s0, int n) {
            fill_failed((size_t)(n / K), (size_t)c->nmis, nk, (size_t)K, row_stride(c, of.max_abs()), mine(c, s0));
        },
        [=](kiwi_hip_ctx *c, int s0, int n) { run(c, 0, n / K, K, of, receiver_weight, anarchy, mine(c, s0)); } };
}

} // namespace waveform_candidates_timescan
