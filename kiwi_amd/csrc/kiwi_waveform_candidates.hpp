// kiwi_waveform_candidates.hpp -- misfits of many GIVEN coefficient vectors per group under the time-domain norms l1norm (the
// point of the call) and l2norm.  The l1 misfit is not quadratic in the coefficients, but the waveform is linear in them: a
// candidate x at a location is v[t] = sum_a x_a s_a[t] with s_a the kept traces of the K basis sources, so a candidate costs K
// multiply-adds and one |.| per window sample and no synthesis.  The time-domain twin of kiwi_spectral_candidates.hpp, included
// by kiwi_hip.hip behind it under the same -ffp-contract=off: every fp32 and fp64 operation below is rounded on its own, and
// tests/waveform_candidates_restatement.py restates each in the same order (the GPU tests ask for bit identity of the kernels
// with that restatement fed with the device's own kept traces).
//
// Sources [isrc0, isrc0 + ngroup K) are ngroup groups of K <= 8 consecutive basis sources, as for kiwi_hip_linear_fit.  Per chunk
// of whole groups:
//   evaluate    run_chunk with the processed rows kept in proc_d exactly as kiwi_hip_linear_fit keeps them (tapered, folded,
//               moment-scaled; filtered where a receiver has a misfit filter; WITHOUT the synthetics factor): misfits, norm factors
//               and global misfits of the basis sources are left exactly as kiwi_hip_eval leaves them
//   slots       wavecand_slot_kernel<K, METHOD>, one workgroup of kThreads lanes per (tile of kThreads candidates, slot, group); a
//               lane owns ONE candidate with xf = (float) x in registers.  kStage samples of the slot's K rows and of its reference
//               side (linfit_gram_kernel's: the filtered reference of the group's first source where the slot has a filter, else
//               the tapered one) are staged in LDS, a sample's K + 1 operands side by side, and read as broadcasts; samples
//               i = 0 .. wlen - 1 ascending into ONE fp64 accumulator per lane:
//                   v = xf_0 s_0[i]; v = v + xf_a s_a[i] (a ascending, fp32);
//                   d = unit ? a_i - v : 1.f a_i - syn_factor v      (misfit_kernel's expressions)
//                   l2norm: acc = sq_acc(acc, d)  |  l1norm: acc += (double) fabsf(d)
//               slot misfit m = (float) sqrt((double) dt acc) | (float) ((double) dt acc) to slab[group][slot][candidate].
//   fold        wavecand_fold_kernel, one candidate per lane, slots ascending from the slab: the expression sequence of
//               speccand_kernel's non-FREE branch, i.e. kiwi_hip_outer_misfits for one draw of weights 1, per SLOT: per receiver r
//               (ascending) M, N = sums (l2norm: roots of sums of squares) of its slots' m, n in fp64 (n: the norm factor of the
//               group's FIRST source); rw = w_r, anarchy: q = rw / (N != 0 ? N : -1), rw = q > 0 or NaN ? q : 0; av = M rw,
//               bv = N rw (squared under l2norm); ms = ms + av 1.0; ns = ns + bv 1.0; misfit = ms / ns (root under l2norm) where
//               ns > 0, else NaN; a negative or NaN quotient is NaN.  A tile's best (NaN passed over, then value, then lowest
//               index) goes to a slab; the tiles' bests are folded per group by speccand_fold_kernel.  No atomics.
// Every slot's accumulator is independent of the others, so cutting the work by slot changes no bit, and a location of 12 960
// candidates fills the device with 51 x nmis workgroups.  Two consequences of the arithmetic:
//   - a unit candidate e_a gives v = s_a[i] exactly (the other products are +-0): its slot misfit is basis source a's own up to
//     the order of the fp64 sum;
//   - the answer does not depend on how the work is cut over workgroups, on chunking (KIWI_HIP_CHUNK_MB), on isrc0, on the piece
//     or on the number of devices.
// There is no free scale: under l1norm the best scale of a direction has no closed form; the moment axis is more candidates.
// Status of a group: 0 evaluated; 1 no receiver counts (the denominator of the fold is not positive): NaN, best_index -1; 2 a basis
// source failed to discretise (set on the host).

namespace waveform_candidates {

constexpr int kThreads = 256;                   // candidates per workgroup
constexpr int kStage = 256;                     // samples per LDS stage
constexpr int kMaxBasis = linfit::kMaxBasis;
// floats per sample in a stage: the K rows and the reference side, padded to whole 16-byte reads (12 KiB per stage at K = 8)
__host__ __device__ constexpr int row_floats(int K) { return (K + 1 + 3) / 4 * 4; }

using spectral_candidates::SlotInfo;

// proc: the kept rows (run_chunk); pairs: the chunk's (source, slot) records where transforms ran, else null; x: [ncand][K] fp32;
// ok: [group] 0 where a basis source failed to discretise; slab: [group][slot][ncand].
// blockIdx.x = tile of candidates, blockIdx.y = slot, blockIdx.z = group
template <int K, int METHOD>
__global__ __launch_bounds__(kThreads) void wavecand_slot_kernel(const float *__restrict__ proc, size_t syn_stride,
                                                                 const CompDev *__restrict__ comps, const float *__restrict__ reft,
                                                                 const float *__restrict__ reffilt, const FftPair *__restrict__ pairs,
                                                                 const int *__restrict__ ok, int nmis, float syn_factor, float dt,
                                                                 const float *__restrict__ x, int ncand, float *__restrict__ slab)
{
    constexpr int R = row_floats(K);
    __shared__ __attribute__((aligned(16))) float sS[kStage * R];
    const int tid = (int)threadIdx.x, m = (int)blockIdx.y, g = (int)blockIdx.z;
    if (!ok[g]) return;                                  // (workgroup-uniform)
    const int cand = (int)blockIdx.x * kThreads + tid;
    const bool live = cand < ncand;
    const bool unit = (syn_factor == 1.f);
    const CompDev cd = comps[m];
    const float *__restrict__ sy = proc + (size_t)g * K * syn_stride + cd.synofs + cd.halo;
    const float *__restrict__ dp = (cd.has_filter && pairs) ? reffilt + pairs[(size_t)g * K * nmis + m].filtofs : reft + cd.refofs;
    float xf[K];
#pragma unroll
    for (int a = 0; a < K; a++) xf[a] = live ? x[(size_t)cand * K + a] : 0.f;
    double acc = 0.0;
    for (int i0 = 0; i0 < cd.wlen; i0 += kStage) {
        const int nst = cd.wlen - i0 < kStage ? cd.wlen - i0 : kStage;
        __syncthreads();
        for (int i = tid; i < nst; i += kThreads) {      // (the rows are contiguous in i: coalesced loads)
#pragma unroll
            for (int a = 0; a < K; a++) sS[i * R + a] = sy[(size_t)a * syn_stride + i0 + i];
            sS[i * R + K] = dp[i0 + i];
        }
        __syncthreads();
#pragma unroll 4
        for (int j = 0; j < nst; j++) {
            float s[R];
#pragma unroll
            for (int q = 0; q < R; q += 4) {
                const float4 t = *reinterpret_cast<const float4 *>(sS + j * R + q);
                s[q] = t.x; s[q + 1] = t.y; s[q + 2] = t.z; s[q + 3] = t.w;
            }
            float v = xf[0] * s[0];
#pragma unroll
            for (int a = 1; a < K; a++) v = v + xf[a] * s[a];
            const float av = s[K];
            const float d = unit ? (av - v) : (1.f * av - syn_factor * v);
            if (METHOD == 1) acc = sq_acc(acc, d);
            else acc += (double)fabsf(d);
        }
    }
    const float mf = METHOD == 1 ? (float)sqrt((double)dt * acc) : (float)((double)dt * acc);
    if (live) slab[((size_t)g * nmis + m) * ncand + cand] = mf;
}

// slab: [group][slot][ncand]; norm: [group][slot]; ok: [group]; info: [slot]; w: [nrec] (0 for a disabled receiver).  misfit:
// [group][ncand] or null; smis: [group][ncand][nmis] or null; tile_v, tile_i: [group][gridDim.x]; status: [group].
// blockIdx.x = tile of candidates, blockIdx.y = group
__global__ __launch_bounds__(kThreads) void wavecand_fold_kernel(const float *__restrict__ slab, const float *__restrict__ norm,
                                                                 const int *__restrict__ ok, const SlotInfo *__restrict__ info,
                                                                 const double *__restrict__ w, int nmis, int l2, int anarchy, int ncand,
                                                                 double *__restrict__ misfit, float *__restrict__ smis,
                                                                 double *__restrict__ tile_v, int *__restrict__ tile_i,
                                                                 int *__restrict__ status)
{
    __shared__ double best_v[kThreads / 64];
    __shared__ int best_i[kThreads / 64];
    const int g = (int)blockIdx.y, tid = (int)threadIdx.x;
    const int cand = (int)blockIdx.x * kThreads + tid;
    const bool live = cand < ncand;
    const size_t cslot = (size_t)g * ncand + (live ? cand : 0);
    const double nan = __longlong_as_double(0x7ff8000000000000LL);
    const bool evaluated = nmis > 0 && ok[g] != 0;
    double ms = 0.0, ns = 0.0;                  // the fold's sums over the receivers
    double Mr = 0.0, Nr = 0.0;                  // the receiver being folded
    for (int m = 0; evaluated && m < nmis; m++) {
        const SlotInfo si = info[m];
        const float mf = slab[((size_t)g * nmis + m) * ncand + (live ? cand : 0)];
        if (smis && live) smis[cslot * nmis + m] = mf;
        const double mv = (double)mf, nv = (double)norm[(size_t)g * nmis + m];
        if (l2) { Mr = Mr + mv * mv; Nr = Nr + nv * nv; }
        else { Mr = Mr + mv; Nr = Nr + nv; }
        if (!si.last) continue;
        if (l2) { Mr = sqrt(Mr); Nr = sqrt(Nr); }
        double rw = w[si.rec];
        if (anarchy) {
            const double q = rw / (Nr != 0.0 ? Nr : -1.0);
            rw = (q > 0.0 || q != q) ? q : 0.0;
        }
        double av = Mr * rw, bv = Nr * rw;
        if (l2) { av = av * av; bv = bv * bv; }
        ms = ms + av * 1.0;
        ns = ns + bv * 1.0;
        Mr = 0.0; Nr = 0.0;
    }
    double mf = nan;
    if (evaluated && ns > 0.0) {
        mf = ms / ns;
        if (l2) mf = sqrt(mf);
        if (!(mf >= 0.0)) mf = nan;
    }
    if (live && misfit) misfit[cslot] = mf;
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

// host arrays of the caller for the groups of ONE call of run().  x [ncand][K], shared by all groups.  best_index, best_misfit,
// status [group]; the others may be null: misfit [group][ncand]; slot_misfit [group][ncand][nmis] and slot_norm [group][nmis] (both
// or neither: the pair kiwi_hip_outer_misfits takes)
struct Call {
    const double *x; int ncand, outer_norm;
    int *best_index; double *best_misfit; int *status;
    double *misfit;
    float *slot_misfit, *slot_norm;
    Call at(int g, int nmis) const
    {
        Call c = *this;
        c.best_index += g; c.best_misfit += g; c.status += g;
        if (misfit) c.misfit += (size_t)g * ncand;
        if (slot_misfit) c.slot_misfit += (size_t)g * ncand * nmis;
        if (slot_norm) c.slot_norm += (size_t)g * nmis;
        return c;
    }
};

// what the call cannot do is refused before anything runs, nothing approximated.  Leaves the context prepared
static void check_setup(kiwi_hip_ctx *c, int K, const Call &cl)
{
    if (K < 1 || K > kMaxBasis)
        throw std::runtime_error("waveform_candidates: K = " + std::to_string(K) + " basis sources per group; 1 to " + std::to_string(kMaxBasis) + " are supported");
    if (cl.ncand < 1) throw std::runtime_error("waveform_candidates: ncand = " + std::to_string(cl.ncand) + "; at least one candidate is needed");
    if (!cl.x || !cl.best_index || !cl.best_misfit || !cl.status)
        throw std::runtime_error("waveform_candidates: null candidates, best_index, best_misfit or status array");
    if (c->method != KIWI_L1NORM && c->method != KIWI_L2NORM)
        throw std::runtime_error("waveform_candidates: the misfit method must be l1norm or l2norm (floating_l2norm goes through "
                                 "linear_fit_candidates_floating, the ampspec norms through spectral_candidates)");
    if (cl.outer_norm != 1 && cl.outer_norm != 2) throw std::runtime_error("waveform_candidates: outer_norm must be 1 (l1norm) or 2 (l2norm)");
    if ((cl.slot_misfit == nullptr) != (cl.slot_norm == nullptr)) throw std::runtime_error("waveform_candidates: slot_misfit and slot_norm come together");
    for (size_t p = 0; p < (size_t)cl.ncand * K; p++)
        if (!std::isfinite(cl.x[p]))
            throw std::runtime_error("waveform_candidates: entry " + std::to_string(p % K) + " of candidate " + std::to_string(p / K) + " is not finite");
    prepare(c);
    if (c->synth_only) throw std::runtime_error("waveform_candidates: every enabled receiver component needs a reference seismogram");
    if (c->any_untapered)
        throw std::runtime_error("waveform_candidates: an enabled receiver has no misfit taper (its comparison span follows the source, so the basis traces have no common span)");
}

static void fill_failed(int ngroup, int nmis, const Call &cl)
{
    const double nan = std::numeric_limits<double>::quiet_NaN();
    for (int g = 0; g < ngroup; g++) { cl.status[g] = 2; cl.best_index[g] = -1; cl.best_misfit[g] = nan; }
    const size_t nc = (size_t)ngroup * cl.ncand;
    if (cl.misfit) std::fill(cl.misfit, cl.misfit + nc, nan);
    if (cl.slot_misfit) std::fill(cl.slot_misfit, cl.slot_misfit + nc * nmis, 0.f);
    if (cl.slot_norm) std::fill(cl.slot_norm, cl.slot_norm + (size_t)ngroup * nmis, 0.f);
}

struct Args {
    const FftPair *pairs; const int *ok; const float *x; int ng, ncand; float *slab;
};

template <int K>
static void launch(kiwi_hip_ctx *c, const Args &a)
{
    const int ntile = (a.ncand + kThreads - 1) / kThreads;
    const dim3 grid((unsigned)ntile, (unsigned)c->nmis, (unsigned)a.ng);
    if (c->method == KIWI_L2NORM)
        hipLaunchKernelGGL((wavecand_slot_kernel<K, 1>), grid, dim3(kThreads), 0, c->stream, c->proc_d.p, c->syn_stride, c->comps_d.p, c->reft_d.p,
                           c->reffilt_d.p, a.pairs, a.ok, c->nmis, c->syn_factor, c->gm.dt, a.x, a.ncand, a.slab);
    else
        hipLaunchKernelGGL((wavecand_slot_kernel<K, 2>), grid, dim3(kThreads), 0, c->stream, c->proc_d.p, c->syn_stride, c->comps_d.p, c->reft_d.p,
                           c->reffilt_d.p, a.pairs, a.ok, c->nmis, c->syn_factor, c->gm.dt, a.x, a.ncand, a.slab);
    HIPCHECK(hipGetLastError());
}

// the groups [isrc0, isrc0 + ngroup K) of the uploaded batch; adds its HIP-event times to c->wavecand_ms: evaluation (run_chunk),
// the slot kernel, the fold kernels, the downloads
static void run(kiwi_hip_ctx *c, int isrc0, int ngroup, int K, const double *receiver_weight, int anarchy, const Call &cl)
{
    check_setup(c, K, cl);
    check_group_range("waveform_candidates", c, isrc0, ngroup, K);
    if (ngroup == 0) return;
    const int nrec = (int)c->recv.size(), nmis = c->nmis;
    const LibraryTransforms library_transforms(c);      // (a misfit filter: the kept traces through the library transforms, as in linfit::run)
    c->misfit_d.ensure((size_t)c->nsrc * c->nmis, &c->dev_bytes);
    c->global_d.ensure((size_t)c->nsrc, &c->dev_bytes);
    if (c->fft_needed && !c->fft_ready) prepare_fft(c, c->reft_h);
    const int proc_which = c->any_filter ? 3 : 2;
    c->fuse_now = can_fuse(c, proc_which, isrc0, ngroup * K);
    if (c->fft_needed && c->fft_cap < K) throw std::runtime_error("waveform_candidates: the transform workspace (KIWI_HIP_CHUNK_MB) does not hold one group");

    const std::vector<double> w = receiver_weights(c, receiver_weight);
    std::vector<SlotInfo> info((size_t)nmis);
    for (int m = 0; m < nmis; m++)
        info[(size_t)m] = SlotInfo{ c->comps[(size_t)m].rec, (m + 1 == nmis || c->comps[(size_t)m + 1].rec != c->comps[(size_t)m].rec) ? 1 : 0,
                                    c->comps[(size_t)m].has_filter, 0 };
    std::vector<float> xf((size_t)cl.ncand * K);
    for (size_t p = 0; p < xf.size(); p++) xf[p] = (float)cl.x[p];
    const size_t ntile = (size_t)(cl.ncand + kThreads - 1) / kThreads;
    // device buffers of the call: kept on the context and grown only (no allocation, and so no device-wide wait, in a call whose
    // sizes the context has seen)
    auto &B = c->wavecand_bufs;
    constexpr size_t kInfoInts = sizeof(SlotInfo) / sizeof(int);
    B.w.ensure((size_t)std::max(nrec, 1), &c->dev_bytes);
    B.x.ensure(xf.size(), &c->dev_bytes);
    B.info.ensure((size_t)std::max(nmis, 1) * kInfoInts, &c->dev_bytes);
    // (w, info, xf and the tables of a chunk are read by these copies: nothing leaves this function, by return or by exception,
    // before the stream is drained)
    struct Drain { hipStream_t s; ~Drain() { (void)hipStreamSynchronize(s); } } drain{ c->stream };
    HIPCHECK(hipMemcpyAsync(B.w.p, w.data(), (size_t)nrec * sizeof(double), hipMemcpyHostToDevice, c->stream));
    HIPCHECK(hipMemcpyAsync(B.x.p, xf.data(), xf.size() * sizeof(float), hipMemcpyHostToDevice, c->stream));
    if (nmis > 0) HIPCHECK(hipMemcpyAsync(B.info.p, info.data(), (size_t)nmis * sizeof(SlotInfo), hipMemcpyHostToDevice, c->stream));

    const PooledEvents<6> ev(c);                           // (ev[5]: immediately in front of the slot kernel)
    std::vector<float> norm_h;
    std::vector<int> ok_h;
    // per group: the slab of slot misfits, the norm factors, the tiles' bests, the candidate outputs
    const size_t per_group = (size_t)nmis * cl.ncand * sizeof(float) + (size_t)nmis * sizeof(float) + sizeof(int) + ntile * (sizeof(double) + sizeof(int)) +
                             (size_t)cl.ncand * ((cl.misfit ? sizeof(double) : 0) + (cl.slot_misfit ? (size_t)nmis * sizeof(float) : 0));
    int g0 = 0;
    while (g0 < ngroup) {
        const int ng = next_group_chunk(c, isrc0, g0, ngroup, K, 2, per_group, c->fft_needed ? c->fft_cap : kNoSourceCap);       // (at most 65535 / K: a grid dimension)
        const int s0 = isrc0 + g0 * K;
        HIPCHECK(hipEventRecord(ev[0], c->stream));
        run_chunk(c, s0, ng * K, proc_which);
        HIPCHECK(hipEventRecord(ev[1], c->stream));
        // the norm factors of the chunk's slots and which of its groups are evaluated at all
        norm_h.assign((size_t)ng * nmis, 0.f);
        ok_h.assign((size_t)ng, 1);
        for (int g = 0; g < ng; g++) {
            for (int i = 0; i < K; i++) if (c->src_status[(size_t)s0 + (size_t)g * K + i]) ok_h[(size_t)g] = 0;
            if (!ok_h[(size_t)g]) continue;
            for (int m = 0; m < nmis; m++)
                norm_h[(size_t)g * nmis + m] = c->fft_needed ? c->norm_src_h[((size_t)s0 + (size_t)g * K) * nmis + m] : c->norm_h[(size_t)m];
        }
        const size_t nc = (size_t)ng * cl.ncand;
        B.slab.ensure(std::max<size_t>(1, nc * nmis), &c->dev_bytes);
        B.norm.ensure(std::max<size_t>(1, norm_h.size()), &c->dev_bytes);
        B.ok.ensure((size_t)ng, &c->dev_bytes);
        B.tile_v.ensure((size_t)ng * ntile, &c->dev_bytes); B.tile_i.ensure((size_t)ng * ntile, &c->dev_bytes);
        B.best_index.ensure((size_t)ng, &c->dev_bytes); B.best_misfit.ensure((size_t)ng, &c->dev_bytes); B.status.ensure((size_t)ng, &c->dev_bytes);
        if (cl.misfit) B.misfit.ensure(nc, &c->dev_bytes);
        if (cl.slot_misfit) B.smis.ensure(std::max<size_t>(1, nc * nmis), &c->dev_bytes);
        if (!norm_h.empty()) HIPCHECK(hipMemcpyAsync(B.norm.p, norm_h.data(), norm_h.size() * sizeof(float), hipMemcpyHostToDevice, c->stream));
        HIPCHECK(hipMemcpyAsync(B.ok.p, ok_h.data(), ok_h.size() * sizeof(int), hipMemcpyHostToDevice, c->stream));
        if (cl.slot_misfit && nmis > 0) HIPCHECK(hipMemsetAsync(B.smis.p, 0, nc * nmis * sizeof(float), c->stream));
        HIPCHECK(hipEventRecord(ev[5], c->stream));
        if (nmis > 0) {
            const Args a{ c->fft_needed ? c->pairs_d.p : (const FftPair *)nullptr, B.ok.p, B.x.p, ng, cl.ncand, B.slab.p };
            by_basis(K, [&](auto k) { launch<k.value>(c, a); });
        }
        HIPCHECK(hipEventRecord(ev[2], c->stream));
        hipLaunchKernelGGL(wavecand_fold_kernel, dim3((unsigned)ntile, (unsigned)ng), dim3(kThreads), 0, c->stream, B.slab.p, B.norm.p, B.ok.p,
                           (const SlotInfo *)B.info.p, B.w.p, nmis, cl.outer_norm == 2 ? 1 : 0, anarchy ? 1 : 0, cl.ncand,
                           cl.misfit ? B.misfit.p : (double *)nullptr, cl.slot_misfit ? B.smis.p : (float *)nullptr, B.tile_v.p, B.tile_i.p, B.status.p);
        HIPCHECK(hipGetLastError());
        hipLaunchKernelGGL(spectral_candidates::speccand_fold_kernel, dim3((unsigned)ng), dim3(64), 0, c->stream, B.tile_v.p, B.tile_i.p, (int)ntile,
                           B.best_index.p, B.best_misfit.p);
        HIPCHECK(hipGetLastError());
        HIPCHECK(hipEventRecord(ev[3], c->stream));
        const Call o = cl.at(g0, nmis);
        HIPCHECK(hipMemcpyAsync(o.best_index, B.best_index.p, (size_t)ng * sizeof(int), hipMemcpyDeviceToHost, c->stream));
        HIPCHECK(hipMemcpyAsync(o.best_misfit, B.best_misfit.p, (size_t)ng * sizeof(double), hipMemcpyDeviceToHost, c->stream));
        HIPCHECK(hipMemcpyAsync(o.status, B.status.p, (size_t)ng * sizeof(int), hipMemcpyDeviceToHost, c->stream));
        if (cl.misfit) HIPCHECK(hipMemcpyAsync(o.misfit, B.misfit.p, nc * sizeof(double), hipMemcpyDeviceToHost, c->stream));
        if (cl.slot_misfit && nmis > 0) HIPCHECK(hipMemcpyAsync(o.slot_misfit, B.smis.p, nc * nmis * sizeof(float), hipMemcpyDeviceToHost, c->stream));
        HIPCHECK(hipEventRecord(ev[4], c->stream));
        HIPCHECK(hipStreamSynchronize(c->stream));
        if (o.slot_norm) std::copy(norm_h.begin(), norm_h.end(), o.slot_norm);
        // (the host's tables of the chunk and their upload lie between ev[1] and ev[5]: in none of the four)
        ev.add_elapsed(c->wavecand_ms, 0, 0, 1);
        ev.add_elapsed(c->wavecand_ms, 1, 5, 2);
        ev.add_elapsed(c->wavecand_ms, 2, 2, 3);
        ev.add_elapsed(c->wavecand_ms, 3, 3, 4);
        g0 += ng;
    }
    leave_evaluated(c, isrc0, ngroup * K, proc_which);
    for_each_failed_group(c, isrc0, ngroup, K, [&](int g) { fill_failed(1, nmis, cl.at(g, nmis)); });
}

// kiwi_hip_waveform_candidates_params piece by piece (PieceCall, kiwi_group_run.hpp)
static PieceCall piece_call(int K, const double *receiver_weight, int anarchy, const Call &cl)
{
    return PieceCall{ K,
        [=](kiwi_hip_ctx *c) { check_setup(c, K, cl); },
        [=](kiwi_hip_ctx *c, int s0, int n) { fill_failed(n / K, c->nmis, cl.at(s0 / K, c->nmis)); },
        [=](kiwi_hip_ctx *c, int s0, int n) { run(c, 0, n / K, K, receiver_weight, anarchy, cl.at(s0 / K, c->nmis)); } };
}

} // namespace waveform_candidates
