// kiwi_spectral_candidates_bootstrap.hpp -- the bootstrap over the receivers of a candidate search under the amplitude-spectrum norms
// (ampspec_l2norm, ampspec_l1norm), joint over group (location) and candidate (mechanism), without the [candidate][slot] array ever
// leaving the device: kiwi_hip_spectral_candidates_bootstrap.  What it answers is DEFINED by two existing calls:
// kiwi_hip_spectral_candidates (free_scale 0) writes slot_misfit [ngroup][ncand][nmis] and slot_norm [ngroup][nmis] as floats,
// kiwi_hip_outer_misfits reads them as ngroup ncand sources of nmis slots (slot m belongs to receiver slot_receiver[m]; the norm row
// of group g repeated for each of its sources) and returns the best source of every draw.  Included by kiwi_hip.hip behind
// kiwi_waveform_candidates_bootstrap.hpp under the same -ffp-contract=off: every fp32 and fp64 operation below is rounded on its own;
// tests/spectral_candidates_bootstrap_restatement.py composes tests/spectral_candidates_restatement.py's slot arrays with
// tests/outer_restatement.py, and the GPU tests ask for bit identity with the host route.  Per chunk of whole groups, behind the
// unchanged evaluation and speccand_spectra_kernel of spectral_candidates::run (its ChunkHook; speccand_kernel is not launched):
//   speccand_slot_kernel<K>   one workgroup of kThreads lanes per (tile of kThreads candidates, slot, group), a lane owns ONE
//       candidate with xf = (float) x in registers.  The slot's kept bins klo .. khi of spec, refamp and filtw are staged in LDS,
//       kStage bins at a time, and read as broadcasts; bins ascend into ONE fp64 accumulator.  The expression sequence is
//       speccand_kernel<K, false>'s per slot, operation for operation: re, im from a = 0 ascending; b = amp_rn(re, im); b = b fw[k]
//       where the receiver has a filter; d = unit ? a - b : 1.f a - syn_factor b; acc = sq_acc(acc, d) | acc += (double) fabsf(d);
//       m = (float) sqrt((double) df acc) | (float) ((double) df acc) to slab[group][slot][candidate] -- a wavefront stores 64
//       consecutive floats.  A slot without kept bins writes 0; the slots of a group that is not evaluated (ntrans == 0: a basis
//       source failed to discretise) are not written, the bootstrap kernel's `failed` flag covers them.  Where speccand_kernel walks
//       the slots of a location one behind the other in ONE workgroup per tile, this grid has nmis times as many: 51 x 150 instead of
//       51 workgroups for 12 960 candidates at one location.  Static LDS 128 (8 K + 8) bytes, 9 KiB at K = 8: eight workgroups of
//       four waves fill a CU's 32 wave slots in 72 of its 160 KiB, so the stage does not bound the occupancy; a longer one would
//       save barriers only for slots of more than 128 kept bins.  No atomics, zero scratch
//       (profiles/spectral_candidates_bootstrap_kernel_resources.json).
//   wavecand_bootstrap_prepare_kernel, wavecand_bootstrap_kernel   kiwi_waveform_candidates_bootstrap.hpp's, unchanged, with
//       nk = 1: the norm side from the chunk's slot norms (SlotRec::norm) as a float [group][nmis] array, then the slab folded per
//       receiver and the draw walk; the fold kernels and the run's arrays of kiwi_candidates_bootstrap.hpp behind, through the
//       waveform sibling's Hook.
//   speccand_boot_status_kernel   one thread per group: ns = 0; ns = ns + b_r 1.0, r ascending, with the prepare kernel's b -- the
//       denominator of speccand_kernel's fold --; status 0 where ns > 0, else 1.  The host sets 2 for a failed group.
// A draw with every source excluded: NaN, -1, -1 -- the one difference from the host route, which answers NaN and index 0.  There are
// no origin times: Boot's offset arrays are null.  The receiver limit is the waveform sibling's kMaxRec.

namespace spectral_candidates_bootstrap {

using candidates_bootstrap::Boot;
using spectral_candidates::kThreads;
using spectral_candidates::kStage;
using spectral_candidates::SlotRec;
using spectral_candidates::SlotInfo;
using spectral_candidates::amp_rn;
using waveform_candidates_bootstrap::kMaxRec;

static const char *const kName = "spectral_candidates_bootstrap";

// spec: the chunk's rows; slots: [group][nmis]; info: [nmis]; x: [ncand][K] fp32; slab: [group][nmis][ncand].
// blockIdx.x = tile of candidates, blockIdx.y = slot, blockIdx.z = group
template <int K>
__global__ __launch_bounds__(kThreads) void speccand_slot_kernel(const float2 *__restrict__ spec, const SlotRec *__restrict__ slots,
                                                                 const SlotInfo *__restrict__ info, const float *__restrict__ refamp,
                                                                 const float *__restrict__ filtw, int nmis, int method, float syn_factor,
                                                                 const float *__restrict__ x, int ncand, float *__restrict__ slab)
{
    __shared__ float2 sS[kStage * K];
    __shared__ float sA[kStage], sF[kStage];
    const int tid = (int)threadIdx.x, m = (int)blockIdx.y, g = (int)blockIdx.z;
    const SlotRec sl = slots[(size_t)g * nmis + m];
    if (sl.ntrans == 0) return;                             // (workgroup-uniform)
    const int has_filter = info[m].has_filter;
    const int cand = (int)blockIdx.x * kThreads + tid;
    const bool live = cand < ncand;
    const bool unit = (syn_factor == 1.f);
    float xf[K];
#pragma unroll
    for (int a = 0; a < K; a++) xf[a] = live ? x[(size_t)cand * K + a] : 0.f;
    const int nb = sl.khi - sl.klo + 1;
    double acc = 0.0;
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
            if (has_filter) b = b * sF[j];
            const float av = sA[j];
            const float d = unit ? (av - b) : (1.f * av - syn_factor * b);
            if (method == 3) acc = sq_acc(acc, d);
            else acc += (double)fabsf(d);
        }
    }
    const float mf = method == 3 ? (float)sqrt((double)sl.df * acc) : (float)((double)sl.df * acc);
    if (live) slab[((size_t)g * nmis + m) * ncand + cand] = mf;
}

// b: [group][nrec], the prepare kernel's.  One thread per group
__global__ __launch_bounds__(256) void speccand_boot_status_kernel(const double *__restrict__ b, int nrec, int ng, int *__restrict__ status)
{
    const int g = (int)(blockIdx.x * 256 + threadIdx.x);
    if (g >= ng) return;
    double ns = 0.0;
    for (int r = 0; r < nrec; r++) ns = ns + b[(size_t)g * nrec + r] * 1.0;
    status[g] = ns > 0.0 ? 0 : 1;
}

// the parent's arrays that the caller of the bootstrap does not see: best_index, best_misfit [group]
struct ParentArrays {
    std::vector<int> best_index; std::vector<double> best_misfit;
    explicit ParentArrays(size_t ngroup) : best_index(ngroup, -1), best_misfit(ngroup, 0.0) {}
};
static spectral_candidates::Call parent_call(const Boot &bt, int *best_index, double *best_misfit)
{
    return spectral_candidates::Call{ bt.x, bt.ncand, bt.outer_norm, 0, best_index, best_misfit, bt.status, nullptr, nullptr, nullptr, nullptr,
                                      0, nullptr, nullptr, nullptr };
}

// what the call cannot do is refused before anything runs: everything kiwi_hip_spectral_candidates refuses of the set-up, and what
// the draws add
static void check_setup(kiwi_hip_ctx *c, int K, const double *receiver_weight, const Boot &bt)
{
    candidates_bootstrap::check_draws(kName, c, candidates_bootstrap::Extra::none, kMaxRec, receiver_weight, bt, [&] {
        int idummy = 0; double ddummy = 0.0;               // (the parent's arrays: checked for null only)
        spectral_candidates::check_setup(c, K, parent_call(bt, &idummy, &ddummy));
    });
}

// the slot kernel and the bootstrap kernels of one chunk of the parent's run; the bootstrap side is the waveform sibling's Hook
struct Hook : spectral_candidates::ChunkHook {
    kiwi_hip_ctx *c; int K;
    waveform_candidates_bootstrap::Hook wb;
    std::vector<float> norm_h;
    DevBuf<float> slab_d, norm_d;
    Hook(kiwi_hip_ctx *ctx, const Boot &bt, int isrc0, int k, int anarchy) : c(ctx), K(k), wb(ctx, bt, isrc0, k, 1, anarchy)
    {
        // per group: the slab of slot misfits and the norm row, and what the waveform hook counts
        per_group = (size_t)bt.ncand * wb.nmis * sizeof(float) + (size_t)wb.nmis * sizeof(float) + wb.per_group;
    }

    void candidates(int ng, const float2 *spec, const SlotRec *slots, const SlotInfo *info, const float *x) override
    {
        const int nmis = wb.nmis, ncand = wb.st.bt.ncand;
        slab_d.ensure(std::max<size_t>(1, (size_t)ng * nmis * ncand), &c->dev_bytes);
        if (nmis == 0) return;
        const dim3 grid((unsigned)wb.st.ntile, (unsigned)nmis, (unsigned)ng);
        by_basis(K, [&](auto k) {
            hipLaunchKernelGGL((speccand_slot_kernel<k.value>), grid, dim3(kThreads), 0, c->stream, spec, slots, info, c->refamp_d.p, c->filtw_d.p,
                               nmis, c->method, c->syn_factor, x, ncand, slab_d.p);
        });
        HIPCHECK(hipGetLastError());
    }

    void after_candidates(int g0, int ng, const std::vector<SlotRec> &sl, int *status) override
    {
        // (norm_h is read by this copy; the parent drains the stream at the end of the chunk, before the next call of this function)
        norm_h.resize(sl.size());
        for (size_t i = 0; i < sl.size(); i++) norm_h[i] = sl[i].norm;
        norm_d.ensure(std::max<size_t>(1, norm_h.size()), &c->dev_bytes);
        if (!norm_h.empty()) HIPCHECK(hipMemcpyAsync(norm_d.p, norm_h.data(), norm_h.size() * sizeof(float), hipMemcpyHostToDevice, c->stream));
        wb.after_fold(g0, ng, slab_d.p, norm_d.p);
        hipLaunchKernelGGL(speccand_boot_status_kernel, dim3((unsigned)((ng + 255) / 256)), dim3(256), 0, c->stream, wb.st.b.p, wb.st.nrec, ng, status);
        HIPCHECK(hipGetLastError());
    }
};

// the groups [isrc0, isrc0 + ngroup K) of the uploaded batch: spectral_candidates::run's chunk loop with the slot kernel in the place
// of its candidate kernels and the bootstrap kernels behind.  Adds its HIP-event times to c->speccand_boot_ms
static void run(kiwi_hip_ctx *c, int isrc0, int ngroup, int K, const double *receiver_weight, int anarchy, const Boot &bt)
{
    check_setup(c, K, receiver_weight, bt);
    check_group_range(kName, c, isrc0, ngroup, K);
    if (ngroup == 0) return;
    if (c->nmis > 65535) throw std::runtime_error(std::string(kName) + ": " + std::to_string(c->nmis) + " misfit slots exceed a launch");

    Hook h(c, bt, isrc0, K, anarchy);
    float boot_ms = 0.f;
    h.ms = &boot_ms;
    h.wb.begin(receiver_weight);

    float parent_ms[4];
    std::copy(c->speccand_ms, c->speccand_ms + 4, parent_ms);
    ParentArrays pa((size_t)ngroup);
    refusing(kName, [&] {
        spectral_candidates::run(c, isrc0, ngroup, K, receiver_weight, anarchy, parent_call(bt, pa.best_index.data(), pa.best_misfit.data()), &h);
    });
    for (int i = 0; i < 3; i++) c->speccand_boot_ms[i] += c->speccand_ms[i] - parent_ms[i];
    c->speccand_boot_ms[3] += boot_ms;
    c->speccand_boot_ms[4] += c->speccand_ms[3] - parent_ms[3];
    h.wb.st.finish(c->speccand_boot_ms + 4);
}

// kiwi_hip_spectral_candidates_bootstrap_params piece by piece
static PieceCall piece_call(int K, const double *receiver_weight, int anarchy, const Boot &bt)
{
    return candidates_bootstrap::piece_call(K, bt,
        [=](kiwi_hip_ctx *c, const Boot &b) { check_setup(c, K, receiver_weight, b); },
        [=](kiwi_hip_ctx *c, int ng, const Boot &b) { run(c, 0, ng, K, receiver_weight, anarchy, b); });
}

} // namespace spectral_candidates_bootstrap
