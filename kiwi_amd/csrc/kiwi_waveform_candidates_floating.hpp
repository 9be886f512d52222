// kiwi_waveform_candidates_floating.hpp -- misfits of many GIVEN coefficient vectors per group under floating_l1norm (the point of
// the call) and floating_l2norm: kiwi_waveform_candidates.hpp with every receiver sliding its reference under the fixed taper by
// whole samples inside its own range (kiwi_hip_set_floating_shiftrange, receiver.f90:439-510).  The reference DATA move and the taper
// stays with the synthetic, so a candidate's combined trace v[i] = sum_a x_a s_a[i] is the same for every shift: it is formed once
// per sample and pass, and a further shift costs a subtraction, a |.| and one fp64 add.  Included by kiwi_hip.hip behind
// kiwi_waveform_candidates.hpp under the same -ffp-contract=off: every fp32 and fp64 operation below is rounded on its own, and
// tests/waveform_candidates_floating_restatement.py restates each in the same order (the GPU tests ask for bit identity of the
// kernels with that restatement fed with the device's own kept traces).
//
// Sources [isrc0, isrc0 + ngroup K) are ngroup groups of K <= 8 consecutive basis sources.  Per chunk of whole groups:
//   evaluate    run_chunk under the floating method with the tapered synthetics kept in proc_d (proc_which 2; the context refuses a
//               misfit filter under a floating norm): misfits, shifts and global misfits of the basis sources are left exactly as
//               kiwi_hip_eval leaves them
//   slots       wavecand_float_kernel<K, METHOD> (METHOD 1 l2 inside, 2 l1 inside), one workgroup of kThreads lanes per (tile of
//               kThreads candidates, enabled receiver, group); a lane owns ONE candidate with xf = (float) x in registers.  Shift
//               index q = 0 .. fl_ns - 1 (shift fl_lo + q) is walked in passes of J = shifts_per_pass(K).  Inside a pass the
//               receiver's slots k ascending, kStage samples at a time in LDS: a staged sample carries the K kept rows and the J
//               tapered, shifted reference values, formed by the staging threads as floating_norm_kernel forms them,
//                   a_q[i] = refx[refxofs + i + (fl_ns - 1 - q)] * tw[refofs + i]                      (fp32 product)
//               side by side, read by the lanes as 16-byte broadcasts.  Per sample, i = 0 .. wlen - 1 ascending:
//                   v = xf_0 s_0[i]; v = v + xf_a s_a[i] (a ascending, fp32)                           (once per pass)
//                   d = unit ? a_q[i] - v : 1.f a_q[i] - syn_factor v
//                   l2: acc_kq = sq_acc(acc_kq, d)  |  l1: acc_kq += (double) fabsf(d)                 (ONE fp64 accumulator per shift)
//               m_kq = (float) sqrt((double) dt acc_kq) | (float) ((double) dt acc_kq);  sum_q = fp32, k ascending from 0.f:
//               sum_q = sum_q + (l1 ? m_kq : m_kq m_kq) -- floating_select_kernel's -- and the FIRST minimum wins:
//               q == 0 || sum_q < best.  After a pass the lane updates its running (best, q*, m_{k,q*}); only the winner goes to
//               memory: slab[group][slot][cand] = m_{k,q*} (float) and shift[group][receiver][cand] = q* (short: the INDEX, at most
//               kMaxFloatShifts - 1, so that a range far from zero still fits; fl_lo is added where it leaves the device).
//   fold        wavecand_fold_kernel and speccand_fold_kernel unchanged on that slab, with the context's floating norm factors (the
//               mean over the shifts of the shifted reference's norm, prepare(); every group's are those of its first source);
//               wavecand_float_shift_kernel gathers the winner's shifts into best_shift[group][nrec] (0 for a receiver that is
//               disabled or where no candidate won) and, on request, turns the shift slab into cand_shift[group][cand][nrec].
// No atomics, zero scratch (profiles/waveform_candidates_floating_kernel_resources.json).  An accumulator's value does not depend on
// the pass its shift falls into, on the tile, on chunking (KIWI_HIP_CHUNK_MB), on isrc0, on the piece or on the device count; with
// every range (0, 0) the slab is wavecand_slot_kernel's bit for bit (a_0[i] is then the tapered reference).
// Unlike kiwi_linfit_candidates_floating.hpp (receiver-level norm factor and fold) this is the reference's per-slot form under
// floating_l2norm as well.  There is no free scale.
// Status of a group: 0 evaluated; 1 no receiver counts: NaN, best_index -1; 2 a basis source failed to discretise (host).

namespace waveform_candidates_floating {

using waveform_candidates::kMaxBasis;
using waveform_candidates::kStage;
using waveform_candidates::kThreads;
using spectral_candidates::SlotInfo;

// floats per staged sample: the K rows and the J shifted references in whole 16-byte reads (16 KiB per stage at K = 8).  J is what
// fills the row that K + 8 needs: 8 to 11 shifts; per lane 2 J registers of accumulators, J sums and kMaxComp J kept misfits, no scratch
__host__ __device__ constexpr int row_floats(int K) { return (K + 8 + 3) / 4 * 4; }
__host__ __device__ constexpr int shifts_per_pass(int K) { return row_floats(K) - K; }

// proc: the kept rows (run_chunk); x: [ncand][K] fp32; ok: [group] 0 where a basis source failed to discretise; slab:
// [group][slot][ncand]; shift: [group][receiver][ncand].  blockIdx.x = tile of candidates, blockIdx.y = receiver, blockIdx.z = group
template <int K, int METHOD>
__global__ __launch_bounds__(kThreads) void wavecand_float_kernel(const float *__restrict__ proc, size_t syn_stride,
                                                                  const RecvDev *__restrict__ recv, const CompDev *__restrict__ comps,
                                                                  const float *__restrict__ refx, const float *__restrict__ tw,
                                                                  const int *__restrict__ ok, int nrec, int nmis, float syn_factor,
                                                                  float dt, const float *__restrict__ x, int ncand,
                                                                  float *__restrict__ slab, short *__restrict__ shift)
{
    constexpr int R = row_floats(K), J = shifts_per_pass(K);
    static_assert(kStage == kThreads, "a staging thread forms one sample of a stage");
    __shared__ __attribute__((aligned(16))) float sS[kStage * R];
    const int tid = (int)threadIdx.x, r = (int)blockIdx.y, g = (int)blockIdx.z;
    if (!ok[g]) return;                                  // (workgroup-uniform, as every branch on rd, cd, q0 and nj below)
    const RecvDev rd = recv[r];
    if (!rd.enabled) return;
    const int cand = (int)blockIdx.x * kThreads + tid;
    const bool live = cand < ncand;
    const bool unit = (syn_factor == 1.f);
    const int ns = comps[rd.slot0].fl_ns;
    const float *__restrict__ src0 = proc + (size_t)g * K * syn_stride;
    float xf[K];
#pragma unroll
    for (int a = 0; a < K; a++) xf[a] = live ? x[(size_t)cand * K + a] : 0.f;
    float best = 0.f, bm[kMaxComp];
    int qb = 0;
#pragma unroll
    for (int k = 0; k < kMaxComp; k++) bm[k] = 0.f;
    for (int q0 = 0; q0 < ns; q0 += J) {
        const int nj = ns - q0 < J ? ns - q0 : J;
        float sum[J], pm[kMaxComp][J];
#pragma unroll
        for (int j = 0; j < J; j++) sum[j] = 0.f;
#pragma unroll
        for (int k = 0; k < kMaxComp; k++) {             // (unrolled: pm is indexed by constants only)
            if (k < rd.ncomp) {
                const CompDev cd = comps[rd.slot0 + k];
                const float *__restrict__ sy = src0 + cd.synofs + cd.halo;
                // shift index q0 + j reads rq[i - j]: indices i + (fl_ns - 1 - q0 - j) in [0, wlen + fl_ns - 2] for j < nj
                const float *__restrict__ rq = refx + cd.refxofs + (cd.fl_ns - 1 - q0);
                const float *__restrict__ tp = tw + cd.refofs;
                double acc[J];
#pragma unroll
                for (int j = 0; j < J; j++) acc[j] = 0.0;
                for (int i0 = 0; i0 < cd.wlen; i0 += kStage) {
                    const int nst = cd.wlen - i0 < kStage ? cd.wlen - i0 : kStage;
                    __syncthreads();                     // the stage before this one has been read by every wavefront
                    if (tid < nst) {                     // (the rows are contiguous in i: coalesced loads)
                        const int i = i0 + tid;
                        float t[R];
#pragma unroll
                        for (int a = 0; a < K; a++) t[a] = sy[(size_t)a * syn_stride + i];
                        const float tv = tp[i];
#pragma unroll
                        for (int j = 0; j < J; j++) t[K + j] = j < nj ? rq[i - j] * tv : 0.f;      // make_array_tapered on the moved data
#pragma unroll
                        for (int p = 0; p < R; p += 4)
                            *reinterpret_cast<float4 *>(sS + tid * R + p) = make_float4(t[p], t[p + 1], t[p + 2], t[p + 3]);
                    }
                    __syncthreads();
#pragma unroll 2
                    for (int n = 0; n < nst; n++) {
                        float s[R];
#pragma unroll
                        for (int p = 0; p < R; p += 4) {
                            const float4 t = *reinterpret_cast<const float4 *>(sS + n * R + p);
                            s[p] = t.x; s[p + 1] = t.y; s[p + 2] = t.z; s[p + 3] = t.w;
                        }
                        float v = xf[0] * s[0];
#pragma unroll
                        for (int a = 1; a < K; a++) v = v + xf[a] * s[a];
                        const float sv = syn_factor * v;
#pragma unroll
                        for (int j = 0; j < J; j++) {
                            const float av = s[K + j];
                            const float d = unit ? (av - v) : (1.f * av - sv);
                            if (METHOD == 1) acc[j] = sq_acc(acc[j], d);
                            else acc[j] += (double)fabsf(d);
                        }
                    }
                }
#pragma unroll
                for (int j = 0; j < J; j++) {
                    const float mf = METHOD == 1 ? (float)sqrt((double)dt * acc[j]) : (float)((double)dt * acc[j]);
                    pm[k][j] = mf;
                    sum[j] = sum[j] + (METHOD == 2 ? mf : mf * mf);
                }
            } else {
#pragma unroll
                for (int j = 0; j < J; j++) pm[k][j] = 0.f;
            }
        }
#pragma unroll
        for (int j = 0; j < J; j++)
            if (j < nj && (q0 + j == 0 || sum[j] < best)) {
                best = sum[j]; qb = q0 + j;
#pragma unroll
                for (int k = 0; k < kMaxComp; k++) bm[k] = pm[k][j];
            }
    }
    if (!live) return;
#pragma unroll
    for (int k = 0; k < kMaxComp; k++)
        if (k < rd.ncomp) slab[((size_t)g * nmis + rd.slot0 + k) * ncand + cand] = bm[k];
    shift[((size_t)g * nrec + r) * ncand + cand] = (short)qb;
}

// shift: [group][receiver][ncand] (indices); best_index: [group]; best_shift: [group][nrec]; cshift: [group][ncand][nrec] or null.
// blockIdx.y = group.  The LAST block of a group gathers the winner's shifts, a receiver per thread; with cshift the blocks in front
// of it turn the shift slab into the caller's layout, a candidate per thread
__global__ __launch_bounds__(kThreads) void wavecand_float_shift_kernel(const short *__restrict__ shift, const RecvDev *__restrict__ recv,
                                                                        const CompDev *__restrict__ comps, const int *__restrict__ ok,
                                                                        const int *__restrict__ best_index, int nrec, int ncand,
                                                                        int *__restrict__ best_shift, short *__restrict__ cshift)
{
    const int g = (int)blockIdx.y, tid = (int)threadIdx.x;
    const short *__restrict__ sg = shift + (size_t)g * nrec * ncand;
    if (blockIdx.x + 1 == gridDim.x) {
        const int bi = ok[g] ? best_index[g] : -1;
        for (int r = tid; r < nrec; r += kThreads)
            best_shift[(size_t)g * nrec + r] = (recv[r].enabled && bi >= 0) ? comps[recv[r].slot0].fl_lo + (int)sg[(size_t)r * ncand + bi] : 0;
        return;
    }
    const int cand = (int)blockIdx.x * kThreads + tid;
    if (cand >= ncand) return;
    for (int r = 0; r < nrec; r++)
        cshift[((size_t)g * ncand + cand) * nrec + r] =
            (recv[r].enabled && ok[g]) ? (short)(comps[recv[r].slot0].fl_lo + (int)sg[(size_t)r * ncand + cand]) : (short)0;
}

// host arrays of the caller for the groups of ONE call of run().  x [ncand][K], shared by all groups.  best_index, best_misfit,
// status [group]; best_shift [group][nrec]; the others may be null: misfit [group][ncand]; cand_shift [group][ncand][nrec] (with
// misfit); slot_misfit [group][ncand][nmis] and slot_norm [group][nmis] (both or neither: the pair kiwi_hip_outer_misfits takes)
struct Call {
    const double *x; int ncand, outer_norm;
    int *best_index; double *best_misfit; int *status; int *best_shift;
    double *misfit; short *cand_shift;
    float *slot_misfit, *slot_norm;
    Call at(int g, int nmis, int nrec) const
    {
        Call c = *this;
        c.best_index += g; c.best_misfit += g; c.status += g; c.best_shift += (size_t)g * nrec;
        if (misfit) c.misfit += (size_t)g * ncand;
        if (cand_shift) c.cand_shift += (size_t)g * ncand * nrec;
        if (slot_misfit) c.slot_misfit += (size_t)g * ncand * nmis;
        if (slot_norm) c.slot_norm += (size_t)g * nmis;
        return c;
    }
};

// what the call cannot do is refused before anything runs, nothing approximated.  Leaves the context prepared
static void check_setup(kiwi_hip_ctx *c, int K, const Call &cl)
{
    const std::string name = "waveform_candidates_floating: ";
    if (K < 1 || K > kMaxBasis)
        throw std::runtime_error(name + "K = " + std::to_string(K) + " basis sources per group; 1 to " + std::to_string(kMaxBasis) + " are supported");
    if (cl.ncand < 1) throw std::runtime_error(name + "ncand = " + std::to_string(cl.ncand) + "; at least one candidate is needed");
    if (!cl.x || !cl.best_index || !cl.best_misfit || !cl.status || !cl.best_shift)
        throw std::runtime_error(name + "null candidates, best_index, best_misfit, status or best_shift array");
    if (c->method != KIWI_FLOATING_L1NORM && c->method != KIWI_FLOATING_L2NORM)
        throw std::runtime_error(name + "the misfit method must be floating_l1norm or floating_l2norm (l1norm and l2norm go through "
                                        "kiwi_hip_waveform_candidates)");
    if (cl.outer_norm != 1 && cl.outer_norm != 2) throw std::runtime_error(name + "outer_norm must be 1 (l1norm) or 2 (l2norm)");
    if ((cl.slot_misfit == nullptr) != (cl.slot_norm == nullptr)) throw std::runtime_error(name + "slot_misfit and slot_norm come together");
    if (cl.cand_shift && !cl.misfit) throw std::runtime_error(name + "a cand_shift array without a misfit array");
    for (size_t p = 0; p < (size_t)cl.ncand * K; p++)
        if (!std::isfinite(cl.x[p]))
            throw std::runtime_error(name + "entry " + std::to_string(p % K) + " of candidate " + std::to_string(p / K) + " is not finite");
    prepare(c);
    if (c->synth_only) throw std::runtime_error(name + "every enabled receiver component needs a reference seismogram");
    if (c->any_untapered)
        throw std::runtime_error(name + "an enabled receiver has no misfit taper (its comparison span follows the source, so the basis traces have no common span)");
    if (cl.cand_shift)
        for (const auto &r : c->recv)
            if (r.enabled && r.ncomp > 0 && (r.float_lo < -32768 || r.float_hi > 32767))
                throw std::runtime_error(name + "a shift range beyond 16 bits does not fit the cand_shift array");
}

static void fill_failed(int ngroup, int nmis, int nrec, const Call &cl)
{
    const double nan = std::numeric_limits<double>::quiet_NaN();
    for (int g = 0; g < ngroup; g++) { cl.status[g] = 2; cl.best_index[g] = -1; cl.best_misfit[g] = nan; }
    std::fill(cl.best_shift, cl.best_shift + (size_t)ngroup * nrec, 0);
    const size_t nc = (size_t)ngroup * cl.ncand;
    if (cl.misfit) std::fill(cl.misfit, cl.misfit + nc, nan);
    if (cl.cand_shift) std::fill(cl.cand_shift, cl.cand_shift + nc * nrec, (short)0);
    if (cl.slot_misfit) std::fill(cl.slot_misfit, cl.slot_misfit + nc * nmis, 0.f);
    if (cl.slot_norm) std::fill(cl.slot_norm, cl.slot_norm + (size_t)ngroup * nmis, 0.f);
}

struct Args {
    const int *ok; const float *x; int ng, ncand; float *slab; short *shift;
};

template <int K>
static void launch(kiwi_hip_ctx *c, const Args &a)
{
    const int ntile = (a.ncand + kThreads - 1) / kThreads, nrec = (int)c->recv.size();
    const dim3 grid((unsigned)ntile, (unsigned)nrec, (unsigned)a.ng);
    if (c->method == KIWI_FLOATING_L2NORM)
        hipLaunchKernelGGL((wavecand_float_kernel<K, 1>), grid, dim3(kThreads), 0, c->stream, c->proc_d.p, c->syn_stride, c->recv_d.p, c->comps_d.p,
                           c->refx_d.p, c->tw_d.p, a.ok, nrec, c->nmis, c->syn_factor, c->gm.dt, a.x, a.ncand, a.slab, a.shift);
    else
        hipLaunchKernelGGL((wavecand_float_kernel<K, 2>), grid, dim3(kThreads), 0, c->stream, c->proc_d.p, c->syn_stride, c->recv_d.p, c->comps_d.p,
                           c->refx_d.p, c->tw_d.p, a.ok, nrec, c->nmis, c->syn_factor, c->gm.dt, a.x, a.ncand, a.slab, a.shift);
    HIPCHECK(hipGetLastError());
}

// the groups [isrc0, isrc0 + ngroup K) of the uploaded batch, on waveform_candidates::run's skeleton; adds its HIP-event times to
// c->wavecand_float_ms: evaluation (run_chunk), the floating slot kernel, the fold kernels, the downloads
static void run(kiwi_hip_ctx *c, int isrc0, int ngroup, int K, const double *receiver_weight, int anarchy, const Call &cl)
{
    check_setup(c, K, cl);
    check_group_range("waveform_candidates_floating", c, isrc0, ngroup, K);
    if (ngroup == 0) return;
    const int nrec = (int)c->recv.size(), nmis = c->nmis;
    c->misfit_d.ensure((size_t)c->nsrc * c->nmis, &c->dev_bytes);
    c->global_d.ensure((size_t)c->nsrc, &c->dev_bytes);
    const int proc_which = 2;                                 // (the context refuses a misfit filter under a floating norm)
    c->fuse_now = can_fuse(c, proc_which, isrc0, ngroup * K);

    const std::vector<double> w = receiver_weights(c, receiver_weight);
    std::vector<SlotInfo> info((size_t)nmis);
    for (int m = 0; m < nmis; m++)
        info[(size_t)m] = SlotInfo{ c->comps[(size_t)m].rec, (m + 1 == nmis || c->comps[(size_t)m + 1].rec != c->comps[(size_t)m].rec) ? 1 : 0, 0, 0 };
    std::vector<float> xf((size_t)cl.ncand * K);
    for (size_t p = 0; p < xf.size(); p++) xf[p] = (float)cl.x[p];
    const size_t ntile = (size_t)(cl.ncand + kThreads - 1) / kThreads;
    // device buffers of the call: kept on the context and grown only
    auto &B = c->wavecand_float_bufs;
    constexpr size_t kInfoInts = sizeof(SlotInfo) / sizeof(int);
    B.w.ensure((size_t)std::max(nrec, 1), &c->dev_bytes);
    B.x.ensure(xf.size(), &c->dev_bytes);
    B.info.ensure((size_t)std::max(nmis, 1) * kInfoInts, &c->dev_bytes);
    // (w, info, xf and the tables of a chunk are read by these copies: nothing leaves this function, by return or by exception,
    // before the stream is drained)
    struct Drain { hipStream_t s; ~Drain() { (void)hipStreamSynchronize(s); } } drain{ c->stream };
    HIPCHECK(hipMemcpyAsync(B.w.p, w.data(), (size_t)nrec * sizeof(double), hipMemcpyHostToDevice, c->stream));
    HIPCHECK(hipMemcpyAsync(B.x.p, xf.data(), xf.size() * sizeof(float), hipMemcpyHostToDevice, c->stream));
    HIPCHECK(hipMemcpyAsync(B.info.p, info.data(), (size_t)nmis * sizeof(SlotInfo), hipMemcpyHostToDevice, c->stream));

    const PooledEvents<6> ev(c);                           // (ev[5]: immediately in front of the floating slot kernel)
    std::vector<float> norm_h;
    std::vector<int> ok_h;
    // per group: the slab of slot misfits and the slab of shifts, the norm factors, the tiles' bests, the outputs
    const size_t per_group = (size_t)nmis * cl.ncand * sizeof(float) + (size_t)nrec * cl.ncand * sizeof(short) + (size_t)nmis * sizeof(float) +
                             sizeof(int) + ntile * (sizeof(double) + sizeof(int)) + (size_t)nrec * sizeof(int) +
                             (size_t)cl.ncand * ((cl.misfit ? sizeof(double) : 0) + (cl.slot_misfit ? (size_t)nmis * sizeof(float) : 0) +
                                                 (cl.cand_shift ? (size_t)nrec * sizeof(short) : 0));
    int g0 = 0;
    while (g0 < ngroup) {
        const int ng = next_group_chunk(c, isrc0, g0, ngroup, K, 2, per_group, kNoSourceCap);       // (at most 65535 / K: a grid dimension)
        const int s0 = isrc0 + g0 * K;
        HIPCHECK(hipEventRecord(ev[0], c->stream));
        run_chunk(c, s0, ng * K, proc_which);
        HIPCHECK(hipEventRecord(ev[1], c->stream));
        // the norm factors of the chunk's slots (the context's floating ones) and which of its groups are evaluated at all
        norm_h.assign((size_t)ng * nmis, 0.f);
        ok_h.assign((size_t)ng, 1);
        for (int g = 0; g < ng; g++) {
            for (int i = 0; i < K; i++) if (c->src_status[(size_t)s0 + (size_t)g * K + i]) ok_h[(size_t)g] = 0;
            if (ok_h[(size_t)g]) std::copy(c->norm_h.begin(), c->norm_h.begin() + nmis, norm_h.begin() + (size_t)g * nmis);
        }
        const size_t nc = (size_t)ng * cl.ncand, ngr = (size_t)ng * nrec;
        B.slab.ensure(nc * nmis, &c->dev_bytes);
        B.shift.ensure(nc * nrec, &c->dev_bytes);
        B.norm.ensure(norm_h.size(), &c->dev_bytes);
        B.ok.ensure((size_t)ng, &c->dev_bytes);
        B.tile_v.ensure((size_t)ng * ntile, &c->dev_bytes); B.tile_i.ensure((size_t)ng * ntile, &c->dev_bytes);
        B.best_index.ensure((size_t)ng, &c->dev_bytes); B.best_misfit.ensure((size_t)ng, &c->dev_bytes); B.status.ensure((size_t)ng, &c->dev_bytes);
        B.best_shift.ensure(ngr, &c->dev_bytes);
        if (cl.misfit) B.misfit.ensure(nc, &c->dev_bytes);
        if (cl.cand_shift) B.cshift.ensure(nc * nrec, &c->dev_bytes);
        if (cl.slot_misfit) B.smis.ensure(nc * nmis, &c->dev_bytes);
        HIPCHECK(hipMemcpyAsync(B.norm.p, norm_h.data(), norm_h.size() * sizeof(float), hipMemcpyHostToDevice, c->stream));
        HIPCHECK(hipMemcpyAsync(B.ok.p, ok_h.data(), ok_h.size() * sizeof(int), hipMemcpyHostToDevice, c->stream));
        if (cl.slot_misfit) HIPCHECK(hipMemsetAsync(B.smis.p, 0, nc * nmis * sizeof(float), c->stream));
        HIPCHECK(hipEventRecord(ev[5], c->stream));
        const Args a{ B.ok.p, B.x.p, ng, cl.ncand, B.slab.p, B.shift.p };
        by_basis(K, [&](auto k) { launch<k.value>(c, a); });
        HIPCHECK(hipEventRecord(ev[2], c->stream));
        hipLaunchKernelGGL(waveform_candidates::wavecand_fold_kernel, dim3((unsigned)ntile, (unsigned)ng), dim3(kThreads), 0, c->stream, B.slab.p,
                           B.norm.p, B.ok.p, (const SlotInfo *)B.info.p, B.w.p, nmis, cl.outer_norm == 2 ? 1 : 0, anarchy ? 1 : 0, cl.ncand,
                           cl.misfit ? B.misfit.p : (double *)nullptr, cl.slot_misfit ? B.smis.p : (float *)nullptr, B.tile_v.p, B.tile_i.p, B.status.p);
        HIPCHECK(hipGetLastError());
        hipLaunchKernelGGL(spectral_candidates::speccand_fold_kernel, dim3((unsigned)ng), dim3(64), 0, c->stream, B.tile_v.p, B.tile_i.p, (int)ntile,
                           B.best_index.p, B.best_misfit.p);
        HIPCHECK(hipGetLastError());
        hipLaunchKernelGGL(wavecand_float_shift_kernel, dim3((unsigned)((cl.cand_shift ? ntile : 0) + 1), (unsigned)ng), dim3(kThreads),
                           0, c->stream, B.shift.p, c->recv_d.p, c->comps_d.p, B.ok.p, B.best_index.p, nrec, cl.ncand, B.best_shift.p,
                           cl.cand_shift ? B.cshift.p : (short *)nullptr);
        HIPCHECK(hipGetLastError());
        HIPCHECK(hipEventRecord(ev[3], c->stream));
        const Call o = cl.at(g0, nmis, nrec);
        HIPCHECK(hipMemcpyAsync(o.best_index, B.best_index.p, (size_t)ng * sizeof(int), hipMemcpyDeviceToHost, c->stream));
        HIPCHECK(hipMemcpyAsync(o.best_misfit, B.best_misfit.p, (size_t)ng * sizeof(double), hipMemcpyDeviceToHost, c->stream));
        HIPCHECK(hipMemcpyAsync(o.status, B.status.p, (size_t)ng * sizeof(int), hipMemcpyDeviceToHost, c->stream));
        HIPCHECK(hipMemcpyAsync(o.best_shift, B.best_shift.p, ngr * sizeof(int), hipMemcpyDeviceToHost, c->stream));
        if (cl.misfit) HIPCHECK(hipMemcpyAsync(o.misfit, B.misfit.p, nc * sizeof(double), hipMemcpyDeviceToHost, c->stream));
        if (cl.cand_shift) HIPCHECK(hipMemcpyAsync(o.cand_shift, B.cshift.p, nc * nrec * sizeof(short), hipMemcpyDeviceToHost, c->stream));
        if (cl.slot_misfit) HIPCHECK(hipMemcpyAsync(o.slot_misfit, B.smis.p, nc * nmis * sizeof(float), hipMemcpyDeviceToHost, c->stream));
        HIPCHECK(hipEventRecord(ev[4], c->stream));
        HIPCHECK(hipStreamSynchronize(c->stream));
        if (o.slot_norm) std::copy(norm_h.begin(), norm_h.end(), o.slot_norm);
        // (the host's tables of the chunk and their upload lie between ev[1] and ev[5]: in none of the four)
        ev.add_elapsed(c->wavecand_float_ms, 0, 0, 1);
        ev.add_elapsed(c->wavecand_float_ms, 1, 5, 2);
        ev.add_elapsed(c->wavecand_float_ms, 2, 2, 3);
        ev.add_elapsed(c->wavecand_float_ms, 3, 3, 4);
        g0 += ng;
    }
    leave_evaluated(c, isrc0, ngroup * K, proc_which);
    for_each_failed_group(c, isrc0, ngroup, K, [&](int g) { fill_failed(1, nmis, nrec, cl.at(g, nmis, nrec)); });
}

// kiwi_hip_waveform_candidates_floating_params piece by piece (PieceCall, kiwi_group_run.hpp)
static PieceCall piece_call(int K, const double *receiver_weight, int anarchy, const Call &cl)
{
    auto mine = [=](const kiwi_hip_ctx *c, int s0) { return cl.at(s0 / K, c->nmis, (int)c->recv.size()); };
    return PieceCall{ K,
        [=](kiwi_hip_ctx *c) { check_setup(c, K, cl); },
        [=](kiwi_hip_ctx *c, int s0, int n) { fill_failed(n / K, c->nmis, (int)c->recv.size(), mine(c, s0)); },
        [=](kiwi_hip_ctx *c, int s0, int n) { run(c, 0, n / K, K, receiver_weight, anarchy, mine(c, s0)); } };
}

} // namespace waveform_candidates_floating
