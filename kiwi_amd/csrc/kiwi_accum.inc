// kiwi_accum.inc -- the accumulate kernels of the trial-source hot path ("convolution": make_seismogram, seismogram.f90:36-301,
// on top of gfdb_get_trace_bilin, gfdb.f90:865-950, and trace_multiply_add, sparse_trace.f90:597-707).
//
// Included by kiwi_accum.hip INSIDE namespace kiwi::exact or kiwi::fused -- the same text compiled under two arithmetic
// contracts:
//   exact  (-ffp-contract=off): every fp32 multiply and add rounded on its own, in the reference's order (its x86-64 host has
//          no fused operation): synthetics and misfits bit-identical to the CPU oracle given equal geometry records;
//   fused  (-ffp-contract=fast): the same operations in the same order, a multiply and the add that consumes it contracted
//          into one v_pk_fma_f32 / v_fma_f32 (one rounding instead of two): tolerance class -- misfits within 1e-6 of the
//          norm factor, synthetics within 2e-6 of the trace maximum (north_star) -- at half the vector instructions.
// Geometry (rows, shifts, weights, coefficients) comes from geometry_kernel, which is never contracted.
//
//   accumulate_kernel          direct: every centroid streams its 4 x n_g rows from global memory (A/B baseline)
//   accumulate_grouped_kernel  blended tiles in LDS shared by the time steps of a sub-fault (and by runs of sources)
//   accumulate_multi_kernel    ... and by 2 or 4 neighbouring trial sources per workgroup
//   accumulate_cell_kernel / accumulate_cellw_kernel   raw rows of a GF cell in registers across its centroids
// Every output sample is owned by one thread and centroids / GF components are added in the reference's order.

// ------------------------------------------------------------------------------------------------
// accumulate

typedef float f4u __attribute__((ext_vector_type(4), aligned(4)));   // dword-aligned 16-byte load
typedef float f2u __attribute__((ext_vector_type(2), aligned(4)));   // dword-aligned 8-byte load

// KIWI_MAD(acc, w, v): acc + w * v, `w` a scalar, `v` a vector.  In the translation units built with -ffp-contract=fast the
// compiler fuses where it likes; the cell family's fused build (KIWI_EXPLICIT_FMA, round 6) is compiled with -ffp-contract=off
// like the exact one -- whose register allocation fits the three waves per SIMD; the contracting compile needed 175-189 registers
// for 168 -- and says HERE which multiply-adds are one operation: every product that is added to an accumulator (the blend's
// second to fourth term, both terms of an apply, the rotation).
#if defined(KIWI_EXPLICIT_FMA)
#ifndef KIWI_CELLW_AHEAD
#define KIWI_CELLW_AHEAD 3
#endif
template <class V> __device__ __forceinline__ V kiwi_mad(V acc, float w, V v)
{
    V ws;
    for (int k = 0; k < (int)(sizeof(V) / sizeof(float)); k++) ws[k] = w;
    return __builtin_elementwise_fma(ws, v, acc);
}
template <class V> __device__ __forceinline__ V kiwi_madv(V acc, V w, V v) { return __builtin_elementwise_fma(w, v, acc); }
#else
template <class V> __device__ __forceinline__ V kiwi_mad(V acc, float w, V v) { return acc + w * v; }
template <class V> __device__ __forceinline__ V kiwi_madv(V acc, V w, V v) { return acc + w * v; }
#endif

// Raw buffer loads for the rows of one group: the descriptor holds the group base (64 bit), the row's start comes as the
// instruction's SCALAR offset and the lane's position as its 32-bit vector offset -- no per-load vector address arithmetic
// (a global_load needs a 64-bit VGPR address per load: one v_lshl_add_u64 each, 40 per group).
typedef int v4i_t __attribute__((ext_vector_type(4)));
typedef int v2i_t __attribute__((ext_vector_type(2)));
__device__ __forceinline__ __amdgpu_buffer_rsrc_t gf_rsrc(const float *base)
{
    return __builtin_amdgcn_make_buffer_rsrc((void *)base, 0, -1, 0x00020000);      // raw buffer, 32-bit data, no range limit below 4 GB
}
__device__ __forceinline__ f4u buf_load4(__amdgpu_buffer_rsrc_t r, int voff_floats, int soff_floats)
{
    // byte offsets as unsigned 32-bit values: the host keeps a cell below 2^30 floats (kiwi_hip_set_gfdb / kiwi_hip_set_interp),
    // so neither wraps
    const v4i_t v = __builtin_amdgcn_raw_buffer_load_b128(r, (int)(4u * (unsigned)voff_floats), (int)(4u * (unsigned)soff_floats), 0);
    return f4u{ __int_as_float(v.x), __int_as_float(v.y), __int_as_float(v.z), __int_as_float(v.w) };
}

// five consecutive samples l-1 .. l+3 of one GF row (l relative to the row's first sample).
// The row is stored as [kRowPad zeros | n samples | end value repeated up to pitch], so clamping
// the start position implements "zero before the span, last value repeated after it"
// (sparse_trace.f90:337-338,696-703) without branches.
__device__ __forceinline__ void load5(const float *__restrict__ rowp, int l, int pitch, float (&v)[5])
{
    int q = kRowPad + l - 1;
    q = min(max(q, 0), pitch - 5);
    const float *p = rowp + q;
    v[0] = p[0];
    const f4u t = *(const f4u *)(p + 1);
    v[1] = t.x; v[2] = t.y; v[3] = t.z; v[4] = t.w;
}

// one Green's function component of one centroid onto 4 consecutive output samples.
// sparse_trace.f90:640-703 (shift, linear sub-sample interpolation, repeated end point) on top
// of gfdb.f90:944-949 (4-neighbour blend, summed in the order t00,t01,t10,t11).
template <bool BLEND>
__device__ __forceinline__ void gf_add(float (&out)[4], const float *__restrict__ G, const int2 *__restrict__ span,
                                       int pitch, const GeoRec &g, int ig, float factor, int j0)
{
    float b[5];
    int jend;
    const int r0 = g.row[0] + ig;
    const int2 s0 = span[r0];
    if (BLEND) {
        const int r1 = g.row[1] + ig, r2 = g.row[2] + ig, r3 = g.row[3] + ig;
        const int2 s1 = span[r1], s2 = span[r2], s3 = span[r3];
        jend = max(max(s0.y, s1.y), max(s2.y, s3.y));
        float v0[5], v1[5], v2[5], v3[5];
        load5(G + (size_t)r0 * pitch, j0 - s0.x, pitch, v0);
        load5(G + (size_t)r1 * pitch, j0 - s1.x, pitch, v1);
        load5(G + (size_t)r2 * pitch, j0 - s2.x, pitch, v2);
        load5(G + (size_t)r3 * pitch, j0 - s3.x, pitch, v3);
#pragma unroll
        for (int i = 0; i < 5; i++) {
            float acc = g.w[0] * v0[i];
            acc = acc + g.w[1] * v1[i];
            acc = acc + g.w[2] * v2[i];
            acc = acc + g.w[3] * v3[i];
            b[i] = acc;
        }
    } else {
        jend = s0.y;
        load5(G + (size_t)r0 * pitch, j0 - s0.x, pitch, b);
    }
    float wr = g.wfrac;
    float wl = 1.f - wr;
    wr = wr * factor;
    wl = wl * factor;
#pragma unroll
    for (int i = 0; i < 4; i++) {
        const bool tail = (j0 + i) > jend;            // sparse_trace.f90:698-703
        const float c1 = tail ? factor : wl;
        const float c2 = tail ? 0.f : wr;
        out[i] = out[i] + c1 * b[i + 1];
        out[i] = out[i] + c2 * b[i];
    }
}

template <int NG, bool BLEND>
__device__ __forceinline__ void centroid_add(float (&ar1)[4], float (&ar2)[4], float (&dz)[4],
                                             const float *__restrict__ G, const int2 *__restrict__ span, int pitch,
                                             const GeoRec &g, const RecvDev &rv, int j0)
{
    // components that are added, in application order (all of them unless a trace is missing: geometry_kernel)
    const int nlh = (g.flags & 8) ? (g.flags >> 8) & 15 : 15, nld = (g.flags & 8) ? (g.flags >> 12) & 15 : 15;
    constexpr int o9 = (NG == 10) ? 1 : 0;       // position shift behind the optional near-field component
#define GA(acc, pos, lim, ig, fac) do { if ((pos) < (lim)) gf_add<BLEND>(acc, G, span, pitch, g, ig, fac, j0); } while (0)
    if (rv.need_h && nlh > 0) {
        if (g.flags & 2) {                       // seismogram.f90:160-203 (a missing trace leaves before the sums are added)
            float t1[4] = { 0.f, 0.f, 0.f, 0.f }, t2[4] = { 0.f, 0.f, 0.f, 0.f };
            gf_add<BLEND>(t1, G, span, pitch, g, 0, g.f[0], j0);
            gf_add<BLEND>(t1, G, span, pitch, g, 1, g.f[1], j0);
            gf_add<BLEND>(t1, G, span, pitch, g, 2, g.f[2], j0);
            if (NG == 10) gf_add<BLEND>(t1, G, span, pitch, g, 8, g.f[5], j0);
            gf_add<BLEND>(t2, G, span, pitch, g, 3, g.f[3], j0);
            gf_add<BLEND>(t2, G, span, pitch, g, 4, g.f[4], j0);
#pragma unroll
            for (int i = 0; i < 4; i++) {
                ar1[i] = ar1[i] + g.cl * t1[i] - g.sl * t2[i];
                ar2[i] = ar2[i] + g.cl * t2[i] + g.sl * t1[i];
            }
        } else {                                 // seismogram.f90:205-231
            GA(ar1, 0, nlh, 0, g.f[0]);
            GA(ar1, 1, nlh, 1, g.f[1]);
            GA(ar1, 2, nlh, 2, g.f[2]);
            if (NG == 10) GA(ar1, 3, nlh, 8, g.f[5]);
            GA(ar2, 3 + o9, nlh, 3, g.f[3]);
            GA(ar2, 4 + o9, nlh, 4, g.f[4]);
        }
    }
    if (rv.has_d) {                              // seismogram.f90:236-253
        GA(dz, 0, nld, 5, g.f[0] * rv.sd);
        GA(dz, 1, nld, 6, g.f[1] * rv.sd);
        GA(dz, 2, nld, 7, g.f[2] * rv.sd);
        if (NG == 10) GA(dz, 3, nld, 9, g.f[5] * rv.sd);
    }
#undef GA
}

template <int NG>
__global__ __launch_bounds__(256) void accumulate_kernel(
    const float *__restrict__ G, const int2 *__restrict__ span, int pitch,
    const GeoRec *__restrict__ recs, const int *__restrict__ cent_ofs, int isrc0, int nrec,
    const RecvDev *__restrict__ recv, float *__restrict__ syn, size_t syn_stride, const int *__restrict__ synrow)
{
    const int tile = blockIdx.x, r = blockIdx.y, s = blockIdx.z;
    if (synrow && synrow[s] != s) return;
    const RecvDev &rv = recv[r];
    if (!rv.enabled) return;
    if (tile * kTile >= rv.wlen) return;
    const int tl = tile * kTile + threadIdx.x * 4;
    const int t0 = rv.wbeg + tl;
    const int cb = cent_ofs[isrc0], c0 = cent_ofs[isrc0 + s], nc = cent_ofs[isrc0 + s + 1] - c0;
    const GeoRec *__restrict__ rc = recs + ((size_t)(c0 - cb) * nrec + (size_t)r * nc);

    float ar1[4] = { 0.f, 0.f, 0.f, 0.f }, ar2[4] = { 0.f, 0.f, 0.f, 0.f }, dz[4] = { 0.f, 0.f, 0.f, 0.f };
    for (int c = 0; c < nc; c++) {               // seismogram.f90:131, table order
        const GeoRec &g = rc[c];
        if (g.row[0] < 0) continue;              // 'cycle' on a missing trace
        const int j0 = t0 - g.ishift;            // strip(x) += trace(x - itraceshift), sparse_trace.f90:605
        if (g.flags & 1) centroid_add<NG, false>(ar1, ar2, dz, G, span, pitch, g, rv, j0);
        else             centroid_add<NG, true>(ar1, ar2, dz, G, span, pitch, g, rv, j0);
    }

    if (tl >= rv.wlen) return;
    float *__restrict__ so = syn + (size_t)s * syn_stride + tl;
    for (int k = 0; k < rv.ncomp; k++) {         // seismogram.f90:256-283
        float4 o;
        const float sg = rv.sign[k];
        switch (rv.comp[k]) {
        case 1: o = make_float4(ar1[0] * sg, ar1[1] * sg, ar1[2] * sg, ar1[3] * sg); break;
        case 2: o = make_float4(ar2[0] * sg, ar2[1] * sg, ar2[2] * sg, ar2[3] * sg); break;
        case 3: o = make_float4(dz[0], dz[1], dz[2], dz[3]); break;       // sign already in the factors (:239)
        case 4: {
            float a[4];
#pragma unroll
            for (int i = 0; i < 4; i++) a[i] = (rv.cl0 * ar1[i] - rv.sl0 * ar2[i]) * sg;
            o = make_float4(a[0], a[1], a[2], a[3]); break; }
        default: {
            float a[4];
#pragma unroll
            for (int i = 0; i < 4; i++) a[i] = (rv.cl0 * ar2[i] + rv.sl0 * ar1[i]) * sg;
            o = make_float4(a[0], a[1], a[2], a[3]); break; }
        }
        *(float4 *)(so + rv.synofs[k]) = o;
    }
}

// ------------------------------------------------------------------------------------------------
// accumulate, grouped: blended GF tiles staged in LDS and reused by every centroid of a sub-fault
//
// Consecutive centroids that sit at the same point (the nt source-time-function steps of one
// sub-fault) need the SAME blended traces, only shifted by a different number of samples and
// weighted differently.  The workgroup therefore blends each needed GF component ONCE per group
// into an LDS tile (coalesced 16-byte global loads, 16-byte LDS stores) that covers the tile plus
// the spread of the group's integer shifts, and then every centroid of the group does its
// shift-interpolate-accumulate from LDS (conflict-free: lane l owns samples l, l+256, l+512, l+768
// of the tile).  Global traffic drops by the group size (5 for the benchmark's bilateral source);
// per-sample operation order is unchanged, so results are bit-identical to accumulate_kernel.


// A GeoRec travels through the grouped kernel "lane-distributed": lane i (< 20) of every wave
// holds dword i of the record in ONE VGPR (a single coalesced 80-byte load that can be issued a
// whole centroid ahead), and fields are broadcast to SGPRs with v_readlane when needed.  Compared
// with scalar loads this removes ~16 serialised SMEM round trips per centroid.
__device__ __forceinline__ int rec_load(const GeoRec *__restrict__ rc, int c, int nc, int lane)
{
    int v = 0;
    if (c < nc && lane < 20) v = ((const int *)(rc + c))[lane];
    return v;
}
#define REC_I(v, k) __builtin_amdgcn_readlane((v), (k))
#define REC_F(v, k) __int_as_float(__builtin_amdgcn_readlane((v), (k)))

// Compact load descriptors (geometry_kernel's off4: databases whose components of a node all start at the same sample and whose
// rows all end in zero).  `o`: lane l holds the position of trace sample 0 inside the rows of node l & 3 (kRowPad - first); `rec`:
// the group's head record, lane-distributed (lanes 0 .. 3: the four node rows).  Rebuilds the lane-distributed descriptor row
// exactly as write_tab lays it out: lane 4 ig + k: tb = (row_k + ig - row_0) pitch (the rows of a node are consecutive: component
// ig of node k is row_k + ig), ta = tb + o_k; lanes 40 .. 51 the end indices of the tail rule: never (every row ends in zero); lanes
// 52 / 53 the smallest / largest o_k, lane 54: one start per node.
__device__ __forceinline__ int off4_load(const int *__restrict__ tc /* first record of the (source, receiver) pair */, int c, int lane)
{
    // (the record's address in scalar registers, the lane's part as a 32-bit offset: left to itself the compiler keeps `tc + (lane & 3)`
    // as a 64-bit pointer per lane across the whole kernel)
    const size_t a = (size_t)(tc + (size_t)c * 4);
    // (a pointer made from integers is a GENERIC pointer to the compiler: the load became a flat_load, which counts on the LDS / scalar
    // wait counter as well -- and the `s_waitcnt lgkmcnt(0)` in front of the next barrier then waited for this round trip to memory, in
    // every wave and group: the "next group's records" phase of the per-CU trace, ~ 1000 cycles.  Global address space: vmcnt alone.)
    typedef const __attribute__((address_space(1))) int *gptr_t;
    const gptr_t q = (gptr_t)(((size_t)(unsigned)__builtin_amdgcn_readfirstlane((int)(a >> 32)) << 32) | (unsigned)__builtin_amdgcn_readfirstlane((int)a));
    return q[lane & 3];
}
template <bool CELLINFO = false>          // (lanes 52 .. 54: read by the cell kernels only)
__device__ __forceinline__ void desc_expand(int o, int rec, int lane, int pitch, int &ta, int &tb)
{
    const int rk = __shfl(rec, lane & 3, 64);
    const int r0 = REC_I(rec, 0);
    const int fl = (rk - r0 + (lane >> 2)) * pitch;
    tb = fl;
    ta = lane < 40 ? fl + o : 0x7fffffff;
    if constexpr (CELLINFO) {
        const int o0 = REC_I(o, 0), o1 = REC_I(o, 1), o2 = REC_I(o, 2), o3 = REC_I(o, 3);
        if (lane == 52) ta = min(min(o0, o1), min(o2, o3));
        if (lane == 53) ta = max(max(o0, o1), max(o2, o3));
        if (lane == 54) ta = 1;
    }
}

__device__ __forceinline__ void rec_head(int v, int o, GeoRec &g)
{
    g.row[0] = REC_I(v, o + 0); g.row[1] = REC_I(v, o + 1); g.row[2] = REC_I(v, o + 2); g.row[3] = REC_I(v, o + 3);
    g.w[0] = REC_F(v, o + 4); g.w[1] = REC_F(v, o + 5); g.w[2] = REC_F(v, o + 6); g.w[3] = REC_F(v, o + 7);
    g.ishift = REC_I(v, o + 8);
    g.flags = REC_I(v, o + 18);
    g.pad = REC_I(v, o + 19);
}

__device__ __forceinline__ f4u load4(const float *__restrict__ rowp, int l, int pitch)
{
    int q = kRowPad + l;
    q = min(max(q, 0), pitch - 4);           // zeros before the span, end value after it (see load5)
    return *(const f4u *)(rowp + q);
}

// Load descriptors (see geometry_kernel): ta / tb are the lane-distributed halves of the group's descriptor row;
// the float index of sample j of node k's trace of component ig is
// clamp(ta[4ig+k] + j, tb[4ig+k], tb[4ig+k] + pitch - 4), which implements "zero before the span, end value
// repeated after it" on the padded row.

// Build the main chunk (LDS positions [4*tid, 4*tid+4)) of SEVERAL components at once: all 4*N
// loads are issued before the first blend so that one L2 round trip is paid per batch, not per
// component (left to itself the compiler serialises load -> blend -> ds_write per component).
// FAST: every row of the group covers the whole tile without clamping (checked once per group), so a
// load address is a wave-uniform row base (SGPR pair) plus the lane's position -- no per-load VALU
// address arithmetic.
template <bool BLEND, bool FAST, int N>
__device__ __forceinline__ void build_batch(float *__restrict__ tile0, int lds_tile, const int (&igs)[N], int p, int jb,
                                            const float *__restrict__ G, int pitch, int ta, int tb, const GeoRec &g)
{
    const int j = jb + p;
    f4u v[N][BLEND ? 4 : 1];
#pragma unroll
    for (int q = 0; q < N; q++) {
#pragma unroll
        for (int k = 0; k < (BLEND ? 4 : 1); k++) {
            const int base = REC_I(ta, 4 * igs[q] + k);
            if constexpr (FAST) {
                v[q][k] = buf_load4(gf_rsrc(G), p, base + jb);       // scalar row offset + the lane's position
            } else {
                const int lo = REC_I(tb, 4 * igs[q] + k);
                const int idx = min(max(base + j, lo), lo + pitch - 4);
                v[q][k] = *(const f4u *)(G + (size_t)(unsigned)idx);
            }
        }
    }
#pragma unroll
    for (int q = 0; q < N; q++) {
        f4u b;
        if constexpr (BLEND) {
            b = g.w[0] * v[q][0];             // gfdb.f90:946-949, summed in this order
            b = b + g.w[1] * v[q][1];
            b = b + g.w[2] * v[q][2];
            b = b + g.w[3] * v[q][3];
        } else {
            b = v[q][0];
        }
        *(float4 *)(tile0 + igs[q] * lds_tile + p) = make_float4(b.x, b.y, b.z, b.w);
    }
}

// Streamed form of build_batch for ALL components: sub-batches of two components (8 loads); two sub-batches are
// kept in flight, the blend of sub-batch i is followed by the issue of sub-batch i + 2.  The whole group then costs
// about one L2 round trip plus the issue time instead of one round trip per batch, with fewer registers in flight.
template <bool BLEND, bool FAST>
__device__ __forceinline__ void pair_issue(f4u (&v)[2][BLEND ? 4 : 1], int ig0, int p, int jb, const float *__restrict__ G,
                                           int pitch, int ta, int tb)
{
    const int j = jb + p;
#pragma unroll
    for (int q = 0; q < 2; q++) {
#pragma unroll
        for (int k = 0; k < (BLEND ? 4 : 1); k++) {
            const int base = REC_I(ta, 4 * (ig0 + q) + k);
            if constexpr (FAST) {
                v[q][k] = buf_load4(gf_rsrc(G), p, base + jb);
            } else {
                const int lo = REC_I(tb, 4 * (ig0 + q) + k);
                const int idx = min(max(base + j, lo), lo + pitch - 4);
                v[q][k] = *(const f4u *)(G + (size_t)(unsigned)idx);
            }
        }
    }
}

template <bool BLEND>
__device__ __forceinline__ void pair_finish(const f4u (&v)[2][BLEND ? 4 : 1], float *__restrict__ tile0, int lds_tile, int ig0, int p,
                                            const GeoRec &g)
{
#pragma unroll
    for (int q = 0; q < 2; q++) {
        f4u b;
        if constexpr (BLEND) {
            b = g.w[0] * v[q][0];             // gfdb.f90:946-949, summed in this order
            b = b + g.w[1] * v[q][1];
            b = b + g.w[2] * v[q][2];
            b = b + g.w[3] * v[q][3];
        } else {
            b = v[q][0];
        }
        *(float4 *)(tile0 + (ig0 + q) * lds_tile + p) = make_float4(b.x, b.y, b.z, b.w);
    }
}

// The halo (LDS positions TILE .. npos, at most kHalo / 4 = 16 chunks of 4 samples per component) is built by
// one lane per (component, chunk) pair so that its loads travel in the same L2 round trip as the second main batch
// instead of costing a round trip of their own.  Per-lane descriptors come from the lane-distributed row by
// ds_bpermute.  halo_issue only loads; halo_finish blends and stores.
struct HaloRegs { f4u v[4]; };

// The load descriptors of a centroid group as the build reads them: a(ig, k) / b(ig, k): ta / tb of node k's row of component ig,
// wave-uniform; ha / hb: the same for the component of a halo lane.
// DescLanes: the lane-distributed descriptor row (write_tab's layout, or desc_expand's copy of it): read-lanes and, for the halo,
// ds_bpermute.
struct DescLanes {
    static constexpr bool linear = false;
    int ta, tb;
    __device__ __forceinline__ int a(int ig, int k) const { return REC_I(ta, 4 * ig + k); }
    __device__ __forceinline__ int b(int ig, int k) const { return REC_I(tb, 4 * ig + k); }
    __device__ __forceinline__ int ha(int hig, int k) const { return __shfl(ta, 4 * hig + k, 64); }
    __device__ __forceinline__ int hb(int hig, int k) const { return __shfl(tb, 4 * hig + k, 64); }
    // every row of the group covers LDS positions 0 .. lds_tile - 1 of a tile that starts at trace sample jb without clamping
    __device__ __forceinline__ bool fast(int jb, int lds_tile, int pitch, int lane, int ng) const
    {
        const bool lane_ok = lane >= 4 * ng || (ta + jb >= tb && ta + jb + lds_tile <= tb + pitch);
        return __builtin_amdgcn_ballot_w64(lane_ok) == ~0ull;
    }
};
// maximum / minimum of wave-uniform integers on the scalar unit (left to itself the compiler moves them to the vector pipe
// for its three-operand forms)
__device__ __forceinline__ int smax_u(int a, int b) { int r; asm("s_max_i32 %0, %1, %2" : "=s"(r) : "s"(a), "s"(b) : "scc"); return r; }
__device__ __forceinline__ int smin_u(int a, int b) { int r; asm("s_min_i32 %0, %1, %2" : "=s"(r) : "s"(a), "s"(b) : "scc"); return r; }
// DescPlan: compact descriptors held in scalar registers (PlanSrc::row, o): what desc_expand lays out in lanes, tb = (row_k + ig -
// row_0) pitch and ta = tb + o_k, as scalar arithmetic (the same 32-bit sums); `hoff`: the halo lane's component times pitch.
struct DescPlan {
    static constexpr bool linear = true;            // a(ig, k) = a(0, k) + ig pitch
    int b0[4], o[4], pitch, hoff;
    __device__ __forceinline__ int b(int ig, int k) const { return b0[k] + ig * pitch; }
    __device__ __forceinline__ int a(int ig, int k) const { return b0[k] + ig * pitch + o[k]; }
    __device__ __forceinline__ int hb(int, int k) const { return b0[k] + hoff; }
    __device__ __forceinline__ int ha(int, int k) const { return b0[k] + hoff + o[k]; }
    __device__ __forceinline__ bool fast(int jb, int lds_tile, int pitch_, int, int) const
    {
        // (ta - tb = o_k in every lane below 4 ng: the lanes' test is that of the smallest and the largest o_k)
        // (on the scalar unit: the compiler's three-operand minimum and maximum are vector instructions, five moves to feed them)
        const int omin = smin_u(smin_u(o[0], o[1]), smin_u(o[2], o[3])), omax = smax_u(smax_u(o[0], o[1]), smax_u(o[2], o[3]));
        return omin + jb >= 0 && omax + jb + lds_tile <= pitch_;
    }
};

template <bool BLEND, bool FAST, typename D>
__device__ __forceinline__ HaloRegs halo_issue(bool active, int ig, int ph, int jb, const float *__restrict__ G, int pitch, const D &d)
{
    HaloRegs h;
#pragma unroll
    for (int k = 0; k < (BLEND ? 4 : 1); k++) {
        const int base = d.ha(ig, k);
        int idx = base + jb + ph;
        if constexpr (!FAST) {
            const int lo = d.hb(ig, k);
            idx = min(max(idx, lo), lo + pitch - 4);
        }
        h.v[k] = f4u{ 0.f, 0.f, 0.f, 0.f };
        if (active) h.v[k] = *(const f4u *)(G + (size_t)(unsigned)idx);
    }
    return h;
}
template <bool BLEND, bool FAST>
__device__ __forceinline__ HaloRegs halo_issue(bool active, int ig, int ph, int jb, const float *__restrict__ G, int pitch,
                                               int ta, int tb)
{
    return halo_issue<BLEND, FAST>(active, ig, ph, jb, G, pitch, DescLanes{ ta, tb });
}

template <bool BLEND>
__device__ __forceinline__ void halo_finish(bool active, const HaloRegs &h, float *__restrict__ tile0, int lds_tile, int ig, int ph,
                                            const GeoRec &g)
{
    f4u b;
    if constexpr (BLEND) {
        b = g.w[0] * h.v[0];                  // gfdb.f90:946-949, summed in this order
        b = kiwi_mad(b, g.w[1], h.v[1]);
        b = kiwi_mad(b, g.w[2], h.v[2]);
        b = kiwi_mad(b, g.w[3], h.v[3]);
    } else {
        b = h.v[0];
    }
    if (active) *(float4 *)(tile0 + ig * lds_tile + ph) = make_float4(b.x, b.y, b.z, b.w);
}

// the same with TWO samples per lane (accumulate_cellw_kernel, round 6: a wave's halo is 12 positions -- cell runs are cut at a
// shift range of 11, which cfg4 never reaches -- so a chunk is one register pair per node: 8 registers instead of 16, 7 packed
// instructions per blend instead of 14)
struct HaloRegs2 { f2u v[4]; };

template <bool FAST>
__device__ __forceinline__ HaloRegs2 halo_issue2(bool active, int ig, int ph, int jb, const float *__restrict__ G, int pitch, int ta, int tb)
{
    HaloRegs2 h;
#pragma unroll
    for (int k = 0; k < 4; k++) {
        const int base = __shfl(ta, 4 * ig + k, 64);
        int idx = base + jb + ph;
        if constexpr (!FAST) {
            const int lo = __shfl(tb, 4 * ig + k, 64);
            idx = min(max(idx, lo), lo + pitch - 2);
        }
        h.v[k] = f2u{ 0.f, 0.f };
        if (active) h.v[k] = *(const f2u *)(G + (size_t)(unsigned)idx);
    }
    return h;
}

__device__ __forceinline__ void halo_finish2(bool active, const HaloRegs2 &h, float *__restrict__ tile0, int lds_tile, int ig, int ph,
                                             float w0, float w1, float w2, float w3)
{
    f2u b = w0 * h.v[0];                      // gfdb.f90:946-949, summed in this order
    b = kiwi_mad(b, w1, h.v[1]);
    b = kiwi_mad(b, w2, h.v[2]);
    b = kiwi_mad(b, w3, h.v[3]);
    if (active) *(float2 *)(tile0 + ig * lds_tile + ph) = make_float2(b.x, b.y);
}

typedef float f2v __attribute__((ext_vector_type(2)));
typedef const __attribute__((address_space(3))) float *lds_cfp;

// Apply-phase mapping of samples to lanes: lane l of wave w owns the four tile samples 256 w + l + 64 q, q = 0..3 (stride
// 64, not four consecutive ones).  The two blended samples an output needs, b[j-1] and b[j], then sit at LDS dwords
// base + 64 q and base + 64 q + 1 of the lane: consecutive lanes read consecutive dwords (no bank conflicts whatever the
// shift), the compiler fuses the reads of two q into one ds_read2st64_b32 whose result IS the aligned register pair a
// packed multiply wants -- for every shift residue alike, so no v_pk_mov assemblies and no per-residue code variants.
// LDS_TILE is a multiple of 64 dwords, which puts all components and q of a centroid within the instruction's offsets.
// NP register pairs per lane: 2 (four outputs per lane: q0,q1 | q2,q3) or 1 (two outputs per lane, accumulate_cell_kernel)
template <int NP = 2> struct TileRegsN { f2v lo[NP], hi[NP]; };   // b[j-1] and b[j] of the lane's outputs
typedef TileRegsN<2> TileRegs;

// The lane's two LDS base addresses of a centroid: b[j-1] and b[j] of its output q = 0 in component 0.  The second is
// the first plus one dword, but hidden from the compiler: it would otherwise pair the adjacent dwords (b[j-1], b[j]) of
// ONE output into a ds_read2_b32 and then shuffle registers, instead of pairing the same quantity of TWO outputs.
struct TileBase { const __attribute__((address_space(3))) float *lo, *hi; };

__device__ __forceinline__ TileBase tile_base(const float *__restrict__ p)
{
    typedef const __attribute__((address_space(3))) float *lds_fp;
    TileBase b;
    b.lo = (lds_fp)p;
    unsigned a = (unsigned)(size_t)(b.lo + 1);
    asm volatile("" : "+v"(a));
    b.hi = (lds_fp)(size_t)a;
    return b;
}

template <int NP = 2>
__device__ __forceinline__ TileRegsN<NP> tile_load(const TileBase &b, int ofs)
{
    TileRegsN<NP> t;
#pragma unroll
    for (int h = 0; h < NP; h++) {
        t.lo[h] = f2v{ b.lo[ofs + 128 * h], b.lo[ofs + 128 * h + 64] };
        t.hi[h] = f2v{ b.hi[ofs + 128 * h], b.hi[ofs + 128 * h + 64] };
    }
    return t;
}

// The lane's 4 output samples are held as two register pairs so that the multiplies and adds are
// v_pk_mul_f32 / v_pk_add_f32 (two IEEE fp32 operations per lane and instruction, each rounded
// separately exactly like the scalar form; no FMA).
template <bool TAIL, int NP = 2>
__device__ __forceinline__ void tile_fma(f2v (&out)[NP], const TileRegsN<NP> &t, int jl, int jend, float factor, float wl, float wr)
{
#pragma unroll
    for (int h = 0; h < NP; h++) {
        f2v c1 = { wl, wl }, c2 = { wr, wr };
        if (TAIL) {                               // sparse_trace.f90:698-703, jl = trace index of b[j-1] of the lane's output q = 0
            const bool t0 = (jl + 128 * h + 1) > jend, t1 = (jl + 128 * h + 64 + 1) > jend;
            c1.x = t0 ? factor : wl; c2.x = t0 ? 0.f : wr;
            c1.y = t1 ? factor : wl; c2.y = t1 ? 0.f : wr;
        }
        out[h] = kiwi_madv(out[h], c1, t.hi[h]);
        out[h] = kiwi_madv(out[h], c2, t.lo[h]);
    }
}

template <bool TAIL, int NP = 2>
__device__ __forceinline__ void tile_add(f2v (&out)[NP], const TileBase &b, int ofs, int jl, int jend,
                                         float factor, float wfrac)
{
    const TileRegsN<NP> t = tile_load<NP>(b, ofs);
    float wr = wfrac;
    float wl = 1.f - wr;
    wr = wr * factor;
    wl = wl * factor;
    tile_fma<TAIL, NP>(out, t, jl, jend, factor, wl, wr);
}

// all GF components of one centroid (reference order)
template <int NG, int LDS_TILE, bool TAIL, int NP = 2>
__device__ __forceinline__ void centroid_apply(f2v (&ar1)[NP], f2v (&ar2)[NP], f2v (&dz)[NP],
                                               const TileBase &chunk0, int jl, const int (&jend)[NG],
                                               bool need_h, bool has_d, int flags, float wfrac, float sd,
                                               float f0, float f1, float f2, float f3, float f4, float f5,
                                               float cl, float sl)
{
    // components that are added, in application order (all of them unless a trace is missing: geometry_kernel)
    const int nlh = (flags & 8) ? (flags >> 8) & 15 : 15, nld = (flags & 8) ? (flags >> 12) & 15 : 15;
    constexpr int o9 = (NG == 10) ? 1 : 0;
#define TADD(acc, ig, fac) tile_add<TAIL, NP>(acc, chunk0, (ig) * LDS_TILE, jl, jend[ig], fac, wfrac)
#define TADDL(acc, pos, lim, ig, fac) do { if ((pos) < (lim)) TADD(acc, ig, fac); } while (0)
    if (need_h && nlh > 0) {
        if (flags & 2) {                         // seismogram.f90:160-203
            f2v t1[NP], t2[NP];
#pragma unroll
            for (int i = 0; i < NP; i++) { t1[i] = f2v{ 0.f, 0.f }; t2[i] = f2v{ 0.f, 0.f }; }
            TADD(t1, 0, f0); TADD(t1, 1, f1); TADD(t1, 2, f2);
            if constexpr (NG == 10) TADD(t1, 8, f5);
            TADD(t2, 3, f3); TADD(t2, 4, f4);
#pragma unroll
            for (int i = 0; i < NP; i++) {
                ar1[i] = ar1[i] + cl * t1[i] - sl * t2[i];
                ar2[i] = ar2[i] + cl * t2[i] + sl * t1[i];
            }
        } else {                                 // seismogram.f90:205-231
            TADDL(ar1, 0, nlh, 0, f0); TADDL(ar1, 1, nlh, 1, f1); TADDL(ar1, 2, nlh, 2, f2);
            if constexpr (NG == 10) TADDL(ar1, 3, nlh, 8, f5);
            TADDL(ar2, 3 + o9, nlh, 3, f3); TADDL(ar2, 4 + o9, nlh, 4, f4);
        }
    }
    if (has_d) {                                 // seismogram.f90:236-253
        TADDL(dz, 0, nld, 5, f0 * sd); TADDL(dz, 1, nld, 6, f1 * sd); TADDL(dz, 2, nld, 7, f2 * sd);
        if constexpr (NG == 10) TADDL(dz, 3, nld, 9, f5 * sd);
    }
#undef TADDL
#undef TADD
}

// The common case (receiver with horizontal and vertical components), software-pipelined: the LDS reads
// of component i + kAhead are issued before the arithmetic of component i, so that a lone wave is not
// stalled for a full LDS round trip per component (a wave can only issue every 4th cycle; with 3 waves per
// SIMD exposed latency is what bounds this kernel).  Same operations in the same order as centroid_apply.
template <int NG, int LDS_TILE, bool TAIL, bool SCOEF, int NP = 2>
__device__ __forceinline__ void centroid_apply_hd(f2v (&ar1)[NP], f2v (&ar2)[NP], f2v (&dz)[NP],
                                                  const TileBase &chunk0, int jl, const int (&jend)[NG],
                                                  int flags, const float *__restrict__ coef, int rec, float sd,
                                                  float cl, float sl)
{
    // rec: the lane-distributed record of the centroid; its weights and interpolation fraction are fetched only where
    // the variant needs them (the tail rule's `factor`, or coefficients computed in registers)
    float wfrac = 0.f, f0 = 0.f, f1 = 0.f, f2 = 0.f, f3 = 0.f, f4 = 0.f, f5 = 0.f;
    if constexpr (TAIL || !SCOEF) {
        wfrac = REC_F(rec, 9);
        f0 = REC_F(rec, 10); f1 = REC_F(rec, 11); f2 = REC_F(rec, 12); f3 = REC_F(rec, 13); f4 = REC_F(rec, 14); f5 = REC_F(rec, 15);
    }
    // coef: the centroid's 2 * NG interpolation coefficients (wl, wr per component in application order), computed
    // by geometry_kernel; the pointer is wave-uniform, so these are scalar loads and the coefficients reach the
    // packed multiplies as SGPR operands -- no vector instructions spent on them
    constexpr int kAhead = 2;
    constexpr int seq10[10] = { 0, 1, 2, 8, 3, 4, 5, 6, 7, 9 }, seq8[8] = { 0, 1, 2, 3, 4, 5, 6, 7 };
    constexpr int nH1 = (NG == 10) ? 4 : 3;      // components summed into the radial trace
    const float fac10[10] = { f0, f1, f2, f5, f3, f4, f0 * sd, f1 * sd, f2 * sd, f5 * sd };
    const float fac8[8] = { f0, f1, f2, f3, f4, f0 * sd, f1 * sd, f2 * sd };
    const bool rot = (flags & 2) != 0;           // seismogram.f90:160-203 vs :205-231
    f2v t1[NP], t2[NP];
#pragma unroll
    for (int k = 0; k < NP; k++) { t1[k] = rot ? f2v{ 0.f, 0.f } : ar1[k]; t2[k] = rot ? f2v{ 0.f, 0.f } : ar2[k]; }
    float cw[2 * NG];
    if constexpr (SCOEF) {                        // scalar loads, issued together with the first LDS reads
#pragma unroll
        for (int i = 0; i < 2 * NG; i++) cw[i] = coef[i];
    } else {                                      // short sources (fused variant): computed here, as centroid_apply does
        const float wr0 = wfrac, wl0 = 1.f - wfrac;
#pragma unroll
        for (int i = 0; i < NG; i++) { const float f = (NG == 10) ? fac10[i] : fac8[i]; cw[coef_wl<NG>(i)] = wl0 * f; cw[coef_wr<NG>(i)] = wr0 * f; }
    }
    TileRegsN<NP> tr[NG];
#pragma unroll
    for (int i = 0; i < kAhead; i++) tr[i] = tile_load<NP>(chunk0, ((NG == 10) ? seq10[i] : seq8[i]) * LDS_TILE);
#pragma unroll
    for (int i = 0; i < NG; i++) {
        if (i + kAhead < NG) tr[i + kAhead] = tile_load<NP>(chunk0, ((NG == 10) ? seq10[i + kAhead] : seq8[i + kAhead]) * LDS_TILE);
        __builtin_amdgcn_sched_barrier(0);
        const int ig = (NG == 10) ? seq10[i] : seq8[i];
        const float fac = (NG == 10) ? fac10[i] : fac8[i];
        const float wl = cw[coef_wl<NG>(i)], wr = cw[coef_wr<NG>(i)];
        if (i < nH1) tile_fma<TAIL, NP>(t1, tr[i], jl, jend[ig], fac, wl, wr);
        else if (i < nH1 + 2) tile_fma<TAIL, NP>(t2, tr[i], jl, jend[ig], fac, wl, wr);
        else tile_fma<TAIL, NP>(dz, tr[i], jl, jend[ig], fac, wl, wr);
        if (i == nH1 + 1) {
            if (rot) {
#pragma unroll
                for (int k = 0; k < NP; k++) {
                    ar1[k] = ar1[k] + cl * t1[k] - sl * t2[k];
                    ar2[k] = ar2[k] + cl * t2[k] + sl * t1[k];
                }
            } else {
#pragma unroll
                for (int k = 0; k < NP; k++) { ar1[k] = t1[k]; ar2[k] = t2[k]; }
            }
        }
    }
}


// ---- epilogue of the accumulate kernels with four outputs per lane (samples tl + 64 q, q = 0 .. 3, held as two register pairs)
// one output trace of the receiver from the accumulators: rotation to N/E and sign (seismogram.f90:256-283), packed
__device__ __forceinline__ void out4(int comp, float sg, float cl0, float sl0, const f2v (&ar1)[2], const f2v (&ar2)[2], const f2v (&dz)[2],
                                     f2v &o01, f2v &o23)
{
    const f2v s2 = { sg, sg }, c2 = { cl0, cl0 }, n2 = { sl0, sl0 };
    switch (comp) {
    case 1: o01 = ar1[0] * s2; o23 = ar1[1] * s2; break;
    case 2: o01 = ar2[0] * s2; o23 = ar2[1] * s2; break;
    case 3: o01 = dz[0]; o23 = dz[1]; break;
    case 4: o01 = (c2 * ar1[0] - n2 * ar2[0]) * s2; o23 = (c2 * ar1[1] - n2 * ar2[1]) * s2; break;
    default: o01 = (c2 * ar2[0] + n2 * ar1[0]) * s2; o23 = (c2 * ar2[1] + n2 * ar1[1]) * s2; break;
    }
}
// the fused comparator over the lane's four samples (what misfit_kernel does per sample: comparator.f90:264,1173-1184,627-667);
// `whole`: all of them lie inside the window (workgroup-uniform).  l2norm with unit factor, the norm of every grid search, has a
// straight-line packed form -- the same operations in the same order as the general loop
__device__ __forceinline__ double fused_acc4(const FuseParams &fp, f2v o01, f2v o23, float mom, const float *__restrict__ rt,
                                             const float *__restrict__ tp, int tl, int wlen, bool whole)
{
    const bool unit = (fp.syn_factor == 1.f);
    double acc = 0.0;
    if (whole && unit && fp.method == 1) {
        const f2v m2 = { mom, mom };
        const f2v t01 = { tp[0], tp[64] }, t23 = { tp[128], tp[192] }, r01 = { rt[0], rt[64] }, r23 = { rt[128], rt[192] };
        const f2v d01 = r01 - (o01 * m2) * t01, d23 = r23 - (o23 * m2) * t23;
        acc = sq_acc(acc, d01.x); acc = sq_acc(acc, d01.y); acc = sq_acc(acc, d23.x); acc = sq_acc(acc, d23.y);
        return acc;
    }
    const float o[4] = { o01.x, o01.y, o23.x, o23.y };
#pragma unroll
    for (int i = 0; i < 4; i++) {
        if (tl + 64 * i >= wlen) break;
        const float v = o[i] * mom;
        const float vt = v * tp[64 * i];
        const float a = rt[64 * i];
        switch (fp.method) {
        case 1: { const float d = unit ? (a - vt) : (1.f * a - fp.syn_factor * vt); acc = sq_acc(acc, d); break; }
        case 2: { const float d = unit ? fabsf(a - vt) : fabsf(1.f * a - fp.syn_factor * vt); acc += (double)d; break; }
        case 5: acc += unit ? (double)(a * vt) : (double)(a * 1.f * vt * fp.syn_factor); break;
        default: { const double x = (double)(1.f * a), y = (double)(fp.syn_factor * vt); acc = fmax(acc, sqrt(x * x + y * y)); break; }
        }
    }
    return acc;
}

// ------------------------------------------------------------------------------------------------
// Register pairs carried between the centroids of a group (round 3), accumulate_grouped_kernel with 256 threads.
//
// The centroids of a group are the time steps of ONE sub-fault: the same blended traces, read at an integer shift that
// usually moves by exactly one sample from step to step (effective_dt == dt of the database: source_bilat.f90:443-457 with
// seismogram.f90:139).  With the stride-64 lane mapping b[j] of step k+1 IS b[j-1] of step k -- the register pairs the lane
// already holds.  The apply keeps the pairs of ALL components of the previous centroid in registers (two sets that swap
// roles at every centroid) and reads only what the new shift needs:
//     shift + 1 -> the old b[j-1] set serves as b[j], only b[j-1] is read        (20 reads instead of 40)
//     shift - 1 -> the old b[j] set serves as b[j-1], only b[j] is read
//     anything else -> both are read.
// The reads are ONE asm statement per set with the pairs as read-modify-write operands: a set that is not read keeps its
// registers, and the compiler sees no merge of a loaded and a kept value (which it answers with a copy per pair, or --
// with the sets as arrays -- by promoting a whole set to one 32-register tuple that is copied and spilled as a whole).
// The compiler's wait-count bookkeeping does not see these reads: set2_wait / set2_dep make the pairs operands of the
// wait, so that the arithmetic cannot be scheduled in front of it.
// ---- (generated text) carried register sets of accumulate_grouped_kernel, 4 outputs per lane, component stride 17 x 64 dwords
struct Set2_10 { f2v &a0, &a1, &a2, &a3, &a4, &a5, &a6, &a7, &a8, &a9, &b0, &b1, &b2, &b3, &b4, &b5, &b6, &b7, &b8, &b9; };
template <int SKIP> __device__ __forceinline__ void set2_read_10(int d, unsigned a, const Set2_10 &S)
{
    asm volatile("s_cmp_eq_u32 %21, %22\n\ts_cbranch_scc1 .Lkiwi_skip%=\n\t"
                 "ds_read2st64_b32 %0, %20 offset1:1\n\t"
                 "ds_read2st64_b32 %1, %20 offset0:17 offset1:18\n\t"
                 "ds_read2st64_b32 %2, %20 offset0:34 offset1:35\n\t"
                 "ds_read2st64_b32 %3, %20 offset0:136 offset1:137\n\t"
                 "ds_read2st64_b32 %4, %20 offset0:51 offset1:52\n\t"
                 "ds_read2st64_b32 %5, %20 offset0:68 offset1:69\n\t"
                 "ds_read2st64_b32 %6, %20 offset0:85 offset1:86\n\t"
                 "ds_read2st64_b32 %7, %20 offset0:102 offset1:103\n\t"
                 "ds_read2st64_b32 %8, %20 offset0:119 offset1:120\n\t"
                 "ds_read2st64_b32 %9, %20 offset0:153 offset1:154\n\t"
                 "ds_read2st64_b32 %10, %20 offset0:2 offset1:3\n\t"
                 "ds_read2st64_b32 %11, %20 offset0:19 offset1:20\n\t"
                 "ds_read2st64_b32 %12, %20 offset0:36 offset1:37\n\t"
                 "ds_read2st64_b32 %13, %20 offset0:138 offset1:139\n\t"
                 "ds_read2st64_b32 %14, %20 offset0:53 offset1:54\n\t"
                 "ds_read2st64_b32 %15, %20 offset0:70 offset1:71\n\t"
                 "ds_read2st64_b32 %16, %20 offset0:87 offset1:88\n\t"
                 "ds_read2st64_b32 %17, %20 offset0:104 offset1:105\n\t"
                 "ds_read2st64_b32 %18, %20 offset0:121 offset1:122\n\t"
                 "ds_read2st64_b32 %19, %20 offset0:155 offset1:156\n\t"
                 "\n.Lkiwi_skip%=:"
                 : "+v"(S.a0), "+v"(S.a1), "+v"(S.a2), "+v"(S.a3), "+v"(S.a4), "+v"(S.a5), "+v"(S.a6), "+v"(S.a7), "+v"(S.a8), "+v"(S.a9), "+v"(S.b0), "+v"(S.b1), "+v"(S.b2), "+v"(S.b3), "+v"(S.b4), "+v"(S.b5), "+v"(S.b6), "+v"(S.b7), "+v"(S.b8), "+v"(S.b9) : "v"(a), "s"(d), "i"(SKIP) : "memory", "scc");
}
__device__ __forceinline__ void set2_wait_10(const Set2_10 &S)
{
    asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(S.a0), "+v"(S.a1), "+v"(S.a2), "+v"(S.a3), "+v"(S.a4), "+v"(S.a5), "+v"(S.a6), "+v"(S.a7), "+v"(S.a8), "+v"(S.a9), "+v"(S.b0), "+v"(S.b1), "+v"(S.b2), "+v"(S.b3), "+v"(S.b4), "+v"(S.b5), "+v"(S.b6), "+v"(S.b7), "+v"(S.b8), "+v"(S.b9) :: "memory");
}
__device__ __forceinline__ void set2_dep_10(const Set2_10 &S)
{
    asm volatile("" : "+v"(S.a0), "+v"(S.a1), "+v"(S.a2), "+v"(S.a3), "+v"(S.a4), "+v"(S.a5), "+v"(S.a6), "+v"(S.a7), "+v"(S.a8), "+v"(S.a9), "+v"(S.b0), "+v"(S.b1), "+v"(S.b2), "+v"(S.b3), "+v"(S.b4), "+v"(S.b5), "+v"(S.b6), "+v"(S.b7), "+v"(S.b8), "+v"(S.b9) :: "memory");
}
__device__ __forceinline__ void set2_dead_10(const Set2_10 &S)
{
    asm volatile("" : "=v"(S.a0), "=v"(S.a1), "=v"(S.a2), "=v"(S.a3), "=v"(S.a4), "=v"(S.a5), "=v"(S.a6), "=v"(S.a7), "=v"(S.a8), "=v"(S.a9), "=v"(S.b0), "=v"(S.b1), "=v"(S.b2), "=v"(S.b3), "=v"(S.b4), "=v"(S.b5), "=v"(S.b6), "=v"(S.b7), "=v"(S.b8), "=v"(S.b9));
}
template <int I> __device__ __forceinline__ f2v &s2a(const Set2_10 &s) { if constexpr (I == 0) return s.a0; else if constexpr (I == 1) return s.a1; else if constexpr (I == 2) return s.a2; else if constexpr (I == 3) return s.a3; else if constexpr (I == 4) return s.a4; else if constexpr (I == 5) return s.a5; else if constexpr (I == 6) return s.a6; else if constexpr (I == 7) return s.a7; else if constexpr (I == 8) return s.a8; else return s.a9; }
template <int I> __device__ __forceinline__ f2v &s2b(const Set2_10 &s) { if constexpr (I == 0) return s.b0; else if constexpr (I == 1) return s.b1; else if constexpr (I == 2) return s.b2; else if constexpr (I == 3) return s.b3; else if constexpr (I == 4) return s.b4; else if constexpr (I == 5) return s.b5; else if constexpr (I == 6) return s.b6; else if constexpr (I == 7) return s.b7; else if constexpr (I == 8) return s.b8; else return s.b9; }
struct Set2_8 { f2v &a0, &a1, &a2, &a3, &a4, &a5, &a6, &a7, &b0, &b1, &b2, &b3, &b4, &b5, &b6, &b7; };
template <int SKIP> __device__ __forceinline__ void set2_read_8(int d, unsigned a, const Set2_8 &S)
{
    asm volatile("s_cmp_eq_u32 %17, %18\n\ts_cbranch_scc1 .Lkiwi_skip%=\n\t"
                 "ds_read2st64_b32 %0, %16 offset1:1\n\t"
                 "ds_read2st64_b32 %1, %16 offset0:17 offset1:18\n\t"
                 "ds_read2st64_b32 %2, %16 offset0:34 offset1:35\n\t"
                 "ds_read2st64_b32 %3, %16 offset0:51 offset1:52\n\t"
                 "ds_read2st64_b32 %4, %16 offset0:68 offset1:69\n\t"
                 "ds_read2st64_b32 %5, %16 offset0:85 offset1:86\n\t"
                 "ds_read2st64_b32 %6, %16 offset0:102 offset1:103\n\t"
                 "ds_read2st64_b32 %7, %16 offset0:119 offset1:120\n\t"
                 "ds_read2st64_b32 %8, %16 offset0:2 offset1:3\n\t"
                 "ds_read2st64_b32 %9, %16 offset0:19 offset1:20\n\t"
                 "ds_read2st64_b32 %10, %16 offset0:36 offset1:37\n\t"
                 "ds_read2st64_b32 %11, %16 offset0:53 offset1:54\n\t"
                 "ds_read2st64_b32 %12, %16 offset0:70 offset1:71\n\t"
                 "ds_read2st64_b32 %13, %16 offset0:87 offset1:88\n\t"
                 "ds_read2st64_b32 %14, %16 offset0:104 offset1:105\n\t"
                 "ds_read2st64_b32 %15, %16 offset0:121 offset1:122\n\t"
                 "\n.Lkiwi_skip%=:"
                 : "+v"(S.a0), "+v"(S.a1), "+v"(S.a2), "+v"(S.a3), "+v"(S.a4), "+v"(S.a5), "+v"(S.a6), "+v"(S.a7), "+v"(S.b0), "+v"(S.b1), "+v"(S.b2), "+v"(S.b3), "+v"(S.b4), "+v"(S.b5), "+v"(S.b6), "+v"(S.b7) : "v"(a), "s"(d), "i"(SKIP) : "memory", "scc");
}
__device__ __forceinline__ void set2_wait_8(const Set2_8 &S)
{
    asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(S.a0), "+v"(S.a1), "+v"(S.a2), "+v"(S.a3), "+v"(S.a4), "+v"(S.a5), "+v"(S.a6), "+v"(S.a7), "+v"(S.b0), "+v"(S.b1), "+v"(S.b2), "+v"(S.b3), "+v"(S.b4), "+v"(S.b5), "+v"(S.b6), "+v"(S.b7) :: "memory");
}
__device__ __forceinline__ void set2_dep_8(const Set2_8 &S)
{
    asm volatile("" : "+v"(S.a0), "+v"(S.a1), "+v"(S.a2), "+v"(S.a3), "+v"(S.a4), "+v"(S.a5), "+v"(S.a6), "+v"(S.a7), "+v"(S.b0), "+v"(S.b1), "+v"(S.b2), "+v"(S.b3), "+v"(S.b4), "+v"(S.b5), "+v"(S.b6), "+v"(S.b7) :: "memory");
}
__device__ __forceinline__ void set2_dead_8(const Set2_8 &S)
{
    asm volatile("" : "=v"(S.a0), "=v"(S.a1), "=v"(S.a2), "=v"(S.a3), "=v"(S.a4), "=v"(S.a5), "=v"(S.a6), "=v"(S.a7), "=v"(S.b0), "=v"(S.b1), "=v"(S.b2), "=v"(S.b3), "=v"(S.b4), "=v"(S.b5), "=v"(S.b6), "=v"(S.b7));
}
template <int I> __device__ __forceinline__ f2v &s2a(const Set2_8 &s) { if constexpr (I == 0) return s.a0; else if constexpr (I == 1) return s.a1; else if constexpr (I == 2) return s.a2; else if constexpr (I == 3) return s.a3; else if constexpr (I == 4) return s.a4; else if constexpr (I == 5) return s.a5; else if constexpr (I == 6) return s.a6; else return s.a7; }
template <int I> __device__ __forceinline__ f2v &s2b(const Set2_8 &s) { if constexpr (I == 0) return s.b0; else if constexpr (I == 1) return s.b1; else if constexpr (I == 2) return s.b2; else if constexpr (I == 3) return s.b3; else if constexpr (I == 4) return s.b4; else if constexpr (I == 5) return s.b5; else if constexpr (I == 6) return s.b6; else return s.b7; }

// ---- the same for a component stride of 9 x 64 dwords (512-sample tiles: two sources per workgroup, accumulate_multi_kernel)
template <int SKIP> __device__ __forceinline__ void set2_read_10_k9(int d, unsigned a, const Set2_10 &S)
{
    asm volatile("s_cmp_eq_u32 %21, %22\n\ts_cbranch_scc1 .Lkiwi_skip%=\n\t"
                 "ds_read2st64_b32 %0, %20 offset1:1\n\t"
                 "ds_read2st64_b32 %1, %20 offset0:9 offset1:10\n\t"
                 "ds_read2st64_b32 %2, %20 offset0:18 offset1:19\n\t"
                 "ds_read2st64_b32 %3, %20 offset0:72 offset1:73\n\t"
                 "ds_read2st64_b32 %4, %20 offset0:27 offset1:28\n\t"
                 "ds_read2st64_b32 %5, %20 offset0:36 offset1:37\n\t"
                 "ds_read2st64_b32 %6, %20 offset0:45 offset1:46\n\t"
                 "ds_read2st64_b32 %7, %20 offset0:54 offset1:55\n\t"
                 "ds_read2st64_b32 %8, %20 offset0:63 offset1:64\n\t"
                 "ds_read2st64_b32 %9, %20 offset0:81 offset1:82\n\t"
                 "ds_read2st64_b32 %10, %20 offset0:2 offset1:3\n\t"
                 "ds_read2st64_b32 %11, %20 offset0:11 offset1:12\n\t"
                 "ds_read2st64_b32 %12, %20 offset0:20 offset1:21\n\t"
                 "ds_read2st64_b32 %13, %20 offset0:74 offset1:75\n\t"
                 "ds_read2st64_b32 %14, %20 offset0:29 offset1:30\n\t"
                 "ds_read2st64_b32 %15, %20 offset0:38 offset1:39\n\t"
                 "ds_read2st64_b32 %16, %20 offset0:47 offset1:48\n\t"
                 "ds_read2st64_b32 %17, %20 offset0:56 offset1:57\n\t"
                 "ds_read2st64_b32 %18, %20 offset0:65 offset1:66\n\t"
                 "ds_read2st64_b32 %19, %20 offset0:83 offset1:84\n\t"
                 "\n.Lkiwi_skip%=:"
                 : "+v"(S.a0), "+v"(S.a1), "+v"(S.a2), "+v"(S.a3), "+v"(S.a4), "+v"(S.a5), "+v"(S.a6), "+v"(S.a7), "+v"(S.a8), "+v"(S.a9), "+v"(S.b0), "+v"(S.b1), "+v"(S.b2), "+v"(S.b3), "+v"(S.b4), "+v"(S.b5), "+v"(S.b6), "+v"(S.b7), "+v"(S.b8), "+v"(S.b9) : "v"(a), "s"(d), "i"(SKIP) : "memory", "scc");
}
template <int SKIP> __device__ __forceinline__ void set2_read_8_k9(int d, unsigned a, const Set2_8 &S)
{
    asm volatile("s_cmp_eq_u32 %17, %18\n\ts_cbranch_scc1 .Lkiwi_skip%=\n\t"
                 "ds_read2st64_b32 %0, %16 offset1:1\n\t"
                 "ds_read2st64_b32 %1, %16 offset0:9 offset1:10\n\t"
                 "ds_read2st64_b32 %2, %16 offset0:18 offset1:19\n\t"
                 "ds_read2st64_b32 %3, %16 offset0:27 offset1:28\n\t"
                 "ds_read2st64_b32 %4, %16 offset0:36 offset1:37\n\t"
                 "ds_read2st64_b32 %5, %16 offset0:45 offset1:46\n\t"
                 "ds_read2st64_b32 %6, %16 offset0:54 offset1:55\n\t"
                 "ds_read2st64_b32 %7, %16 offset0:63 offset1:64\n\t"
                 "ds_read2st64_b32 %8, %16 offset0:2 offset1:3\n\t"
                 "ds_read2st64_b32 %9, %16 offset0:11 offset1:12\n\t"
                 "ds_read2st64_b32 %10, %16 offset0:20 offset1:21\n\t"
                 "ds_read2st64_b32 %11, %16 offset0:29 offset1:30\n\t"
                 "ds_read2st64_b32 %12, %16 offset0:38 offset1:39\n\t"
                 "ds_read2st64_b32 %13, %16 offset0:47 offset1:48\n\t"
                 "ds_read2st64_b32 %14, %16 offset0:56 offset1:57\n\t"
                 "ds_read2st64_b32 %15, %16 offset0:65 offset1:66\n\t"
                 "\n.Lkiwi_skip%=:"
                 : "+v"(S.a0), "+v"(S.a1), "+v"(S.a2), "+v"(S.a3), "+v"(S.a4), "+v"(S.a5), "+v"(S.a6), "+v"(S.a7), "+v"(S.b0), "+v"(S.b1), "+v"(S.b2), "+v"(S.b3), "+v"(S.b4), "+v"(S.b5), "+v"(S.b6), "+v"(S.b7) : "v"(a), "s"(d), "i"(SKIP) : "memory", "scc");
}
// ---- ... and of 5 x 64 dwords (256-sample tiles: four sources per workgroup)
template <int SKIP> __device__ __forceinline__ void set2_read_10_k5(int d, unsigned a, const Set2_10 &S)
{
    asm volatile("s_cmp_eq_u32 %21, %22\n\ts_cbranch_scc1 .Lkiwi_skip%=\n\t"
                 "ds_read2st64_b32 %0, %20 offset1:1\n\t"
                 "ds_read2st64_b32 %1, %20 offset0:5 offset1:6\n\t"
                 "ds_read2st64_b32 %2, %20 offset0:10 offset1:11\n\t"
                 "ds_read2st64_b32 %3, %20 offset0:40 offset1:41\n\t"
                 "ds_read2st64_b32 %4, %20 offset0:15 offset1:16\n\t"
                 "ds_read2st64_b32 %5, %20 offset0:20 offset1:21\n\t"
                 "ds_read2st64_b32 %6, %20 offset0:25 offset1:26\n\t"
                 "ds_read2st64_b32 %7, %20 offset0:30 offset1:31\n\t"
                 "ds_read2st64_b32 %8, %20 offset0:35 offset1:36\n\t"
                 "ds_read2st64_b32 %9, %20 offset0:45 offset1:46\n\t"
                 "ds_read2st64_b32 %10, %20 offset0:2 offset1:3\n\t"
                 "ds_read2st64_b32 %11, %20 offset0:7 offset1:8\n\t"
                 "ds_read2st64_b32 %12, %20 offset0:12 offset1:13\n\t"
                 "ds_read2st64_b32 %13, %20 offset0:42 offset1:43\n\t"
                 "ds_read2st64_b32 %14, %20 offset0:17 offset1:18\n\t"
                 "ds_read2st64_b32 %15, %20 offset0:22 offset1:23\n\t"
                 "ds_read2st64_b32 %16, %20 offset0:27 offset1:28\n\t"
                 "ds_read2st64_b32 %17, %20 offset0:32 offset1:33\n\t"
                 "ds_read2st64_b32 %18, %20 offset0:37 offset1:38\n\t"
                 "ds_read2st64_b32 %19, %20 offset0:47 offset1:48\n\t"
                 "\n.Lkiwi_skip%=:"
                 : "+v"(S.a0), "+v"(S.a1), "+v"(S.a2), "+v"(S.a3), "+v"(S.a4), "+v"(S.a5), "+v"(S.a6), "+v"(S.a7), "+v"(S.a8), "+v"(S.a9), "+v"(S.b0), "+v"(S.b1), "+v"(S.b2), "+v"(S.b3), "+v"(S.b4), "+v"(S.b5), "+v"(S.b6), "+v"(S.b7), "+v"(S.b8), "+v"(S.b9) : "v"(a), "s"(d), "i"(SKIP) : "memory", "scc");
}
template <int SKIP> __device__ __forceinline__ void set2_read_8_k5(int d, unsigned a, const Set2_8 &S)
{
    asm volatile("s_cmp_eq_u32 %17, %18\n\ts_cbranch_scc1 .Lkiwi_skip%=\n\t"
                 "ds_read2st64_b32 %0, %16 offset1:1\n\t"
                 "ds_read2st64_b32 %1, %16 offset0:5 offset1:6\n\t"
                 "ds_read2st64_b32 %2, %16 offset0:10 offset1:11\n\t"
                 "ds_read2st64_b32 %3, %16 offset0:15 offset1:16\n\t"
                 "ds_read2st64_b32 %4, %16 offset0:20 offset1:21\n\t"
                 "ds_read2st64_b32 %5, %16 offset0:25 offset1:26\n\t"
                 "ds_read2st64_b32 %6, %16 offset0:30 offset1:31\n\t"
                 "ds_read2st64_b32 %7, %16 offset0:35 offset1:36\n\t"
                 "ds_read2st64_b32 %8, %16 offset0:2 offset1:3\n\t"
                 "ds_read2st64_b32 %9, %16 offset0:7 offset1:8\n\t"
                 "ds_read2st64_b32 %10, %16 offset0:12 offset1:13\n\t"
                 "ds_read2st64_b32 %11, %16 offset0:17 offset1:18\n\t"
                 "ds_read2st64_b32 %12, %16 offset0:22 offset1:23\n\t"
                 "ds_read2st64_b32 %13, %16 offset0:27 offset1:28\n\t"
                 "ds_read2st64_b32 %14, %16 offset0:32 offset1:33\n\t"
                 "ds_read2st64_b32 %15, %16 offset0:37 offset1:38\n\t"
                 "\n.Lkiwi_skip%=:"
                 : "+v"(S.a0), "+v"(S.a1), "+v"(S.a2), "+v"(S.a3), "+v"(S.a4), "+v"(S.a5), "+v"(S.a6), "+v"(S.a7), "+v"(S.b0), "+v"(S.b1), "+v"(S.b2), "+v"(S.b3), "+v"(S.b4), "+v"(S.b5), "+v"(S.b6), "+v"(S.b7) : "v"(a), "s"(d), "i"(SKIP) : "memory", "scc");
}
template <int NG> struct Set2Sel;
template <> struct Set2Sel<10> { typedef Set2_10 type; };
template <> struct Set2Sel<8> { typedef Set2_8 type; };
// (the set is NOT read when d == SKIP: the comparison happens inside the asm statement on the scalar d -- a flag computed
// outside reaches an "s" operand through a vector register)
template <int K, int SKIP> __device__ __forceinline__ void set2_read(int d, unsigned a, const Set2_10 &S)
{
    if constexpr (K == 17) set2_read_10<SKIP>(d, a, S); else if constexpr (K == 9) set2_read_10_k9<SKIP>(d, a, S); else set2_read_10_k5<SKIP>(d, a, S);
}
template <int K, int SKIP> __device__ __forceinline__ void set2_read(int d, unsigned a, const Set2_8 &S)
{
    if constexpr (K == 17) set2_read_8<SKIP>(d, a, S); else if constexpr (K == 9) set2_read_8_k9<SKIP>(d, a, S); else set2_read_8_k5<SKIP>(d, a, S);
}
__device__ __forceinline__ void set2_wait(const Set2_10 &S) { set2_wait_10(S); }
__device__ __forceinline__ void set2_wait(const Set2_8 &S) { set2_wait_8(S); }
__device__ __forceinline__ void set2_dep(const Set2_10 &S) { set2_dep_10(S); }
__device__ __forceinline__ void set2_dep(const Set2_8 &S) { set2_dep_8(S); }
__device__ __forceinline__ void set2_dead(const Set2_10 &S) { set2_dead_10(S); }
__device__ __forceinline__ void set2_dead(const Set2_8 &S) { set2_dead_8(S); }

template <int N, int I = 0, class F> __device__ __forceinline__ void static_for(F &&f)
{
    if constexpr (I < N) { f(std::integral_constant<int, I>{}); static_for<N, I + 1>(f); }
}

// All GF components of one centroid from the register sets L (b[j-1]) and H (b[j]), reference order (centroid_apply_hd's
// operations); a: LDS byte address of b[j-1] of the lane's first output in component 0; coef: the centroid's coefficient line
// (wave-uniform pointer: scalar loads, SGPR operands of the packed multiplies).
template <int NG, bool ROT, int K = 17>
__device__ __forceinline__ void carry2_apply(f2v (&ar1)[2], f2v (&ar2)[2], f2v (&dz)[2], const typename Set2Sel<NG>::type &L,
                                             const typename Set2Sel<NG>::type &H, unsigned a,
                                             int dh, int dl /* previous shift position minus this one (none: 0x7fff): 1 keeps H, -1 keeps L */,
                                             const float *__restrict__ coef, float cl, float sl)
{
    constexpr int nH1 = (NG == 10) ? 4 : 3;      // components summed into the radial trace
    float cw[2 * NG];
#pragma unroll
    for (int i = 0; i < 2 * NG; i++) cw[i] = coef[i];
    static_assert(K == 17 || K == 9 || K == 5, "component stride in units of 64 dwords");
    set2_read<K, 1>(dh, a + 4, H);            // shift + 1 (d == 1): the b[j] set is in place
    set2_read<K, -1>(dl, a, L);               // shift - 1: the b[j-1] set is
    set2_wait(H);
    set2_dep(L);
    f2v t1[2], t2[2];
#pragma unroll
    for (int k = 0; k < 2; k++) { t1[k] = ROT ? f2v{ 0.f, 0.f } : ar1[k]; t2[k] = ROT ? f2v{ 0.f, 0.f } : ar2[k]; }
    static_for<NG>([&](auto I) __attribute__((always_inline)) {
        constexpr int i = decltype(I)::value;
        const f2v c1 = { cw[coef_wl<NG>(i)], cw[coef_wl<NG>(i)] }, c2 = { cw[coef_wr<NG>(i)], cw[coef_wr<NG>(i)] };
        // (t1 / t2 start from 0 + product HERE, unlike the assembly routine: written as (c1 x) + (c2 y) the contracted build may fuse
        // either product into the add, and the kernels must round alike under `fused` -- found by the randomised sweep, ng = 8)
        if constexpr (i < nH1) {
            t1[0] = t1[0] + c1 * s2a<i>(H); t1[0] = t1[0] + c2 * s2a<i>(L);
            t1[1] = t1[1] + c1 * s2b<i>(H); t1[1] = t1[1] + c2 * s2b<i>(L);
        } else if constexpr (i < nH1 + 2) {
            t2[0] = t2[0] + c1 * s2a<i>(H); t2[0] = t2[0] + c2 * s2a<i>(L);
            t2[1] = t2[1] + c1 * s2b<i>(H); t2[1] = t2[1] + c2 * s2b<i>(L);
        } else {
            dz[0] = dz[0] + c1 * s2a<i>(H); dz[0] = dz[0] + c2 * s2a<i>(L);
            dz[1] = dz[1] + c1 * s2b<i>(H); dz[1] = dz[1] + c2 * s2b<i>(L);
        }
        if constexpr (i == nH1 + 1) {
#pragma unroll
            for (int k = 0; k < 2; k++) {
                if (ROT) {
                    ar1[k] = ar1[k] + cl * t1[k] - sl * t2[k];
                    ar2[k] = ar2[k] + cl * t2[k] + sl * t1[k];
                } else {
                    ar1[k] = t1[k]; ar2[k] = t2[k];
                }
            }
        }
    });
}

template <int NG>
__device__ __forceinline__ typename Set2Sel<NG>::type make_set2(f2v &a0, f2v &a1, f2v &a2, f2v &a3, f2v &a4, f2v &a5, f2v &a6, f2v &a7, f2v &a8, f2v &a9,
                                                                f2v &b0, f2v &b1, f2v &b2, f2v &b3, f2v &b4, f2v &b5, f2v &b6, f2v &b7, f2v &b8, f2v &b9)
{
    if constexpr (NG == 10) return Set2_10{ a0, a1, a2, a3, a4, a5, a6, a7, a8, a9, b0, b1, b2, b3, b4, b5, b6, b7, b8, b9 };
    else return Set2_8{ a0, a1, a2, a3, a4, a5, a6, a7, b0, b1, b2, b3, b4, b5, b6, b7 };
}

// ---- the apply of one centroid group as a hand-allocated assembly routine (accumulate_multi_kernel; accumulate_grouped_kernel for
// workgroups of one source)
#include "kiwi_apply_asm.inc"
#include "kiwi_apply_steps_asm.inc"     // (generated at build time: Makefile, tools/gen_apply_asm.py steps)
// Scalar loads whose only purpose is to bring 512 bytes behind p into the scalar data cache.  Nothing waits for them; the
// register they all write must stay allocated until they have returned (the caller keeps it live across the build).
__device__ __forceinline__ int coef_warm(const float *p)
{
    int d;
    asm volatile("s_load_dword %0, %1, 0x0\n\ts_load_dword %0, %1, 0x40\n\ts_load_dword %0, %1, 0x80\n\ts_load_dword %0, %1, 0xc0\n\t"
                 "s_load_dword %0, %1, 0x100\n\ts_load_dword %0, %1, 0x140\n\ts_load_dword %0, %1, 0x180\n\ts_load_dword %0, %1, 0x1c0"
                 : "=&s"(d) : "s"(p) : "memory");
    return d;
}
#if KIWI_ARITH == 1
#define KIWI_APPLY_ASM(NGV, KV, RV) apply_group_asm_##NGV##_k##KV##_##RV##_fused
#define KIWI_APPLY_PLAN(NGV, KV, RV) apply_steps_asm_##NGV##_k##KV##_##RV##_fused
#else
#define KIWI_APPLY_ASM(NGV, KV, RV) apply_group_asm_##NGV##_k##KV##_##RV##_exact
#define KIWI_APPLY_PLAN(NGV, KV, RV) apply_steps_asm_##NGV##_k##KV##_##RV##_exact
#endif

template <int NG, int T, bool FUSE, bool RUNS, bool COMPACT /* `tab` holds compact descriptors, four ints per record (geometry_kernel's off4; desc_expand), not 128-int rows */>
__global__ __launch_bounds__(T) __attribute__((amdgpu_waves_per_eu(3))) void accumulate_grouped_kernel(
    const float *__restrict__ G, const int2 *__restrict__ span, int pitch,
    const GeoRec *__restrict__ recs, const int *__restrict__ cent_ofs, int isrc0, int nrec,
    const RecvDev *__restrict__ recv, float *__restrict__ syn, size_t syn_stride, int ntiles,
    const int *__restrict__ tab, const float *__restrict__ coefs, const int *__restrict__ run_first, FuseParams fp,
    const int *__restrict__ pairflag /* see geometry_kernel */,
    int pairsel /* 0 all pairs, 1 not the cell kernel's, 3 not the duo kernel's */,
    const int *__restrict__ mate, const int *__restrict__ mate4 /* pairsel 3: groups of two / four sources accumulate_multi_kernel takes */,
    const int *__restrict__ synrow /* optional: sources that share another source's synthetics are not synthesised */,
    const int *__restrict__ fam_ofs, const int *__restrict__ fam_list /* FUSE with synrow: the sources that share source s's
                                          synthetics, fam_list[fam_ofs[s] .. fam_ofs[s + 1]): compared here with their moments */)
{
    constexpr bool compact = COMPACT;
    // run_first != nullptr: blockIdx.x indexes RUNS of consecutive trial sources [run_first[b], run_first[b+1]) that the
    // host found to have identical centroid geometry (same points and times: only the moment tensors differ, e.g. a
    // strike/dip/rake grid at a fixed location) and to consist of a single centroid group each.  The blended tiles
    // are then built ONCE and every source of the run is applied from them -- the sharing across trial sources
    // SURVEY.md 8d asks to report separately.  Per-source operations and their order are unchanged.
    constexpr int TILE = 4 * T;                          // samples per workgroup, 4 consecutive per thread
    constexpr int LDS_TILE = TILE + kHalo;
    __shared__ __attribute__((aligned(16))) float tiles[NG][LDS_TILE];
    // SOURCE index fastest in dispatch order: the workgroups resident at any moment are the same
    // (tile, receiver) of many neighbouring trial sources, which read (nearly) the same GF rows at
    // the same time, and blocks b, b+8, ... share an XCD and therefore its L2 (dispatch is
    // round-robin over the 8 XCDs; speed only, never correctness).  Measured alternative: giving each XCD a
    // contiguous eighth of this order (all sources of one (tile, receiver) on ONE XCD, eight different
    // (tile, receiver) sets in flight) is 4 % slower at cfg3 and 6 % at cfg4 -- eight L2s holding the same few rows
    // cost nothing, eight times as many distinct rows in flight load the Infinity Fabric.
    const int s = RUNS ? run_first[blockIdx.x] : (int)blockIdx.x;               // first (or only) source of this workgroup
    const int s_end = RUNS ? run_first[blockIdx.x + 1] : s + 1;
    const bool multi = RUNS && s_end - s > 1;
    const int tile = blockIdx.y % ntiles, r = blockIdx.y / ntiles;
    const RecvDev &rv = recv[r];
    if (!rv.enabled) return;
    if (tile * TILE >= rv.wlen) return;
    if (pairsel == 1 && cell_pair(rv, pairflag, s, nrec, r)) return;
    if (pairsel == 3 && (multi_taken_fwd<4>(rv, pairflag, mate4, s, nrec, r) || multi_taken_fwd<2>(rv, pairflag, mate, s, nrec, r))) return;
    if (synrow && !multi && synrow[s] != s) return;  // (in a run the sources that share synthetics are left out one by one)
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int t_tile0 = rv.wbeg + tile * TILE;
    const int cb = cent_ofs[isrc0], c0 = cent_ofs[isrc0 + s], nc = cent_ofs[isrc0 + s + 1] - c0;
    const GeoRec *__restrict__ rc = recs + ((size_t)(c0 - cb) * nrec + (size_t)r * nc);
    const int *__restrict__ tc = tab + ((size_t)(c0 - cb) * nrec + (size_t)r * nc) * (compact ? 4 : 128);
    const bool need_h = rv.need_h != 0, has_d = rv.has_d != 0;
    const float sd = rv.sd;

    f2v ar1[2] = { { 0.f, 0.f }, { 0.f, 0.f } }, ar2[2] = { { 0.f, 0.f }, { 0.f, 0.f } }, dz[2] = { { 0.f, 0.f }, { 0.f, 0.f } };
    // rotation to N/E, signs and store of one source's accumulators (seismogram.f90:256-283)
    auto store = [&](int js) {
        // (run + fused comparator: the lane's window position and the reference / taper addresses built on it are recomputed per
        // source from an opaque copy of the thread index -- kept across the group loop as invariants they were spilled to scratch)
        int tid_s = tid;
        if constexpr (RUNS && FUSE) asm volatile("" : "+v"(tid_s));
        const int tl = tile * TILE + 4 * (tid_s & ~63) + (tid_s & 63);     // window sample of the lane's output q = 0; q-th: + 64 q
        if (!FUSE && tl >= rv.wlen) return;
        float *__restrict__ so = syn + (size_t)js * syn_stride + tl;
        float mom = 0.f;
        if constexpr (FUSE) mom = fp.moment[fp.isrc0 + js];
        const bool whole = tile * TILE + TILE <= rv.wlen;
        for (int k = 0; k < rv.ncomp; k++) {
            f2v o01, o23;
            out4(rv.comp[k], rv.sign[k], rv.cl0, rv.sl0, ar1, ar2, dz, o01, o23);
            if constexpr (!FUSE) {
                const float o[4] = { o01.x, o01.y, o23.x, o23.y };
#pragma unroll
                for (int i = 0; i < 4; i++)
                    if (tl + 64 * i < rv.wlen) so[rv.synofs[k] + 64 * i] = o[i];      // 256 contiguous bytes per wave and store
                continue;
            }
            // ---- fused comparator, then a wave reduction; the partial of (source, slot, tile, wave) is summed by
            // misfit_finish_kernel in a fixed order
            double acc = fused_acc4(fp, o01, o23, mom, fp.reft + rv.refofs[k] + tl, fp.tw + rv.refofs[k] + tl, tl, rv.wlen, whole);
            acc = wave_reduce_f64(acc, fp.method == 6);                 // total in lane 63
            if (lane == 63)
                fp.partial[((size_t)js * fp.nmis + rv.slot0 + k) * fp.nparts + tile * (T / 64) + (tid >> 6)] = acc;
        }
    };
    // a source and, with the fused comparator, the sources that share its synthetics (other moments; minimizer_engine.f90:516-521)
    auto store_family = [&](int js) {
        __builtin_amdgcn_s_setprio(1);                   // (the epilogue's loads of reference and taper first: cfg2 12.62 -> 12.48 ms)
        store(js);
        __builtin_amdgcn_s_setprio(0);
        if constexpr (FUSE) {
            if (fam_ofs)
                for (int q = fam_ofs[js]; q < fam_ofs[js + 1]; q++) store(fam_list[q]);
        }
    };
    bool stored = false;
    int c = 0;
    int cur = rec_load(rc, 0, nc, lane);                 // record c, lane-distributed
    int ta = 0, tb = 0;                                  // load descriptors of record c (a rejected trial source has no centroids, no rows)
    // (compact form: `ta` carries the four offsets until desc_expand at the top of the group, next to its head record)
    if (nc > 0) { if constexpr (compact) ta = off4_load(tc, 0, lane); else { ta = tc[lane]; tb = tc[64 + lane]; } }
    // carried register sets (see set2_read): the common case of 256-thread workgroups
    constexpr bool kCarry = (T == 256);
    f2v xa0, xa1, xa2, xa3, xa4, xa5, xa6, xa7, xa8, xa9, xb0, xb1, xb2, xb3, xb4, xb5, xb6, xb7, xb8, xb9;
    f2v ya0, ya1, ya2, ya3, ya4, ya5, ya6, ya7, ya8, ya9, yb0, yb1, yb2, yb3, yb4, yb5, yb6, yb7, yb8, yb9;
    typedef typename Set2Sel<NG>::type SetT;
    const SetT X = make_set2<NG>(xa0, xa1, xa2, xa3, xa4, xa5, xa6, xa7, xa8, xa9, xb0, xb1, xb2, xb3, xb4, xb5, xb6, xb7, xb8, xb9);
    const SetT Y = make_set2<NG>(ya0, ya1, ya2, ya3, ya4, ya5, ya6, ya7, ya8, ya9, yb0, yb1, yb2, yb3, yb4, yb5, yb6, yb7, yb8, yb9);
    while (c < nc) {
        GeoRec g0;
        rec_head(cur, 0, g0);
        if (g0.row[0] < 0) {                             // 'cycle' on a missing trace
            c++;
            int lane_c = lane;                           // (opaque copy, run + fused comparator: see the carried path below)
            if constexpr (RUNS && FUSE) asm volatile("" : "+v"(lane_c));
            cur = rec_load(rc, c, nc, lane_c);
            if (c < nc) { if constexpr (compact) ta = off4_load(tc, c, lane); else { ta = tc[(size_t)c * 128 + lane]; tb = tc[(size_t)c * 128 + 64 + lane]; } }
            continue;
        }
        if constexpr (compact) desc_expand(ta, cur, lane, pitch, ta, tb);
        // ---- the group starting here (hint computed by geometry_kernel)
        const int cend = c + (g0.pad & 0xff);
        const int smax = g0.ishift + ((g0.pad >> 8) & 0xff), smin = g0.ishift - ((g0.pad >> 16) & 0xff);
        // LDS position p holds blended trace sample jb + p
        const int jb = t_tile0 - smax - 1;
        const int npos = TILE + (smax - smin) + 8;       // positions read by the group (<= LDS_TILE)
        const bool direct = (g0.flags & 1) != 0;
        // end indices of the blended traces (tail rule); their minima over the horizontal / vertical components
        // come precomputed from geometry_kernel so that no per-component branching is needed here
        int jend[NG];
#pragma unroll
        for (int ig = 0; ig < NG; ig++) jend[ig] = REC_I(ta, 40 + ig);
        const int jend_h = REC_I(ta, 50), jend_d = REC_I(ta, 51);
        const int jend_min = min(need_h ? jend_h : 0x7fffffff, has_d ? jend_d : 0x7fffffff);
        // carried register sets: receivers with horizontal and vertical components, every component added, no tail rule
        // anywhere in the tile for any shift of the group; the group's cos / sin of the back-azimuth change and its flags are
        // those of its head record (same point, same receiver), its integer shifts come in one load (lane k = centroid c + k)
        bool carry_grp = false;
        int ishv = 0, cur_next = 0;
        float gcl = 0.f, gsl = 0.f;
        if constexpr (kCarry) {
            carry_grp = need_h && has_d && !(g0.flags & 8) && !((jb + (smax - smin) + TILE) > jend_min);
            if (carry_grp) {
                // (run + fused comparator: the lane index of these two loads through an opaque copy -- the record array's base plus the
                // lane's offset, a loop invariant, was the last register that instantiation spilled)
                int lane_o = lane;
                if constexpr (RUNS && FUSE) asm volatile("" : "+v"(lane_o));
                if (lane_o < (g0.pad & 0xff)) ishv = rc[c + lane_o].ishift;
                cur_next = rec_load(rc, cend, nc, lane_o);
                gcl = REC_F(cur, 16); gsl = REC_F(cur, 17);
            }
        }
        // the build phase first (see accumulate_multi_kernel: cfg3-scatter 38.9 -> 37.6 ms); not in runs of sources, where one
        // build serves many applies (cfg2: 12.46 -> 12.60 with it)
        if constexpr (!RUNS) __builtin_amdgcn_s_setprio(1);
        {
            float *tile0 = &tiles[0][0];
            // descriptors are relative to the first row of the group's cell (64-bit base, see write_tab)
            const float *__restrict__ Gg = G + (size_t)g0.row[0] * (size_t)pitch;
            // all 40 rows of the group cover [jb, jb + LDS_TILE) inside their padded storage?  (lane l < 40 holds
            // row l's descriptors; workgroup-uniform because every wave holds the same table)
            const bool lane_ok = lane >= 4 * NG || (ta + jb >= tb && ta + jb + LDS_TILE <= tb + pitch);
            const bool fast = __builtin_amdgcn_ballot_w64(lane_ok) == ~0ull;
#define BUILD_B(IGS, P) do { \
                if (fast) { if (direct) build_batch<false, true>(tile0, LDS_TILE, IGS, P, jb, Gg, pitch, ta, tb, g0); \
                            else        build_batch<true, true>(tile0, LDS_TILE, IGS, P, jb, Gg, pitch, ta, tb, g0); } \
                else      { if (direct) build_batch<false, false>(tile0, LDS_TILE, IGS, P, jb, Gg, pitch, ta, tb, g0); \
                            else        build_batch<true, false>(tile0, LDS_TILE, IGS, P, jb, Gg, pitch, ta, tb, g0); } \
            } while (0)
            constexpr int H1 = NG / 2;
            int igA[H1], igB[NG - H1];
#pragma unroll
            for (int q = 0; q < H1; q++) igA[q] = q;
#pragma unroll
            for (int q = 0; q < NG - H1; q++) igB[q] = H1 + q;
            const int igH10[6] = { 0, 1, 2, 3, 4, 8 }, igD10[4] = { 5, 6, 7, 9 };      // horizontals / vertical only
            const int igH8[5] = { 0, 1, 2, 3, 4 }, igD8[3] = { 5, 6, 7 };
            // halo: pair q = (component slot, chunk) -> lanes; kHaloIter passes cover 16 * (number of components) pairs.
            // T = 256: one pass, component-major.  T < 256 (short windows): chunk-major -- a group reads only the first few chunks
            // behind the tile (its shift range + 8 samples), so the FIRST pass holds all of them for shift ranges up to
            // 4 T / ncmp - 8 samples; only that pass travels with the main loads (16 registers), the others -- rare -- are
            // loaded and stored one after the other behind them (three passes in flight cost 48 registers and spilled)
            constexpr int kHaloIter = (16 * NG + T - 1) / T;
            constexpr bool kHaloChunkMajor = T < 256;
            const int ncmp = (need_h && has_d) ? NG : (need_h ? (NG == 10 ? 6 : 5) : (NG == 10 ? 4 : 3));
            // (the lane's halo slot is recomputed per group from a copy of the thread index the compiler cannot see through: hoisted
            // out of the group loop as loop invariants, the LDS and row offsets derived from it were the registers the run + fused-
            // comparator instantiations spilled)
            int tid_h = tid;
            if constexpr (RUNS && FUSE) asm volatile("" : "+v"(tid_h));
            auto halo_lane = [&](int it, int &ig_out, int &ph_out) __attribute__((always_inline)) {
                const int q = tid_h + it * T;
                const int slot = kHaloChunkMajor ? q % ncmp : q >> 4, chunk = kHaloChunkMajor ? q / ncmp : q & 15;
                int ig = slot;                                            // all components: slot = component
                if (!(need_h && has_d)) {
                    if (need_h) ig = (slot == 5) ? 8 : slot;              // 0 1 2 3 4 8
                    else        ig = (NG == 10 && slot == 3) ? 9 : 5 + slot;   // 5 6 7 9
                }
                ig_out = min(ig, NG - 1);
                ph_out = TILE + 4 * min(chunk, 15);
                return slot < ncmp && chunk < 16 && ph_out < npos;
            };
            constexpr int kHaloLive = kHaloChunkMajor ? 1 : kHaloIter;   // passes in flight with the main loads
            bool hact[kHaloLive];
            int hig[kHaloLive], hph[kHaloLive];
            HaloRegs hr[kHaloLive];
#pragma unroll
            for (int it = 0; it < kHaloLive; it++) hact[it] = halo_lane(it, hig[it], hph[it]);
#define HALO_ISSUE() do { _Pragma("unroll") for (int it = 0; it < kHaloLive; it++) { \
                if (fast) { if (direct) hr[it] = halo_issue<false, true>(hact[it], hig[it], hph[it], jb, Gg, pitch, ta, tb); \
                            else        hr[it] = halo_issue<true, true>(hact[it], hig[it], hph[it], jb, Gg, pitch, ta, tb); } \
                else      { if (direct) hr[it] = halo_issue<false, false>(hact[it], hig[it], hph[it], jb, Gg, pitch, ta, tb); \
                            else        hr[it] = halo_issue<true, false>(hact[it], hig[it], hph[it], jb, Gg, pitch, ta, tb); } } } while (0)
#define HALO_FINISH() do { _Pragma("unroll") for (int it = 0; it < kHaloLive; it++) { \
                if (direct) halo_finish<false>(hact[it], hr[it], tile0, LDS_TILE, hig[it], hph[it], g0); \
                else        halo_finish<true>(hact[it], hr[it], tile0, LDS_TILE, hig[it], hph[it], g0); } \
                if constexpr (kHaloChunkMajor) { \
                    /* the passes behind the first, where the group's shifts reach that far (workgroup-uniform) */ \
                    for (int it = 1; it < kHaloIter && 4 * ((it * T) / ncmp) < npos - TILE; it++) { \
                        int ig_, ph_; \
                        const bool act_ = halo_lane(it, ig_, ph_); \
                        HaloRegs h_; \
                        if (direct) { h_ = halo_issue<false, false>(act_, ig_, ph_, jb, Gg, pitch, ta, tb); halo_finish<false>(act_, h_, tile0, LDS_TILE, ig_, ph_, g0); } \
                        else        { h_ = halo_issue<true, false>(act_, ig_, ph_, jb, Gg, pitch, ta, tb); halo_finish<true>(act_, h_, tile0, LDS_TILE, ig_, ph_, g0); } \
                    } } } while (0)
            if (need_h && has_d) {
                // streamed: NG / 2 sub-batches of two components, two in flight (see pair_issue)
                constexpr int NP = NG / 2;
#define STREAM(BL, FA) do { \
                    f4u va[2][BL ? 4 : 1], vb[2][BL ? 4 : 1]; \
                    pair_issue<BL, FA>(va, 0, 4 * tid, jb, Gg, pitch, ta, tb); \
                    pair_issue<BL, FA>(vb, 2, 4 * tid, jb, Gg, pitch, ta, tb); \
                    __syncthreads();        /* the tiles are free: every wave has applied the previous group (see multi_build) */ \
                    _Pragma("unroll") for (int i = 0; i < NP; i++) { \
                        __builtin_amdgcn_sched_barrier(0); \
                        if ((i & 1) == 0) { pair_finish<BL>(va, tile0, LDS_TILE, 2 * i, 4 * tid, g0); \
                                            if (i + 2 < NP) pair_issue<BL, FA>(va, 2 * (i + 2), 4 * tid, jb, Gg, pitch, ta, tb); } \
                        else              { pair_finish<BL>(vb, tile0, LDS_TILE, 2 * i, 4 * tid, g0); \
                                            if (i + 2 < NP) pair_issue<BL, FA>(vb, 2 * (i + 2), 4 * tid, jb, Gg, pitch, ta, tb); } \
                        if (i == NP - 3) HALO_ISSUE(); \
                    } } while (0)
                if (fast) { if (direct) STREAM(false, true); else STREAM(true, true); }
                else      { if (direct) STREAM(false, false); else STREAM(true, false); }
#undef STREAM
                HALO_FINISH();
            } else if (need_h) {
                HALO_ISSUE();
                __syncthreads();
                if constexpr (NG == 10) BUILD_B(igH10, 4 * tid); else BUILD_B(igH8, 4 * tid);
                HALO_FINISH();
            } else {
                HALO_ISSUE();
                __syncthreads();
                if constexpr (NG == 10) BUILD_B(igD10, 4 * tid); else BUILD_B(igD8, 4 * tid);
                HALO_FINISH();
            }
#undef HALO_ISSUE
#undef HALO_FINISH
#undef BUILD_B
        }
        // descriptors of the NEXT group: in flight while this group is applied
        if (cend < nc) { if constexpr (compact) ta = off4_load(tc, cend, lane); else { ta = tc[(size_t)cend * 128 + lane]; tb = tc[(size_t)cend * 128 + 64 + lane]; } }
        __syncthreads();
        if constexpr (!RUNS) __builtin_amdgcn_s_setprio(0);
        if (kCarry && carry_grp) {
            // ---- apply with carried register sets: the two sets swap roles at EVERY centroid (pairs of centroids, roles
            // static): after a centroid L holds its b[j-1] and H its b[j]; with the roles swapped, shift + 1 finds b[j] in place
            // and reads b[j-1], shift - 1 finds b[j-1] in place and reads b[j]; every other step reads both.  The rotating /
            // plain branch (seismogram.f90:160-203 / :205-231) is the same for the whole group: two copies of the loop.
            // In a run (RUNS: geometry-identical sources sharing these tiles) source after source, the carried sets passing from
            // the last centroid of one to the first of the next (shift - k + 1 steps back: for two time steps per source the set
            // that is in place again); accumulators and coefficient rows per source.
            const unsigned abase = (unsigned)(size_t)(lds_cfp)&tiles[0][4 * (tid & ~63) + lane];
            if constexpr ((NG == 10 || NG == 8) && !RUNS) {
                // one source per workgroup: the whole group in the hand-allocated assembly routine of accumulate_multi_kernel
                // (kiwi_apply_asm.inc; component stride 17 x 64 dwords here).  cfg3-scatter 39.0 -> 37.0 ms per 1024 sources.
                const size_t crow = ((size_t)(cent_ofs[isrc0 + s] - cb) * nrec + (size_t)r * nc + c) * kCoefLine;
                const unsigned clo = __builtin_amdgcn_readfirstlane((unsigned)crow), chi = __builtin_amdgcn_readfirstlane((unsigned)(crow >> 32));
                const float *__restrict__ coef_u = coefs + (((size_t)chi << 32) | clo);
                const float gcl_u = __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(gcl))), gsl_u = __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(gsl)));
                const int n = cend - c;
                static_assert(!kCarry || LDS_TILE == 17 * 64, "component stride of the assembly routine");
                if constexpr (NG == 10) {
                    if (g0.flags & 2) KIWI_APPLY_ASM(10, 17, rot)(ar1[0], ar1[1], ar2[0], ar2[1], dz[0], dz[1], abase, ishv, smax, n, coef_u, gcl_u, gsl_u);
                    else              KIWI_APPLY_ASM(10, 17, plain)(ar1[0], ar1[1], ar2[0], ar2[1], dz[0], dz[1], abase, ishv, smax, n, coef_u, gcl_u, gsl_u);
                } else {
                    if (g0.flags & 2) KIWI_APPLY_ASM(8, 17, rot)(ar1[0], ar1[1], ar2[0], ar2[1], dz[0], dz[1], abase, ishv, smax, n, coef_u, gcl_u, gsl_u);
                    else              KIWI_APPLY_ASM(8, 17, plain)(ar1[0], ar1[1], ar2[0], ar2[1], dz[0], dz[1], abase, ishv, smax, n, coef_u, gcl_u, gsl_u);
                }
                cur = cur_next;
            } else {
            int eprev = 0;
            bool have = false;
#define KIWI_C2STEP(LL, HH, RV, CC) do { \
                const int e = smax - __builtin_amdgcn_readlane(ishv, (CC) - c);      /* LDS position of b[j-1] of the tile's first sample */ \
                const int d = have ? eprev - e : 0x7fff; \
                /* `same`: the sets are in the roles of the previous step (first centroid of a source behind a source with an odd \
                   number of centroids): both are in place when the shift has not moved, none otherwise */ \
                const int dh = same ? (d == 0 ? 1 : 0x7fff) : d, dl = same ? (d == 0 ? -1 : 0x7fff) : d; \
                same = false; \
                carry2_apply<NG, RV>(ar1, ar2, dz, LL, HH, abase + 4u * (unsigned)e, dh, dl, coef_grp + (size_t)((CC) - c) * kCoefLine, gcl, gsl); \
                have = true; eprev = e; } while (0)
#define KIWI_C2SOURCES(RV) do { \
                set2_dead(X); set2_dead(Y);       /* nothing is carried into a group, its first centroid reads both sets: tells the register allocator so */ \
                for (int js = s; js < s_end; js++) { \
                    if (multi) { \
                        ar1[0] = ar1[1] = ar2[0] = ar2[1] = dz[0] = dz[1] = f2v{ 0.f, 0.f }; \
                        if (synrow && synrow[js] != js) continue;       /* evaluated with the source it shares synthetics with */ \
                    } \
                    const size_t crow = ((size_t)(cent_ofs[isrc0 + js] - cb) * nrec + (size_t)r * nc + c) * kCoefLine; \
                    const unsigned clo = __builtin_amdgcn_readfirstlane((unsigned)crow), chi = __builtin_amdgcn_readfirstlane((unsigned)(crow >> 32)); \
                    const float *__restrict__ coef_grp = coefs + (((size_t)chi << 32) | clo); \
                    int cc = c; \
                    /* odd count in a run: the sets end in the roles they started in, and the next source's first centroid finds \
                       them so (point sources of ONE centroid: no LDS read at all behind the first source of the run) */ \
                    bool same = RUNS && multi && have && ((cend - c) & 1); \
                    for (; cc + 1 < cend; cc += 2) { KIWI_C2STEP(X, Y, RV, cc); KIWI_C2STEP(Y, X, RV, cc + 1); } \
                    if (cc < cend) KIWI_C2STEP(X, Y, RV, cc); \
                    if (multi) store_family(js); \
                } } while (0)
            if (g0.flags & 2) KIWI_C2SOURCES(true); else KIWI_C2SOURCES(false);
#undef KIWI_C2SOURCES
#undef KIWI_C2STEP
            cur = cur_next;
            }
        } else
        // ---- apply: every centroid of the group, in table order (seismogram.f90:131); in a run, source after source
        for (int js = s; js < s_end; js++) {
        const GeoRec *__restrict__ rcj = multi ? recs + ((size_t)(cent_ofs[isrc0 + js] - cb) * nrec + (size_t)r * nc) : rc;
        // first record of the NEXT source of the run: in flight while this one is applied
        int cur_next_src = 0;
        if (multi) {
            if (js + 1 < s_end) {
                int lane_o = lane;               // (opaque copy, run + fused comparator: see the carried path above)
                if constexpr (RUNS && FUSE) asm volatile("" : "+v"(lane_o));
                cur_next_src = rec_load(recs + ((size_t)(cent_ofs[isrc0 + js + 1] - cb) * nrec + (size_t)r * nc), c, nc, lane_o);
            }
            ar1[0] = ar1[1] = ar2[0] = ar2[1] = dz[0] = dz[1] = f2v{ 0.f, 0.f };
            if (synrow && synrow[js] != js) { cur = cur_next_src; continue; }      // evaluated with the source it shares synthetics with
        }
        // coefficient rows of the group's centroids: wave-uniform by construction; readfirstlane tells the compiler so
        // (-> scalar address arithmetic and scalar loads of the coefficients)
        const size_t crow = ((size_t)(cent_ofs[isrc0 + js] - cb) * nrec + (size_t)r * nc + c) * kCoefLine;
        const unsigned clo = __builtin_amdgcn_readfirstlane((unsigned)crow), chi = __builtin_amdgcn_readfirstlane((unsigned)(crow >> 32));
        const float *__restrict__ coef_grp = coefs + (((size_t)chi << 32) | clo);
        for (int cc = c; cc < cend; cc++) {
            const int nxt = rec_load(rcj, cc + 1, nc, lane);     // prefetch the next record
            constexpr int ro = 0;
            const int ishift = REC_I(cur, ro + 8);
            // (the interpolation fraction and the six weights are read from the record only by the variants that use them:
            // with scalar-loaded coefficients and no tail rule they are not needed at all)
            const float cl = REC_F(cur, ro + 16), sl = REC_F(cur, ro + 17);
            const int flags = REC_I(cur, ro + 18);
            const float *__restrict__ coef = coef_grp + (size_t)(cc - c) * kCoefLine;
            const int e = smax - ishift;                 // LDS position of b[j-1] of the tile's first sample
            const int u0 = 4 * (tid & ~63) + lane;       // this lane's first tile sample (the others: + 64 q)
            const TileBase chunk0 = tile_base(&tiles[0][e + u0]);
            const int jl = jb + e + u0;                  // trace index of b[j-1] of the lane's output q = 0
            const bool tail = (jb + e + TILE) > jend_min;        // workgroup-uniform
#define APPLY(TV) do { \
                if (need_h && has_d && !(flags & 8)) centroid_apply_hd<NG, LDS_TILE, TV, !(FUSE && RUNS)>(ar1, ar2, dz, chunk0, jl, jend, flags, coef, cur, sd, cl, sl); \
                else centroid_apply<NG, LDS_TILE, TV>(ar1, ar2, dz, chunk0, jl, jend, need_h, has_d, flags, \
                                                      REC_F(cur, 9), sd, REC_F(cur, 10), REC_F(cur, 11), REC_F(cur, 12), REC_F(cur, 13), \
                                                      REC_F(cur, 14), REC_F(cur, 15), cl, sl); } while (0)
            if (!tail) APPLY(false); else APPLY(true);
#undef APPLY
            cur = nxt;
        }
        if (multi) { store_family(js); cur = cur_next_src; }
        }
        stored = multi;
        c = cend;                                        // (the barrier in front of the next group's LDS writes stands in its build)
    }
    if (!multi) store_family(s);
    else if (!stored) {                                  // every centroid skipped: the run's synthetics are zero
        ar1[0] = ar1[1] = ar2[0] = ar2[1] = dz[0] = dz[1] = f2v{ 0.f, 0.f };
        for (int js = s; js < s_end; js++)
            if (!(synrow && synrow[js] != js)) store_family(js);
    }
}

template <bool BLEND, bool FAST, typename D>
__device__ __forceinline__ void one_issue(f4u (&v)[BLEND ? 4 : 1], int ig, int p, int jb, const float *__restrict__ G,
                                          int pitch, const D &d)
{
    const int j = jb + p;
#pragma unroll
    for (int k = 0; k < (BLEND ? 4 : 1); k++) {
        const int base = d.a(ig, k);
        if constexpr (FAST) {
            v[k] = buf_load4(gf_rsrc(G), p, base + jb);
        } else {
            const int lo = d.b(ig, k);
            const int idx = min(max(base + j, lo), lo + pitch - 4);
            v[k] = *(const f4u *)(G + (size_t)(unsigned)idx);
        }
    }
}

// The same loads as one_issue<true, true>, hidden from the compiler's wait-count bookkeeping.  Left to itself the compiler puts an
// `s_waitcnt vmcnt(0)` in front of the second and the third wave-task's loads (the registers of a task the wave does not have are
// reused for a flag on that path, and its pass then drains every load in flight): the tasks' rows came in two or three L2 round
// trips one after the other instead of one (per-CU event trace, round 5: 1800 cycles from the first load to the barrier behind the
// last one).  As assembly statements the loads are just register definitions to the compiler; the wait for a task's rows is the
// statement vm_wait<>, which takes the task's registers as operands so that nothing that uses them can be scheduled in front of it.
// vmcnt counts loads in flight and they return in order: vm_wait<4 k> lets the k wave-tasks issued behind this one stay in flight
// (a load the compiler issues in between -- the group's integer shifts in shadow() -- makes the wait one load stricter, never weaker).
template <typename D>
__device__ __forceinline__ void one_issue_hidden(f4u (&v)[4], int ig, int p, int jb, const float *__restrict__ G, const D &d)
{
    const size_t gi = (size_t)G;
    const v4i_t rs = { (int)(unsigned)gi, (int)((unsigned)(gi >> 32) & 0xffffu), -1, 0x00020000 };      // (= gf_rsrc(G))
    const int voff = (int)(4u * (unsigned)p);
#pragma unroll
    for (int k = 0; k < 4; k++) {
        const int soff = (int)(4u * (unsigned)(d.a(ig, k) + jb));
        asm volatile("buffer_load_dwordx4 %0, %1, %2, %3 offen" : "=v"(v[k]) : "v"(voff), "s"(rs), "s"(soff));
    }
}
// The same for descriptors that are linear in the component (DescPlan): t[k] = a(0, k) + jb, formed once per group and kept from the
// compiler's reassociation by the caller, leaves an add and a shift per load (three scalar instructions as the sum of four terms).
__device__ __forceinline__ void one_issue_hidden_linear(f4u (&v)[4], int igp /* ig pitch */, int p, const float *__restrict__ G, const int (&t)[4])
{
    const size_t gi = (size_t)G;
    const v4i_t rs = { (int)(unsigned)gi, (int)((unsigned)(gi >> 32) & 0xffffu), -1, 0x00020000 };      // (= gf_rsrc(G))
    const int voff = (int)(4u * (unsigned)p);
#pragma unroll
    for (int k = 0; k < 4; k++) {
        const int soff = (int)(4u * (unsigned)(t[k] + igp));
        asm volatile("buffer_load_dwordx4 %0, %1, %2, %3 offen" : "=v"(v[k]) : "v"(voff), "s"(rs), "s"(soff));
    }
}
// (ONE statement per task, the choice between the two counts inside it: two statements on the two sides of a branch would each be a
// definition of the task's registers, and the compiler joins them through copies placed in FRONT of the wait -- copies of
// registers whose loads are still in flight)
template <int CNT_FULL, int CNT_SHORT>
__device__ __forceinline__ void vm_wait(f4u (&v)[4], int full /* wave-uniform: 0 -> CNT_SHORT */)
{
    if constexpr (CNT_FULL == CNT_SHORT)
        asm volatile("s_waitcnt vmcnt(%4)" : "+v"(v[0]), "+v"(v[1]), "+v"(v[2]), "+v"(v[3]) : "n"(CNT_FULL));
    else
        asm volatile("s_cmp_eq_u32 %6, 0\n\ts_cbranch_scc1 1f\n\ts_waitcnt vmcnt(%4)\n\ts_branch 2f\n1:\n\ts_waitcnt vmcnt(%5)\n2:"
                     : "+v"(v[0]), "+v"(v[1]), "+v"(v[2]), "+v"(v[3]) : "n"(CNT_FULL), "n"(CNT_SHORT), "s"(full) : "scc");
}

template <bool BLEND>
__device__ __forceinline__ void one_finish(const f4u (&v)[BLEND ? 4 : 1], float *__restrict__ tile0, int lds_tile, int ig, int p,
                                           const GeoRec &g)
{
    f4u b;
    if constexpr (BLEND) {
        b = g.w[0] * v[0];                    // gfdb.f90:946-949, summed in this order
        b = b + g.w[1] * v[1];
        b = b + g.w[2] * v[2];
        b = b + g.w[3] * v[3];
    } else {
        b = v[0];
    }
    *(float4 *)(tile0 + ig * lds_tile + p) = make_float4(b.x, b.y, b.z, b.w);
}

// ---- the blend of four sources on the matrix pipe (exact contract, NS = 4; round 5; built with -DKIWI_MFMA_BLEND=1, NOT the default) ----
// Measured (make EXTRA=-DKIWI_MFMA_BLEND=1): results bit-identical to the vector-pipe blend (the GPU parity suite passes unchanged), and the
// kernel is SLOWER: cfg3 114.8 -> 126.0 ms per 4096 sources, cfg3-100pt 47.6 -> 56.0 ms per 512.  The wave's own build is no shorter -- 16
// matrix instructions of two passes each stand where 32 packed multiplies stood, the adds wait for them chunk by chunk, and the rows cost
// four times the load instructions --; what the other waves gain from the freer vector pipe (the blend's multiplies are 7 % of the kernel
// with them removed altogether) does not pay for it.
#ifndef KIWI_MFMA_BLEND
#define KIWI_MFMA_BLEND 0
#endif
// v_mfma_f32_4x4x1_16b_f32 computes, in each of 16 blocks of four lanes, D[i][j] = A[i] * B[j] + C[i][j] -- K = 1: ONE product and
// one rounding.  With C = -0 that is fma(a, b, -0), the separately rounded product a * b for every input (a non-zero product is
// unchanged by adding -0, +0 + -0 = +0, -0 + -0 = -0; checked on the hardware against v_mul_f32 over 16.8 M random bit patterns,
// zeros, denormals, infinities and NaNs included: profiles/microbench/mfma_product.hip).  Operands: lane 4 b + i supplies A[b][i],
// lane 4 b + j supplies B[b][j], register r of lane 4 b + j receives D[b][r][j].  With A = one register of raw samples (one sample
// per lane, 64 consecutive samples of a node row) and B = that node's blend weight of source j = lane & 3, ONE instruction yields
// the four sources' products for 64 samples, lane 4 b + j holding source j's for samples 4 b .. 4 b + 3 in four consecutive
// registers: exactly the 16 bytes that lane then writes into source j's tile set.  The adds stay on the vector pipe, in the
// reference's order ((w0 v0 + w1 v1) + w2 v2) + w3 v3 (gfdb.f90:946-949) -- 6 packed adds per 64 samples and four sources where
// the vector pipe alone needs 16 packed multiplies + 12 packed adds (56 -> 24 packed instructions per wave-task; the matrix pipe
// takes 16 instructions in their place and runs beside the vector pipe).  The price: the rows come in as one sample per lane, four
// dword loads per row and task where one 16-byte load did.
typedef float f4m __attribute__((ext_vector_type(4)));
struct RowsDw { float r[4][4]; };      // [node][64-sample chunk] of one wave-task: lane l holds sample 64 m + l of the slab

// the 16 loads of a wave-task, hidden from the compiler's wait-count bookkeeping like one_issue_hidden's
template <typename D>
__device__ __forceinline__ void rows_issue_dw(RowsDw &v, int ig, int lane, int jb, const float *__restrict__ G, const D &d)
{
    const size_t gi = (size_t)G;
    const v4i_t rs = { (int)(unsigned)gi, (int)((unsigned)(gi >> 32) & 0xffffu), -1, 0x00020000 };      // (= gf_rsrc(G))
    const int voff = (int)(4u * (unsigned)lane);
#pragma unroll
    for (int k = 0; k < 4; k++) {
        const int soff = (int)(4u * (unsigned)(d.a(ig, k) + jb));
        asm volatile("buffer_load_dword %0, %1, %2, %3 offen" : "=v"(v.r[k][0]) : "v"(voff), "s"(rs), "s"(soff));
        asm volatile("buffer_load_dword %0, %1, %2, %3 offen offset:256" : "=v"(v.r[k][1]) : "v"(voff), "s"(rs), "s"(soff));
        asm volatile("buffer_load_dword %0, %1, %2, %3 offen offset:512" : "=v"(v.r[k][2]) : "v"(voff), "s"(rs), "s"(soff));
        asm volatile("buffer_load_dword %0, %1, %2, %3 offen offset:768" : "=v"(v.r[k][3]) : "v"(voff), "s"(rs), "s"(soff));
    }
}
// the wait for a task's 16 registers (one statement, the choice between two counts inside it: see vm_wait)
template <int CNT_FULL, int CNT_SHORT>
__device__ __forceinline__ void vm_wait16(RowsDw &v, int full /* wave-uniform: 0 -> CNT_SHORT */)
{
#define KIWI_R16 "+v"(v.r[0][0]), "+v"(v.r[0][1]), "+v"(v.r[0][2]), "+v"(v.r[0][3]), "+v"(v.r[1][0]), "+v"(v.r[1][1]), "+v"(v.r[1][2]), "+v"(v.r[1][3]), \
                 "+v"(v.r[2][0]), "+v"(v.r[2][1]), "+v"(v.r[2][2]), "+v"(v.r[2][3]), "+v"(v.r[3][0]), "+v"(v.r[3][1]), "+v"(v.r[3][2]), "+v"(v.r[3][3])
    if constexpr (CNT_FULL == CNT_SHORT)
        asm volatile("s_waitcnt vmcnt(%16)" : KIWI_R16 : "n"(CNT_FULL));
    else
        asm volatile("s_cmp_eq_u32 %18, 0\n\ts_cbranch_scc1 1f\n\ts_waitcnt vmcnt(%16)\n\ts_branch 2f\n1:\n\ts_waitcnt vmcnt(%17)\n2:"
                     : KIWI_R16 : "n"(CNT_FULL), "n"(CNT_SHORT), "s"(full) : "scc");
#undef KIWI_R16
}
// blend of one wave-task for the four sources and the write into their tile sets; dst: the lane's first float of component 0
// in ITS source's set (source lane & 3, samples 4 (lane >> 2) ..), w[k]: node k's weight of that source
__device__ __forceinline__ void mfma_finish(const RowsDw &v, float *__restrict__ dst, const float (&w)[4], bool write)
{
    const f4m negz = { -0.f, -0.f, -0.f, -0.f };
#pragma unroll
    for (int m = 0; m < 4; m++) {
        f4m b = __builtin_amdgcn_mfma_f32_4x4x1f32(v.r[0][m], w[0], negz, 0, 0, 0);      // gfdb.f90:946-949, summed in this order
        b = b + __builtin_amdgcn_mfma_f32_4x4x1f32(v.r[1][m], w[1], negz, 0, 0, 0);
        b = b + __builtin_amdgcn_mfma_f32_4x4x1f32(v.r[2][m], w[2], negz, 0, 0, 0);
        b = b + __builtin_amdgcn_mfma_f32_4x4x1f32(v.r[3][m], w[3], negz, 0, 0, 0);
        if (write) *(float4 *)(dst + 64 * m) = make_float4(b.x, b.y, b.z, b.w);
    }
}

// floats from one tile set of accumulate_multi_kernel to the next: NS = 4 under KIWI_MFMA_BLEND pads by 8 so that the four lanes of a block -- which
// write the same position of the four sets (mfma_finish) -- fall into different LDS banks (ds_write_b128: groups of 8 consecutive lanes,
// bank = dword address mod 32: lanes 4 b + j of a group cover banks 8 j + 4 (b & 1) .. + 3)
template <int NG, int NS> __host__ __device__ constexpr int multi_set_stride() { return NG * (1024 / NS + kHalo) + ((NS == 4 && KIWI_MFMA_BLEND) ? 8 : 0); }

// (A/B: -DKIWI_MULTI_COEF_WARM=1 warms the coefficient lines of a group with plans too, as the record path does: measured as worth
// nothing, DESIGN 3.3)
#ifndef KIWI_MULTI_COEF_WARM
#define KIWI_MULTI_COEF_WARM 0
#endif

// whether wave `wv` has the last wave-task of multi_build (1) or not (0)
template <int NG, int NS> __device__ __forceinline__ int multi_last_task(int wv)
{
    // (wv is 0 .. 3: two sources per workgroup, or four and a multiple of four components, and every wave has every task)
    if constexpr (NS == 2 || NG % 4 == 0) return 1;
    constexpr int N = (NG + 3) / 4;                      // (NS = 4: tasks per wave at most)
    // (the sign bit of component - NG, not a comparison: a select on a wave-uniform condition is a vector instruction to the
    // compiler, and its result reaches an assembly statement's scalar operand in a vector register)
    return (int)((unsigned)(wv + 4 * (N - 1) - NG) >> 31);          // (NS = 4: the last task's component is wv + 4 (N - 1))
}

// Build of accumulate_multi_kernel: NS tile sets of TILE = 1024 / NS samples (+ halo).  A wave-task = one component's 64 main
// chunks (chunk = 4 samples) of one 256-sample slab; NS = 2: wave w takes components 2 i + (w >> 1), slab w & 1; NS = 4: wave w
// components w + 4 i (one slab); the halo chunks go to the LAST threads, chunk-major (thread 255 - q: chunk q / NG of component
// q % NG): a group reads only the first few chunks behind the tile (its shift range + 8 samples), so the halo is the work of the
// last wave alone -- the one with the fewest main tasks (NS = 4: 3, 3, 2, 2) --, `whalo` says whether this wave has any.  Every chunk's four node rows are loaded ONCE and
// blended with the weights of each source into its tile set (gfdb.f90:946-949, summed in this order) -- `only` >= 0: into that
// source's set alone.  A centroid exactly on a node carries the weights (1, 0, 0, 0) over four copies of its row:
// 1 v + 0 v + 0 v + 0 v is v bit for bit, so there is no unblended variant.
// `reweigh(gl)`: the blend weights once more (gl[].w), for the halo's blend.  It stands on the far side of a branch; weights it shares
// with the tasks in front of it reach it as 64-bit (w, w) pairs which the compiler lays out in the common block, two scalar moves per
// weight in EVERY wave, whereas weights that arrive inside the block are broadcast by the packed instructions' operand selects.  With
// plans (RW) reweigh() is NS scalar loads from lines the shadow's loads have just brought in, in the one wave that has halo lanes and
// the fewest tasks; without, the halo takes gw as before.  (The same for the last wave-task of the waves that have one was measured
// and costs time: those waves are the ones the barrier waits for, and the loads' round trip stands in their way -- DESIGN 3.3.)
// The lanes' halo test -- which lanes hold a halo chunk of this group -- comes from the caller as `hact` WITHOUT plans (!RW: it
// made `whalo` from it by a ballot; `hq`, `npos` and `reweigh` are unused) and is formed here, inside the halo's block, from `hq`, `hph`
// and `npos` WITH plans (RW: `hact` is unused, `whalo` is the caller's scalar compare): halo_lanes() below, the one place that knows.
template <int NG, bool FAST, int NS, bool RW, typename D, typename Shadow, typename Reweigh>
__device__ __forceinline__ void multi_build(float *__restrict__ tile0, int wv, int lane, int tid, int jb, const float *__restrict__ G,
                                            int pitch, const D &d, const GeoRec (&gw)[NS], int only, bool hact, bool whalo, int hig, int hph,
                                            int lastf /* multi_last_task(wv), in a scalar register */, int hq, int npos /* RW: hact is formed here */,
                                            Shadow shadow, Reweigh reweigh)
{
    constexpr int TILE = 1024 / NS, LDS_TILE = TILE + kHalo, DEPTH = 3, SET = multi_set_stride<NG, NS>();
    constexpr int N = (NS == 2) ? NG / 2 : (NG + 3) / 4;           // wave-tasks per wave at most
    const int p = (NS == 2) ? 4 * (64 * (wv & 1) + lane) : 4 * lane;
    auto comp = [&](int i) { return (NS == 2) ? 2 * i + (wv >> 1) : wv + 4 * i; };
    // (linear descriptors: the group's four row positions once, see one_issue_hidden_linear; opaque, or the compiler spreads the sum
    // over the loads again)
    int t[4] = { 0, 0, 0, 0 };
    if constexpr (FAST && D::linear) {
#pragma unroll
        for (int k = 0; k < 4; k++) { t[k] = d.a(0, k) + jb; asm("" : "+s"(t[k])); }
    }
    HaloRegs hv;
    // (a wave without a halo lane skips the halo; in the others inactive lanes load a valid chunk too: no merge of registers)
    if (whalo) hv = halo_issue<true, FAST>(true, hig, hph, jb, G, pitch, d);
    // (RW: formed HERE, in the one wave that has any halo lane, from a copy of `npos` the compiler cannot move: as a value of the
    // group's top it is a compare and two lane reads in every wave)
    auto halo_lanes = [&]() __attribute__((always_inline)) {
        if constexpr (RW) {
            int npos_o = npos;
            asm volatile("" : "+s"(npos_o));
            return hq < 16 * NG && hph < npos_o;
        } else return hact;
    };
    // (tasks 0 .. N - 2 exist in every wave, the last one only where its component does: NS = 4, NG = 10: waves 0 and 1)
    const bool last_ok = lastf != 0;
    if constexpr (KIWI_MFMA_BLEND && FAST && NS == 4 && KIWI_ARITH == 0) {
        // ---- the products of the blend on the matrix pipe (see mfma_finish); `only` >= 0: every lane blends, the lanes of that source write
        RowsDw v[N];
#pragma unroll
        for (int i = 0; i < DEPTH && i < N; i++) if (i < N - 1 || last_ok) rows_issue_dw(v[i], comp(i), lane, jb, G, d);
        __syncthreads();                                 // (as below)
        shadow();
        const int me = lane & 3;
        float w[4];
#pragma unroll
        for (int k = 0; k < 4; k++) w[k] = me == 0 ? gw[0].w[k] : (me == 1 ? gw[1].w[k] : (me == 2 ? gw[2].w[k] : gw[3].w[k]));
        float *__restrict__ dst = tile0 + me * SET + 4 * (lane >> 2);
        const bool write = only < 0 || only == me;
#pragma unroll
        for (int i = 0; i < N; i++) {
            __builtin_amdgcn_sched_barrier(0);
            if (i < N - 1 || last_ok) {
                const int behind = (i + DEPTH < N ? i + DEPTH : N) - 1 - i;
                const bool short_ = behind > 0 && i + DEPTH >= N;
                switch (behind) {
                case 0: vm_wait16<0, 0>(v[i], 1); break;
                case 1: if (short_) vm_wait16<16, 0>(v[i], lastf); else vm_wait16<16, 16>(v[i], 1); break;
                default: if (short_) vm_wait16<32, 16>(v[i], lastf); else vm_wait16<32, 32>(v[i], 1); break;
                }
                mfma_finish(v[i], dst + comp(i) * LDS_TILE, w, write);
            }
            if (i + DEPTH < N && (i + DEPTH < N - 1 || last_ok)) rows_issue_dw(v[i + DEPTH], comp(i + DEPTH), lane, jb, G, d);
        }
        if (whalo) {
            const bool hact_l = halo_lanes();
#pragma unroll
            for (int s = 0; s < NS; s++)
                if (only < 0 || only == s) halo_finish<true>(hact_l, hv, tile0 + s * SET, LDS_TILE, hig, hph, gw[s]);
        }
        return;
    }
    f4u v[N][4];
    auto issue = [&](int i) __attribute__((always_inline)) {
        if constexpr (FAST && D::linear) one_issue_hidden_linear(v[i], comp(i) * pitch, p, G, t);
        else if constexpr (FAST) one_issue_hidden(v[i], comp(i), p, jb, G, d);
        else one_issue<true, false>(v[i], comp(i), p, jb, G, pitch, d);
    };
#pragma unroll
    for (int i = 0; i < DEPTH && i < N; i++) if (i < N - 1 || last_ok) issue(i);
    // The barrier that frees the tile sets (every wave has applied the previous group) stands HERE, behind the first loads of
    // this group and in front of its first LDS write: a wave that is done applying has its loads in flight while it waits
    // for the others.  (Workgroup-uniform call: every wave takes the same variant of this function.)
    __syncthreads();
    // In the shadow of the loads (a round trip to L2 under load is ~1500 cycles in which this wave has nothing to issue): whatever
    // the caller needs later and the loads did not need -- the blend weights (gw[].w), the apply's parameters.
    shadow();
#pragma unroll
    for (int i = 0; i < N; i++) {
        __builtin_amdgcn_sched_barrier(0);
        if (i < N - 1 || last_ok) {
            if constexpr (FAST) {
                // wave-tasks in flight behind task i: i + 1 .. min(i + DEPTH, N) - 1, the last of them only where it exists
                // (i is a constant once the loop is unrolled: the switch folds to one statement)
                const int behind = (i + DEPTH < N ? i + DEPTH : N) - 1 - i;
                const bool short_ = behind > 0 && i + DEPTH >= N;         // (the window reaches the last task: one less where it is missing)
                switch (behind) {
                case 0: vm_wait<0, 0>(v[i], 1); break;
                case 1: if (short_) vm_wait<4, 0>(v[i], lastf); else vm_wait<4, 4>(v[i], 1); break;
                default: if (short_) vm_wait<8, 4>(v[i], lastf); else vm_wait<8, 8>(v[i], 1); break;
                }
            }
#pragma unroll
            for (int s = 0; s < NS; s++)
                if (only < 0 || only == s) one_finish<true>(v[i], tile0 + s * SET, LDS_TILE, comp(i), p, gw[s]);
        }
        if (i + DEPTH < N && (i + DEPTH < N - 1 || last_ok)) issue(i + DEPTH);
    }
    if (whalo) {
        if constexpr (RW) {
            GeoRec gl[NS];
            reweigh(gl);
            const bool hact_l = halo_lanes();
#pragma unroll
            for (int s = 0; s < NS; s++)
                if (only < 0 || only == s) halo_finish<true>(hact_l, hv, tile0 + s * SET, LDS_TILE, hig, hph, gl[s]);
        } else {
#pragma unroll
            for (int s = 0; s < NS; s++)
                if (only < 0 || only == s) halo_finish<true>(halo_lanes(), hv, tile0 + s * SET, LDS_TILE, hig, hph, gw[s]);
        }
    }
}


// ------------------------------------------------------------------------------------------------
// accumulate, several trial sources per workgroup (round 3)
//
// Measured on accumulate_grouped_kernel (cfg3, 1024 sources per launch): build phase alone 22.8 ms, apply phase alone
// 22.7 ms, together 38.6 ms -- and the build alone moves 713 GB from the L2s to the CUs (40 node rows of 1088 samples per
// group and workgroup) in those 22.8 ms: 31 TB/s of the ~34.5 TB/s the L2s deliver.  The build is bound by L2 bandwidth,
// the apply by vector issue, and a workgroup alternates between the two.  What shrinks the first: NEIGHBOURING trial sources
// of a grid search put their sub-faults into the same cells of the Green's function grid (a strike step of 0.1 degree moves a
// sub-fault by metres, the nodes are kilometres apart): the 40 node rows a group needs are the same for all of them, only
// the four blend weights differ.  This kernel gives a workgroup the same (receiver, tile) of NS = 2 or 4 CONSECUTIVE trial
// sources, tiles of 1024 / NS samples: every group's node rows are loaded ONCE and blended NS times, into a tile set per
// source (NS x (1024 / NS + 64) x NG floats of LDS: 46 / 51 KB, three workgroups per CU); each wave then applies the
// centroids of ONE of the sources from that source's tile set (carry2_apply, as accumulate_grouped_kernel).  Per output
// sample: 1 / NS of the L2 traffic and of the build's addresses, descriptors and loads (the blend arithmetic stays), the
// apply as before.  Where the sources' groups do NOT all sit in the same cell with the same tile origin, the workgroup
// builds the tile sets one after the other.
//
// Grouping (host, eval): aligned groups of NS sources of a chunk whose centroid tables have the same STRUCTURE -- same
// number of centroids, same boundaries of the centroid groups (group_len) -- so that they walk their groups in lockstep;
// `mate[k]` says so for group k.  Of those the kernel takes the (group, receiver) combinations where every source is "clean"
// for the receiver (horizontal and vertical components, no missing trace, no tail rule: pairflag of geometry_kernel);
// accumulate_grouped_kernel runs behind it for everything else (pairsel 3).
template <int NS>
__device__ __forceinline__ bool multi_taken(const RecvDev &rv, const int *__restrict__ pairflag, const int *__restrict__ mate,
                                            int s, int nrec, int r)
{
    if (!mate) return false;
    const int a = s - s % NS;
    if (!mate[a / NS] || !rv.need_h || !rv.has_d) return false;
    int f = 0;
#pragma unroll
    for (int i = 0; i < NS; i++) f |= pairflag[(size_t)(a + i) * nrec + r];
    return f == 0;
}

// ---- the plans of accumulate_multi_kernel (PlanSrc, kiwi_common.hpp).  At the top of every centroid group each of the kernel's waves
// used to derive the group's parameters from the head records of its NS sources: NS lane-distributed record loads, some thirty
// read-lanes, ballots over the sources' rows, the merge of their shift ranges, desc_expand's shuffle -- vector-pipe instructions all,
// the same in the four waves of the sixteen (NS = 4) tile workgroups of a (source group, receiver) pair.  Here ONE thread does it per
// (source group, receiver), once per evaluation, and walks the pair's centroid groups; the decisions are those of the kernel's own
// loop top (the !PLAN branch there), statement for statement.
template <int NS>
__global__ __launch_bounds__(64) void multi_plan_kernel(const GeoRec *__restrict__ recs, const int *__restrict__ cent_ofs, int isrc0, int nrec, int pitch,
    const RecvDev *__restrict__ recv, const int *__restrict__ off4, const int *__restrict__ pairflag, const int *__restrict__ mate,
    const int *__restrict__ mate_wider, const int *__restrict__ plan_ofs, int4 *__restrict__ plan,
    int regular_on /* 0: no plan is marked regular (KIWI_HIP_MULTI_REGULAR=0) */, int repeat_on /* 0: no plan names repeated shifts (KIWI_HIP_MULTI_REPEAT=0) */,
    unsigned *__restrict__ count /* debug: [0] += PlanSrc written, [1] += regular ones, [2] += ones with a repeat mask; or null */)
{
    constexpr int TILE = 1024 / NS, LDS_TILE = TILE + kHalo;
    const int k = (int)blockIdx.x, s0 = NS * k, r = (int)(blockIdx.y * 64 + threadIdx.x);
    if (r >= nrec) return;
    const RecvDev &rv = recv[r];
    if (!rv.enabled) return;
    if (!multi_taken<NS>(rv, pairflag, mate, s0, nrec, r)) return;
    if constexpr (NS == 2) { if (multi_taken<4>(rv, pairflag, mate_wider, s0, nrec, r)) return; }
    const int cb = cent_ofs[isrc0];
    const int nc = cent_ofs[isrc0 + s0 + 1] - cent_ofs[isrc0 + s0];
    const size_t pbeg = (size_t)plan_ofs[k], pend = (size_t)plan_ofs[k + 1];      // (the host counted the groups: nothing is written past them)
    size_t pi = pbeg + (size_t)r;
    for (int c = 0; c < nc && pi < pend; pi += (size_t)nrec) {
        const GeoRec *h[NS];
        int smaxs[NS], smins[NS], npos = 0;
        bool shared = true, same_rows = true;
#pragma unroll
        for (int i = 0; i < NS; i++) {
            h[i] = recs + ((size_t)(cent_ofs[isrc0 + s0 + i] - cb) * nrec + (size_t)r * nc + c);
            smaxs[i] = h[i]->ishift + ((h[i]->pad >> 8) & 0xff);
            smins[i] = h[i]->ishift - ((h[i]->pad >> 16) & 0xff);
            npos = max(npos, TILE + (smaxs[i] - smins[i]) + 8);
            if (i > 0) {
                same_rows = same_rows && h[i]->row[0] == h[0]->row[0] && h[i]->row[1] == h[0]->row[1] && h[i]->row[2] == h[0]->row[2] && h[i]->row[3] == h[0]->row[3];
                shared = shared && smaxs[i] == smaxs[0];
            }
        }
        shared = shared && same_rows;
        if (same_rows && !shared) {
            int smax_c = smaxs[0], smin_c = smins[0];
#pragma unroll
            for (int i = 1; i < NS; i++) { smax_c = max(smax_c, smaxs[i]); smin_c = min(smin_c, smins[i]); }
            if (TILE + (smax_c - smin_c) + 8 <= LDS_TILE) {
                shared = true;
                npos = TILE + (smax_c - smin_c) + 8;
#pragma unroll
                for (int i = 0; i < NS; i++) smaxs[i] = smax_c;
            }
        }
        const int glen = h[0]->pad & 0xff;
        int4 *__restrict__ out = plan + pi * (kPlanStride / 16);
        unsigned nreg = 0, nrep = 0;
#pragma unroll
        for (int i = 0; i < NS; i++) {
            const int4 o = *(const int4 *)(off4 + ((size_t)(cent_ofs[isrc0 + s0 + i] - cb) * nrec + (size_t)r * nc + c) * 4);
            // regular: the test the apply routine makes at every step (`s_cmp_lg_u32 d, 4`, tools/gen_apply_asm.py), made once here
            const int e0 = smaxs[i] - h[i]->ishift;
            bool regular = regular_on != 0 && e0 >= 0 && e0 <= kPlanE0Mask;
            // repeats: a group of at most five whose every step is its predecessor's shift + 1 or its predecessor's shift, bit j of the
            // mask: record j + 1 stays (PlanSrc::head) -- a step that stays needs no tile read, lines_repeat() of tools/gen_apply_asm.py
            bool steps01 = regular && repeat_on != 0 && glen <= 5;
            int repeats = 0;
            for (int j = 1; j < glen && c + j < nc; j++) {
                const int d = h[i][j].ishift - h[i][j - 1].ishift;
                regular = regular && d == 1;
                steps01 = steps01 && (d == 0 || d == 1);
                if (d == 0 && j <= 4) repeats |= 1 << (j - 1);
            }
            if (regular || !steps01) repeats = 0;
            nreg += regular ? 1u : 0u;
            nrep += repeats ? 1u : 0u;
            const int head = (h[i]->flags & 0xffff) | (regular || repeats ? (e0 << kPlanE0Shift) | (regular ? kPlanRegularBit : 0) | (repeats << kPlanRepeatShift) : 0)
                             | (glen << 16) | ((shared ? 1 : 0) << 23) | ((npos - TILE) << 24);
            // (rows 1 .. 3 as the kernel's build uses them, DescPlan::b0: the same 32-bit products it formed per group and wave)
            out[4 * i + 0] = make_int4(h[i]->row[0], (h[i]->row[1] - h[i]->row[0]) * pitch, (h[i]->row[2] - h[i]->row[0]) * pitch, (h[i]->row[3] - h[i]->row[0]) * pitch);
            out[4 * i + 1] = o;
            out[4 * i + 2] = make_int4(__float_as_int(h[i]->w[0]), __float_as_int(h[i]->w[1]), __float_as_int(h[i]->w[2]), __float_as_int(h[i]->w[3]));
            out[4 * i + 3] = make_int4(smaxs[i], head, __float_as_int(h[i]->cl), __float_as_int(h[i]->sl));
        }
        if (count) { atomicAdd(count, (unsigned)NS); atomicAdd(count + 1, nreg); atomicAdd(count + 2, nrep); }
        if (glen < 1) break;
        c += glen;
    }
}

typedef const __attribute__((address_space(4))) v4i_t *plan_cptr;
// Scalar loads whose only purpose is to bring the NS lines of a plan into the scalar data cache (see coef_warm).
template <int NS>
__device__ __forceinline__ int plan_warm(size_t p)
{
    int d;
    if constexpr (NS == 4)
        asm volatile("s_load_dword %0, %1, 0x0\n\ts_load_dword %0, %1, 0x40\n\ts_load_dword %0, %1, 0x80\n\ts_load_dword %0, %1, 0xc0" : "=&s"(d) : "s"(p) : "memory");
    else
        asm volatile("s_load_dword %0, %1, 0x0\n\ts_load_dword %0, %1, 0x40" : "=&s"(d) : "s"(p) : "memory");
    return d;
}

template <int NG, bool FUSE, int NS, bool COMPACT /* `tab` holds compact descriptors, four ints per record (geometry_kernel's off4; desc_expand), not 128-int rows */,
          bool PLAN /* the group loop's parameters come from multi_plan_kernel's plans (scalar loads), not from the head records */>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(3))) void accumulate_multi_kernel(
    const float *__restrict__ G, const int2 *__restrict__ span, int pitch,
    const GeoRec *__restrict__ recs, const int *__restrict__ cent_ofs, int isrc0, int nrec,
    const RecvDev *__restrict__ recv, float *__restrict__ syn, size_t syn_stride, int ntiles,
    const int *__restrict__ tab, const float *__restrict__ coefs, FuseParams fp, const int *__restrict__ pairflag, const int *__restrict__ mate,
    const int *__restrict__ mate_wider /* NS = 2: the groups of four the wider launch has taken (or null) */,
    const PlanSrc *__restrict__ plan, const int *__restrict__ plan_ofs /* PLAN: first plan of every source group (kiwi_common.hpp) */)
{
    constexpr bool compact = COMPACT;
    static_assert(NS == 2 || NS == 4, "sources per workgroup");
    static_assert(!PLAN || COMPACT, "plans hold compact descriptors");
    constexpr int TILE = 1024 / NS, LDS_TILE = TILE + kHalo, K = LDS_TILE / 64, WPS = 4 / NS;       // WPS: waves per source
    constexpr int SET = multi_set_stride<NG, NS>();
    __shared__ __attribute__((aligned(16))) float tiles[NS * SET];      // NS tile sets of NG rows of LDS_TILE floats
    const int s0 = NS * (int)blockIdx.x;                 // chunk-local sources s0 .. s0 + NS - 1
    const int tile = blockIdx.y % ntiles, r = blockIdx.y / ntiles;
    const RecvDev &rv = recv[r];
    if (!rv.enabled) return;
    if (tile * TILE >= rv.wlen) return;
    if (!multi_taken<NS>(rv, pairflag, mate, s0, nrec, r)) return;
    if constexpr (NS == 2) { if (multi_taken<4>(rv, pairflag, mate_wider, s0, nrec, r)) return; }
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int sh = wv / WPS;                             // the source this wave applies
    const int t_tile0 = rv.wbeg + tile * TILE;
    const int cb = cent_ofs[isrc0];
    const int nc = cent_ofs[isrc0 + s0 + 1] - cent_ofs[isrc0 + s0];      // (every source of the group has nc centroids)
    const size_t base_me = (size_t)(cent_ofs[isrc0 + s0 + sh] - cb) * nrec + (size_t)r * nc;
    const GeoRec *__restrict__ rc = recs + base_me;      // this wave's source
    const float sd = rv.sd;
    (void)sd;
    const int u0 = 256 * (wv % WPS) + lane;              // the lane's first sample of its source's tile (the others: + 64 q)

    f2v ar1[2] = { { 0.f, 0.f }, { 0.f, 0.f } }, ar2[2] = { { 0.f, 0.f }, { 0.f, 0.f } }, dz[2] = { { 0.f, 0.f }, { 0.f, 0.f } };
    f2v xa0, xa1, xa2, xa3, xa4, xa5, xa6, xa7, xa8, xa9, xb0, xb1, xb2, xb3, xb4, xb5, xb6, xb7, xb8, xb9;
    f2v ya0, ya1, ya2, ya3, ya4, ya5, ya6, ya7, ya8, ya9, yb0, yb1, yb2, yb3, yb4, yb5, yb6, yb7, yb8, yb9;
    typedef typename Set2Sel<NG>::type SetT;
    const SetT X = make_set2<NG>(xa0, xa1, xa2, xa3, xa4, xa5, xa6, xa7, xa8, xa9, xb0, xb1, xb2, xb3, xb4, xb5, xb6, xb7, xb8, xb9);
    const SetT Y = make_set2<NG>(ya0, ya1, ya2, ya3, ya4, ya5, ya6, ya7, ya8, ya9, yb0, yb1, yb2, yb3, yb4, yb5, yb6, yb7, yb8, yb9);

    // head records of the group starting at c of EVERY source, load descriptors of the first one, lane-distributed
    // (the record index of every source's first record as a scalar computed ONCE: left as an expression of cent_ofs[] the compiler
    // re-loads the offsets at every use -- a scalar-load round trip, and a drain of the LDS counter with it, per group and phase)
    long long rbase[NS];
#pragma unroll
    for (int i = 0; i < NS; i++) {
        const long long b = (long long)(cent_ofs[isrc0 + s0 + i] - cb) * nrec + (long long)r * nc;
        rbase[i] = ((long long)__builtin_amdgcn_readfirstlane((int)(b >> 32)) << 32) | (unsigned)__builtin_amdgcn_readfirstlane((int)b);
    }
    auto recs_of = [&](int i) { return recs + (size_t)rbase[i]; };
    auto tab_of = [&](int i) { return tab + (size_t)rbase[i] * (compact ? 4 : 128); };
    int c = 0;
    int cur[NS];
    int ta = 0, tb = 0;                                   // (compact form: `ta` carries the four offsets until desc_expand at the group's top)
    if constexpr (!PLAN) {
#pragma unroll
        for (int i = 0; i < NS; i++) cur[i] = rec_load(recs_of(i), 0, nc, lane);
        if constexpr (compact) ta = off4_load(tab_of(0), 0, lane);
        else { ta = tab_of(0)[lane]; tb = tab_of(0)[64 + lane]; }
    }
    // halo: one lane per (4-sample chunk, component), chunk-major from the last thread down (see multi_build)
    const int hq = 255 - tid, hch = min(hq / NG, 15), hig = hq % NG, hph = TILE + 4 * hch;
    // PLAN: this group's plan, a wave-uniform address in the constant address space (scalar loads); the next group's is kPlanStride nrec
    // bytes on ([centroid group][receiver])
    size_t pcur = 0;
    if constexpr (PLAN) {
        const size_t a = (size_t)plan + ((size_t)plan_ofs[blockIdx.x] + (size_t)r) * kPlanStride;
        pcur = ((size_t)(unsigned)__builtin_amdgcn_readfirstlane((int)(a >> 32)) << 32) | (unsigned)__builtin_amdgcn_readfirstlane((int)a);
    }
    const int pstep = nrec * kPlanStride;
    const int hoff = PLAN ? hig * pitch : 0;
    auto plan4 = [&](int byte) { return *(plan_cptr)(pcur + (size_t)(unsigned)byte); };
    // this wave's coefficient lines (80 bytes per step, consecutive): a scalar pointer that advances by the group's length -- as
    // (base_me + c) * kCoefLine it was a 64-bit product and a reload of `coefs` per group
    const float *__restrict__ coef_cur = nullptr;
    if constexpr (PLAN) {
        const size_t a = (size_t)(coefs + base_me * kCoefLine);
        coef_cur = (const float *)(((size_t)(unsigned)__builtin_amdgcn_readfirstlane((int)(a >> 32)) << 32) | (unsigned)__builtin_amdgcn_readfirstlane((int)a));
    }
    // halo lanes of this wave: thread 255 - q has chunk q / NG, so the wave's first halo chunk is that of its last thread,
    // q = 64 (3 - wv) -- the wave has a halo lane in a group that reads more than 4 * (that chunk) positions behind the tile
    const int lastf = PLAN ? __builtin_amdgcn_readfirstlane(multi_last_task<NG, NS>(wv)) : 0;      // (a scalar once: it was a lane read per wait)
    const int hq_wave = 64 * (3 - wv);
    const int hthr = hq_wave < 16 * NG ? 4 * (hq_wave / NG) : 0x7fffffff;
    while (c < nc) {
        GeoRec g[NS];
        int smaxs[NS], smins[NS], npos = 0;
        bool shared = true, same_rows = true;
        int glen_p = 0;
        int flags = 0, smax = 0;
        float gcl = 0.f, gsl = 0.f;
        DescPlan dp;
        if constexpr (PLAN) {
            // (the plan's address as the loop's own value: derived from the induction variable the compiler keeps ONE pointer 240
            // bytes into the plan and forms every line's address with an add and an add-with-carry in front of its load; an opaque
            // base leaves the lines' offsets to the loads' immediate fields)
            asm volatile("" : "+s"(pcur));
            // rows and offsets of the first source (of all of them where the build is shared) and this wave's own source's line
            // with the group's header (PlanSrc::head: glen, shared, npos are equal in all NS), its flags and rotation: three scalar
            // loads from lines multi_plan_kernel wrote and the previous group's shadow() brought into the scalar cache
            const v4i_t rw = plan4(0), of = plan4(16), me = plan4(64 * sh + 48);
            g[0].row[0] = rw.x;
            dp = DescPlan{ { 0, rw.y, rw.z, rw.w }, { of.x, of.y, of.z, of.w }, pitch, hoff };      // (PlanSrc::row: 1 .. 3 are offsets already)
            const unsigned head = (unsigned)me.y;
            glen_p = (int)((head >> 16) & 0x7fu);
            shared = ((head >> 23) & 1u) != 0u;
            npos = TILE + (int)(head >> 24);
            smax = me.x;
            flags = me.y & 0xffff; gcl = __int_as_float(me.z); gsl = __int_as_float(me.w);
            smaxs[0] = plan4(48).x;                          // (one dword: a branch around it for shared builds costs more than the load)
        }
        if constexpr (compact && !PLAN) desc_expand(ta, cur[0], lane, pitch, ta, tb);
        if constexpr (!PLAN) {
#pragma unroll
        for (int i = 0; i < NS; i++) {
            // of the head record: blend weights, integer shift and group hint of every source; the four node rows of the first
            // one only -- the others' are compared where they lie (lanes 0 .. 3 of the lane-distributed records)
            g[i].ishift = REC_I(cur[i], 8);                                   // (the weights: in the shadow of the build's loads)
            g[i].pad = REC_I(cur[i], 19);
            smaxs[i] = g[i].ishift + ((g[i].pad >> 8) & 0xff);
            smins[i] = g[i].ishift - ((g[i].pad >> 16) & 0xff);
            npos = max(npos, TILE + (smaxs[i] - smins[i]) + 8);
            // the node rows once for all -- if all sit in the same cell and read it from the same tile origin
            if (i == 0) g[0].row[0] = REC_I(cur[0], 0);
            else {
                same_rows = same_rows && (__builtin_amdgcn_ballot_w64(cur[i] != cur[0]) & 0xfull) == 0ull;
                shared = shared && smaxs[i] == smaxs[0];
            }
        }
        shared = shared && same_rows;
        if (same_rows && !shared) {
            // the sources of a time sweep: same cell, shifts a few samples apart.  ONE tile origin all the same -- that of the
            // largest shift -- when the shifts of all of them still fit the tile's halo; every source counts its positions from it
            int smax_c = smaxs[0], smin_c = smins[0];
#pragma unroll
            for (int i = 1; i < NS; i++) { smax_c = smax_u(smax_c, smaxs[i]); smin_c = smin_u(smin_c, smins[i]); }
            if (TILE + (smax_c - smin_c) + 8 <= LDS_TILE) {
                shared = true;
                npos = TILE + (smax_c - smin_c) + 8;
#pragma unroll
                for (int i = 0; i < NS; i++) smaxs[i] = smax_c;
            }
        }
        }
        const int glen = PLAN ? glen_p : (g[0].pad & 0xff);                // (same structure: equal for all)
        const int cend = c + glen;
        // this wave's source: what its apply needs (equal for all centroids of the group: same point, same receiver) -- fetched
        // in the shadow of the build's loads, like the blend weights
        if constexpr (!PLAN) {
            smax = smaxs[0];
#pragma unroll
            for (int i = 1; i < NS; i++) if (sh == i) smax = smaxs[i];
        }
        int ishv = 0, warm_ = 0, pwarm_ = 0;
        const float *__restrict__ coef_grp = coef_cur;
        auto shadow = [&]() {
            if constexpr (PLAN) {
                // the blend weights of every source: scalar loads (this wave's source's flags and rotation came with the group's header:
                // values the shadow defines reach the apply through vector registers, the build's variants being what they are)
#pragma unroll
                for (int i = 0; i < NS; i++) {
                    const v4i_t w = plan4(64 * i + 32);
                    g[i].w[0] = __int_as_float(w.x); g[i].w[1] = __int_as_float(w.y); g[i].w[2] = __int_as_float(w.z); g[i].w[3] = __int_as_float(w.w);
                }
                // the next group's plan on its way into the scalar cache (none behind the last group: nothing is read past the plans)
                if (c + glen < nc) pwarm_ = plan_warm<NS>(pcur + (size_t)(unsigned)pstep);
            } else {
#pragma unroll
            for (int i = 0; i < NS; i++) { g[i].w[0] = REC_F(cur[i], 4); g[i].w[1] = REC_F(cur[i], 5); g[i].w[2] = REC_F(cur[i], 6); g[i].w[3] = REC_F(cur[i], 7); }
            int curme = cur[0];
#pragma unroll
            for (int i = 1; i < NS; i++) if (sh == i) curme = cur[i];
            flags = REC_I(curme, 18);
            gcl = REC_F(curme, 16); gsl = REC_F(curme, 17);
            }
            // the group's integer shifts, lane k: step k -- not for a group the plan calls regular or whose repeats it names
            // (PlanSrc::head: its apply takes e0, the step count and those bits).  Wave-uniform: the waves of a workgroup may differ.
            // (the empty statement keeps the wave-uniform test a scalar branch of its own: merged with the lanes' test it is six
            // instructions of mask arithmetic in every group, also in those that skip the load)
            if (!(PLAN && (flags & (kPlanRegularBit | kPlanRepeatMask)))) { if constexpr (PLAN) asm volatile(""); if (lane < glen) ishv = rc[c + lane].ishift; }
            // this group's coefficient lines on their way into the scalar cache
            if constexpr (!PLAN) {
                const size_t crow = (base_me + c) * kCoefLine;
                const unsigned clo = __builtin_amdgcn_readfirstlane((unsigned)crow), chi = __builtin_amdgcn_readfirstlane((unsigned)(crow >> 32));
                coef_grp = coefs + (((size_t)chi << 32) | clo);
            }
            // (not with plans: measured as worth nothing there, DESIGN 3.3 -- eight scalar loads and a register held per group)
            if constexpr (NG == 10 && (!PLAN || KIWI_MULTI_COEF_WARM)) warm_ = coef_warm(coef_grp);
        };
        auto noshadow = []() {};
        // the blend weights once more for the halo's blend (see multi_build): from the plan through a copy of its address the compiler
        // cannot match with the shadow's loads
        auto reweigh = [&](GeoRec (&gl)[NS]) {
            if constexpr (PLAN) {
                size_t q = pcur;
                asm volatile("" : "+s"(q));
#pragma unroll
                for (int i = 0; i < NS; i++) {
                    const v4i_t w = *(plan_cptr)(q + (size_t)(unsigned)(64 * i + 32));
                    gl[i].w[0] = __int_as_float(w.x); gl[i].w[1] = __int_as_float(w.y); gl[i].w[2] = __int_as_float(w.z); gl[i].w[3] = __int_as_float(w.w);
                }
            }
        };
        // ---- build
        // (whether this wave has a halo lane in this group: with plans a scalar compare, else a vector compare over the lanes and a ballot)
#define KIWI_MULTI_BUILD(DESC, I0, ONLY, NPOS, SHADOW) do { \
            const int jb_ = t_tile0 - smaxs[I0] - 1;      /* LDS position p of a tile set holds its source's blended trace sample jb + p */ \
            const float *__restrict__ Gg = G + (size_t)g[I0].row[0] * (size_t)pitch; \
            const bool fast = (DESC).fast(jb_, LDS_TILE, pitch, lane, NG); \
            const bool hact = PLAN ? false : hq < 16 * NG && hph < (NPOS); \
            const bool whalo = PLAN ? (NPOS) - TILE > hthr : __builtin_amdgcn_ballot_w64(hact) != 0ull; \
            const int lastf_ = PLAN ? lastf : __builtin_amdgcn_readfirstlane(multi_last_task<NG, NS>(wv)); \
            if (fast) multi_build<NG, true, NS, PLAN>(&tiles[0], wv, lane, tid, jb_, Gg, pitch, DESC, g, ONLY, hact, whalo, hig, hph, lastf_, hq, NPOS, SHADOW, reweigh); \
            else      multi_build<NG, false, NS, PLAN>(&tiles[0], wv, lane, tid, jb_, Gg, pitch, DESC, g, ONLY, hact, whalo, hig, hph, lastf_, hq, NPOS, SHADOW, reweigh); } while (0)
        // A workgroup in its build phase is waiting for memory most of the time: its waves go first whenever they have an
        // instruction to issue (loads out early, the blend done as soon as the rows arrive), the workgroups that are applying
        // fill the rest of the issue slots.  Measured: cfg3 133.5 -> 127.2 ms per 4096 sources, cfg3-100pt 55.2 -> 51.3 (the
        // other way round -- apply first -- 137.8 / 57.5; priority 1, 2 and 3 alike).
        __builtin_amdgcn_s_setprio(1);
        if constexpr (PLAN) {
            if (shared) KIWI_MULTI_BUILD(dp, 0, -1, npos, shadow);
            else {
                KIWI_MULTI_BUILD(dp, 0, 0, npos, shadow);
#pragma unroll
                for (int i = 1; i < NS; i++) {           // (rows, offsets and tile origin of the others only here: not kept in registers)
                    const v4i_t rw = plan4(64 * i), of = plan4(64 * i + 16);
                    smaxs[i] = plan4(64 * i + 48).x;
                    g[i].row[0] = rw.x;
                    const DescPlan di{ { 0, rw.y, rw.z, rw.w }, { of.x, of.y, of.z, of.w }, pitch, hoff };
                    KIWI_MULTI_BUILD(di, i, i, npos, noshadow);
                }
            }
            asm volatile("" :: "s"(pwarm_));             // (the warming loads' target register stays allocated until here)
            pcur += (size_t)(unsigned)pstep;
        } else {
        if (shared) KIWI_MULTI_BUILD((DescLanes{ ta, tb }), 0, -1, npos, shadow);
        else {
            KIWI_MULTI_BUILD((DescLanes{ ta, tb }), 0, 0, npos, shadow);
#pragma unroll
            for (int i = 1; i < NS; i++) {               // (descriptors of the others only here: not kept in registers)
                int tai, tbi;
                if constexpr (compact) desc_expand(off4_load(tab_of(i), c, lane), cur[i], lane, pitch, tai, tbi);
                else { tai = tab_of(i)[(size_t)c * 128 + lane]; tbi = tab_of(i)[(size_t)c * 128 + 64 + lane]; }
                g[i].row[0] = REC_I(cur[i], 0);
                KIWI_MULTI_BUILD((DescLanes{ tai, tbi }), i, i, npos, noshadow);
            }
        }
        // head records and descriptors of the NEXT group: in flight while this group is applied
#pragma unroll
        for (int i = 0; i < NS; i++) cur[i] = rec_load(recs_of(i), cend, nc, lane);
        if (cend < nc) {
            if constexpr (compact) ta = off4_load(tab_of(0), cend, lane);
            else { ta = tab_of(0)[(size_t)cend * 128 + lane]; tb = tab_of(0)[(size_t)cend * 128 + 64 + lane]; }
        }
        }
#undef KIWI_MULTI_BUILD
        __syncthreads();
        __builtin_amdgcn_s_setprio(0);
        // ---- apply: this wave's source from its tile set.  (No tail rule and no partly added centroid here: multi_taken()
        // admits only pairs whose rows all end in zero and whose centroids all find all their traces.)
        {
            const unsigned abase = (unsigned)(size_t)(lds_cfp)&tiles[sh * SET + u0];
            if constexpr (NG == 10 || NG == 8) {
                if constexpr (!PLAN || KIWI_MULTI_COEF_WARM) asm volatile("" :: "s"(warm_));          // (the warming loads' target register stays allocated until here)
                // (with plans the rotation, the header word and the coefficient pointer ARE scalars -- scalar loads and scalar
                // arithmetic at the loop's top level; a read of the first lane would take them through a vector register)
                float gcl_u = gcl, gsl_u = gsl;
                if constexpr (!PLAN) { gcl_u = __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(gcl))); gsl_u = __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(gsl))); }
                const float *__restrict__ coef_u = coef_grp;
                if constexpr (!PLAN) {
                    const size_t cg_ = (size_t)coef_grp;
                    coef_u = (const float *)(((size_t)(unsigned)__builtin_amdgcn_readfirstlane((int)(cg_ >> 32)) << 32) | (unsigned)__builtin_amdgcn_readfirstlane((int)cg_));
                }
                // the whole group in ONE hand-allocated assembly routine (kiwi_apply_asm.inc): two register sets that swap roles, the LDS reads and
                // the coefficient line of step k + 1 under the arithmetic of step k
                // (eight-component databases -- far-field Green's functions, gfdb.f90:57 -- have routines of their own since round 6: the
                // compiler's allocation of the C++ form below spilled 1-4 registers there and ran 14 % under the ten-component rate)
                const int n = cend - c;
#define KIWI_ASM_ARGS ar1[0], ar1[1], ar2[0], ar2[1], dz[0], dz[1], abase, ishv, smax, n, coef_u, gcl_u, gsl_u
#define KIWI_PLAN_ARGS ar1[0], ar1[1], ar2[0], ar2[1], dz[0], dz[1], abase, ishv, smax, n, coef_u, gcl_u, gsl_u, head_u
                if constexpr (PLAN) {
                    // regular group, group with named repeats or neither (the plan's header word, PlanSrc::head): the three texts in one
                    // statement, the choice scalar bit tests inside it (apply_steps_asm_*, tools/gen_apply_asm.py routine_steps) -- a
                    // regular group takes the routine with neither the shifts nor a test per step (apply_regular_asm_*'s text), one with
                    // repeats that text with a bit test per step and no tile read for a step that stays
                    const int head_u = flags;
                    // (rot or plain chosen by the lanes: on a scalar branch the compiler joins the two statements' accumulators
                    // through six 64-bit copies in front of each -- DESIGN 3.3, Regular groups)
                    int rot_v = flags & 2;
                    asm("" : "+v"(rot_v));
                    if constexpr (NG == 10) {
                        if (rot_v) { if constexpr (K == 5) KIWI_APPLY_PLAN(10, 5, rot)(KIWI_PLAN_ARGS); else KIWI_APPLY_PLAN(10, 9, rot)(KIWI_PLAN_ARGS); }
                        else           { if constexpr (K == 5) KIWI_APPLY_PLAN(10, 5, plain)(KIWI_PLAN_ARGS); else KIWI_APPLY_PLAN(10, 9, plain)(KIWI_PLAN_ARGS); }
                    } else {
                        if (rot_v) { if constexpr (K == 5) KIWI_APPLY_PLAN(8, 5, rot)(KIWI_PLAN_ARGS); else KIWI_APPLY_PLAN(8, 9, rot)(KIWI_PLAN_ARGS); }
                        else           { if constexpr (K == 5) KIWI_APPLY_PLAN(8, 5, plain)(KIWI_PLAN_ARGS); else KIWI_APPLY_PLAN(8, 9, plain)(KIWI_PLAN_ARGS); }
                    }
                } else
                if constexpr (NG == 10) {
                    if (flags & 2) { if constexpr (K == 5) KIWI_APPLY_ASM(10, 5, rot)(KIWI_ASM_ARGS); else KIWI_APPLY_ASM(10, 9, rot)(KIWI_ASM_ARGS); }
                    else           { if constexpr (K == 5) KIWI_APPLY_ASM(10, 5, plain)(KIWI_ASM_ARGS); else KIWI_APPLY_ASM(10, 9, plain)(KIWI_ASM_ARGS); }
                } else {
                    if (flags & 2) { if constexpr (K == 5) KIWI_APPLY_ASM(8, 5, rot)(KIWI_ASM_ARGS); else KIWI_APPLY_ASM(8, 9, rot)(KIWI_ASM_ARGS); }
                    else           { if constexpr (K == 5) KIWI_APPLY_ASM(8, 5, plain)(KIWI_ASM_ARGS); else KIWI_APPLY_ASM(8, 9, plain)(KIWI_ASM_ARGS); }
                }
#undef KIWI_ASM_ARGS
#undef KIWI_PLAN_ARGS
            } else {
            int cc = c, eprev = 0;
            bool have = false;
#define KIWI_C2STEP(LL, HH, RV, CC) do { \
                const int e = smax - __builtin_amdgcn_readlane(ishv, (CC) - c);       /* LDS position of b[j-1] of the tile's first sample */ \
                const int d = have ? eprev - e : 0x7fff; \
                carry2_apply<NG, RV, K>(ar1, ar2, dz, LL, HH, abase + 4u * (unsigned)e, d, d, coef_grp + (size_t)((CC) - c) * kCoefLine, gcl, gsl); \
                have = true; eprev = e; } while (0)
            if (flags & 2) {
                set2_dead(X); set2_dead(Y);
                for (; cc + 1 < cend; cc += 2) { KIWI_C2STEP(X, Y, true, cc); KIWI_C2STEP(Y, X, true, cc + 1); }
                if (cc < cend) KIWI_C2STEP(X, Y, true, cc);
            } else {
                set2_dead(X); set2_dead(Y);
                for (; cc + 1 < cend; cc += 2) { KIWI_C2STEP(X, Y, false, cc); KIWI_C2STEP(Y, X, false, cc + 1); }
                if (cc < cend) KIWI_C2STEP(X, Y, false, cc);
            }
#undef KIWI_C2STEP
            }
        }
        if constexpr (PLAN) coef_cur += (size_t)(unsigned)(glen * kCoefLine);
        c = cend;                                        // (the barrier in front of the next group's LDS writes: multi_build)
    }
    // ---- rotation to N/E, signs and store (or fused comparison) of this wave's source (seismogram.f90:256-283)
    {
        const int js = s0 + sh;
        const int tl = tile * TILE + u0;                 // window sample of the lane's output q = 0; q-th: + 64 q
        if (!FUSE && tl >= rv.wlen) return;
        float *__restrict__ so = syn + (size_t)js * syn_stride + tl;
        float mom = 0.f;
        if constexpr (FUSE) mom = fp.moment[fp.isrc0 + js];
        const bool whole = tile * TILE + TILE <= rv.wlen;
        for (int k = 0; k < rv.ncomp; k++) {
            f2v o01, o23;
            out4(rv.comp[k], rv.sign[k], rv.cl0, rv.sl0, ar1, ar2, dz, o01, o23);
            if constexpr (!FUSE) {
                const float o[4] = { o01.x, o01.y, o23.x, o23.y };
#pragma unroll
                for (int i = 0; i < 4; i++)
                    if (tl + 64 * i < rv.wlen) so[rv.synofs[k] + 64 * i] = o[i];
                continue;
            }
            double acc = fused_acc4(fp, o01, o23, mom, fp.reft + rv.refofs[k] + tl, fp.tw + rv.refofs[k] + tl, tl, rv.wlen, whole);
            acc = wave_reduce_f64(acc, fp.method == 6);                 // total in lane 63
            if (lane == 63)
                fp.partial[((size_t)js * fp.nmis + rv.slot0 + k) * fp.nparts + tile * WPS + (wv % WPS)] = acc;
        }
    }
}

// ------------------------------------------------------------------------------------------------
// accumulate, cell groups: the raw node traces stay in registers across the centroids of one GF cell
//
// Sources whose sub-faults are all different points (eikonal ruptures: one centroid per cell of the rupture grid) give
// accumulate_grouped_kernel groups of ONE centroid: every centroid re-fetches its 4 x NG node rows although its
// neighbours in the table sit in the same 4-node cell of the Green's function grid and need the very same rows -- only
// the four blend weights change.  Here a group is a run of consecutive centroids in the same cell (cellgroup_kernel):
// the workgroup loads the raw rows of the tile ONCE per group into registers (4 x NG dwordx4 per lane) and, per centroid,
// blends them with that centroid's weights (gfdb.f90:944-949, same order) into the LDS tile the apply phase reads, exactly
// as the grouped kernel does after its loads.  Per output sample the operations and their order are those of
// accumulate_kernel, so the results are bit-identical.  The halo (positions beyond the tile that the shifts reach) is held
// the same way: one 4-sample chunk of one component per halo lane, 16 more registers.
template <int SPL> struct RawVec;
template <> struct RawVec<4> { typedef f4u type; };
template <> struct RawVec<2> { typedef f2u type; };

// raw rows of one cell over the tile's main chunk (SPL samples per lane at LDS position p): always the clamped form of the
// address (no separate clamp-free variant: the loads run once per GROUP) and always all four nodes: a centroid exactly on
// a node carries the weights (1, 0, 0, 0) and four times the same row, and 1 v + 0 v + 0 v + 0 v is v bit for bit (also
// for -0), so no separate unblended form is needed (gfdb.f90:890-893 vs :944-949)
// The components one workgroup of accumulate_cell_kernel works on, in APPLICATION order (seismogram.f90:171-250):
// PART 0 = all of them; PART 1 = the horizontal block 1 2 3 [9] 4 5 (radial and transverse sums, rotated into the north /
// east or away / right traces), PART 2 = the vertical block 6 7 8 [10].  Two workgroups per (source, tile, receiver) halve
// the raw rows a lane keeps in registers (more waves per SIMD) at the price of doing the per-centroid bookkeeping twice.
template <int NG, int PART> struct CellPart;
template <> struct CellPart<10, 0> { static constexpr int n = 10; static constexpr int first = 0; __device__ static constexpr int ig(int i) { return i < 3 ? i : (i == 3 ? 8 : (i < 9 ? i - 1 : 9)); } };
template <> struct CellPart<8, 0>  { static constexpr int n = 8; static constexpr int first = 0; __device__ static constexpr int ig(int i) { return i; } };
template <> struct CellPart<10, 1> { static constexpr int n = 6; static constexpr int first = 0; __device__ static constexpr int ig(int i) { return i < 3 ? i : (i == 3 ? 8 : i - 1); } };
template <> struct CellPart<10, 2> { static constexpr int n = 4; static constexpr int first = 6; __device__ static constexpr int ig(int i) { return i < 3 ? 5 + i : 9; } };
template <> struct CellPart<8, 1>  { static constexpr int n = 5; static constexpr int first = 0; __device__ static constexpr int ig(int i) { return i; } };
template <> struct CellPart<8, 2>  { static constexpr int n = 3; static constexpr int first = 5; __device__ static constexpr int ig(int i) { return 5 + i; } };

template <int NG, int PART, int SPL> using RawArr = typename RawVec<SPL>::type[CellPart<NG, PART>::n][4];

// FAST: the whole tile lies inside every row of the cell (tab[52], tab[53]; the caller's test): no clamp -- the lane's
// position is the same vector offset for all loads and the row's sample-0 position goes into the load's scalar offset: one
// scalar instruction per load and no vector one
// UNI (with FAST; tab[54]): the rows of a node are `pitch` apart AND start at the same sample: the four descriptors of component 0
// give all forty positions
template <int NG, int PART, int SPL, bool FAST = false, bool UNI = false>
__device__ __forceinline__ void raw_issue(RawArr<NG, PART, SPL> &v, int p, int jb,
                                          const float *__restrict__ G, int pitch, int ta, int tb)
{
    typedef typename RawVec<SPL>::type RV;
    typedef CellPart<NG, PART> P;
    __builtin_assume(pitch >= 8);
    const int p4 = 4 * p, hi4 = 4 * (pitch - 4);
    if constexpr (FAST) {
        const unsigned jb4 = 4u * (unsigned)jb;
        unsigned node0[4] = { 0u, 0u, 0u, 0u };
        if constexpr (UNI) {
#pragma unroll
            for (int k = 0; k < 4; k++) node0[k] = 4u * (unsigned)REC_I(ta, k) + jb4;
        }
#pragma unroll
        for (int i = 0; i < P::n; i++) {
#pragma unroll
            for (int k = 0; k < 4; k++) {
                // byte position of tile sample 0 in the cell
                const unsigned so = UNI ? node0[k] + (unsigned)P::ig(i) * (4u * (unsigned)pitch)
                                        : 4u * (unsigned)REC_I(ta, 4 * P::ig(i) + k) + jb4;
                if constexpr (SPL == 4) {
                    const v4i_t w = __builtin_amdgcn_raw_buffer_load_b128(gf_rsrc(G), p4, (int)so, 0);
                    v[i][k] = RV{ __int_as_float(w.x), __int_as_float(w.y), __int_as_float(w.z), __int_as_float(w.w) };
                } else {
                    const v2i_t w = __builtin_amdgcn_raw_buffer_load_b64(gf_rsrc(G), p4, (int)so, 0);
                    v[i][k] = RV{ __int_as_float(w.x), __int_as_float(w.y) };
                }
            }
        }
        return;
    }
#pragma unroll
    for (int i = 0; i < P::n; i++) {
#pragma unroll
        for (int k = 0; k < 4; k++) {
            // row start (wave-uniform: scalar base address) + this lane's clamped position inside the row (32-bit offset):
            // one address register per load instead of a 64-bit pair, and nothing here overflows for tensors beyond 2^31 bytes
            const int base = REC_I(ta, 4 * P::ig(i) + k), lo = REC_I(tb, 4 * P::ig(i) + k);
            // lane position inside the row, clamped (one v_add + one v_med3 per load); the row start is the load's scalar offset
            // byte offset of LDS position 0 inside the row: scalar arithmetic (kept there by hand -- left to itself the
            // compiler re-associates it into the lanes), then one add and one v_med3 per load for the lane's clamped position
            int u4, q4;
            asm("s_sub_i32 %0, %1, %2\n\ts_add_i32 %0, %0, %3\n\ts_lshl_b32 %0, %0, 2" : "=&s"(u4) : "s"(base), "s"(lo), "s"(jb) : "scc");
            asm("v_add_u32 %0, %1, %2\n\tv_med3_i32 %0, %0, 0, %3" : "=&v"(q4) : "s"(u4), "v"(p4), "s"(hi4));
            if constexpr (SPL == 4) {
                const v4i_t w = __builtin_amdgcn_raw_buffer_load_b128(gf_rsrc(G), q4, (int)(4u * (unsigned)lo), 0);
                v[i][k] = RV{ __int_as_float(w.x), __int_as_float(w.y), __int_as_float(w.z), __int_as_float(w.w) };
            } else {
                const v2i_t w = __builtin_amdgcn_raw_buffer_load_b64(gf_rsrc(G), q4, (int)(4u * (unsigned)lo), 0);
                v[i][k] = RV{ __int_as_float(w.x), __int_as_float(w.y) };
            }
        }
    }
}

template <int NG, int PART, int SPL>
__device__ __forceinline__ void raw_blend_store(const RawArr<NG, PART, SPL> &v, float *__restrict__ tile0,
                                                int lds_tile, int p, float w0, float w1, float w2, float w3)
{
    typedef typename RawVec<SPL>::type RV;
#pragma unroll
    for (int i = 0; i < CellPart<NG, PART>::n; i++) {
        RV b = w0 * v[i][0];                      // gfdb.f90:946-949, summed in this order
        b = kiwi_mad(b, w1, v[i][1]);
        b = kiwi_mad(b, w2, v[i][2]);
        b = kiwi_mad(b, w3, v[i][3]);
        if constexpr (SPL == 4) *(float4 *)(tile0 + i * lds_tile + p) = make_float4(b.x, b.y, b.z, b.w);
        else                    *(float2 *)(tile0 + i * lds_tile + p) = make_float2(b.x, b.y);
    }
}

// One centroid's components of PART from the LDS tiles (tile i = i-th component of the part in application order); the same
// operations in the same order as centroid_apply_hd performs for these components.
template <int NG, int PART, int LDS_TILE, bool TAIL, int NP>
__device__ __forceinline__ void cell_apply(f2v (&ar1)[NP], f2v (&ar2)[NP], f2v (&dz)[NP], const TileBase &chunk0, int jl,
                                           const int (&jend)[CellPart<NG, PART>::n], int flags,
                                           const float (&cw)[2 * CellPart<NG, PART>::n] /* (wl, wr) per component in application order */,
                                           int rec, float sd, float cl, float sl)
{
    typedef CellPart<NG, PART> P;
    constexpr int nH1 = (NG == 10) ? 4 : 3;      // components summed into the radial trace
    constexpr int nH = (NG == 10) ? 6 : 5;       // horizontal block
    constexpr int g0 = P::first;                 // application-order index of the part's first component
    float fac[P::n];
#pragma unroll
    for (int i = 0; i < P::n; i++) fac[i] = 0.f;
    if constexpr (TAIL) {                         // the tail rule needs the plain factors (sparse_trace.f90:698-703)
        const float f0 = REC_F(rec, 10), f1 = REC_F(rec, 11), f2 = REC_F(rec, 12), f3 = REC_F(rec, 13), f4 = REC_F(rec, 14), f5 = REC_F(rec, 15);
        const float all10[10] = { f0, f1, f2, f5, f3, f4, f0 * sd, f1 * sd, f2 * sd, f5 * sd };
        const float all8[8] = { f0, f1, f2, f3, f4, f0 * sd, f1 * sd, f2 * sd };
#pragma unroll
        for (int i = 0; i < P::n; i++) fac[i] = (NG == 10) ? all10[g0 + i] : all8[g0 + i];
    }
    constexpr int kAhead = 2;
    TileRegsN<NP> tr[P::n];
#pragma unroll
    for (int i = 0; i < kAhead && i < P::n; i++) tr[i] = tile_load<NP>(chunk0, i * LDS_TILE);
    const bool rot = (flags & 2) != 0;           // seismogram.f90:160-203 vs :205-231
    f2v t1[NP], t2[NP];
    if constexpr (PART != 2) {
#pragma unroll
        for (int k = 0; k < NP; k++) { t1[k] = rot ? f2v{ 0.f, 0.f } : ar1[k]; t2[k] = rot ? f2v{ 0.f, 0.f } : ar2[k]; }
    }
#pragma unroll
    for (int i = 0; i < P::n; i++) {
        if (i + kAhead < P::n) tr[i + kAhead] = tile_load<NP>(chunk0, (i + kAhead) * LDS_TILE);
        __builtin_amdgcn_sched_barrier(0);
        const int a = g0 + i;                    // application-order index
        if (a < nH1)     tile_fma<TAIL, NP>(t1, tr[i], jl, jend[i], fac[i], cw[coef_wl<NG>(g0 + i)], cw[coef_wr<NG>(g0 + i)]);
        else if (a < nH) tile_fma<TAIL, NP>(t2, tr[i], jl, jend[i], fac[i], cw[coef_wl<NG>(g0 + i)], cw[coef_wr<NG>(g0 + i)]);
        else             tile_fma<TAIL, NP>(dz, tr[i], jl, jend[i], fac[i], cw[coef_wl<NG>(g0 + i)], cw[coef_wr<NG>(g0 + i)]);
        if (a == nH - 1) {
            if (rot) {
#pragma unroll
                for (int k = 0; k < NP; k++) {
                    ar1[k] = ar1[k] + cl * t1[k] - sl * t2[k];
                    ar2[k] = ar2[k] + cl * t2[k] + sl * t1[k];
                }
            } else {
#pragma unroll
                for (int k = 0; k < NP; k++) { ar1[k] = t1[k]; ar2[k] = t2[k]; }
            }
        }
    }
}

// waves per SIMD the register allocation aims at: the whole component set (PART 0) keeps 80 + 16 raw registers per lane and
// runs best at two, a half set (PART 1 / 2) at three
// SPL: output samples per lane (tile = SPL * T samples).  With four the raw rows of a group take 160 registers per lane and
// leave room for one wave per SIMD only; with two they take 80 and the kernel keeps the grouped kernel's three waves.
//
// Takes the (source, receiver) pairs of cell_pair(): receivers with horizontal and vertical components, no centroid with a
// missing trace; accumulate_grouped_kernel is launched behind it for the other pairs.
//
// Schedule.  Two LDS tile sets: while centroid k is applied from one, centroid k + 1 of the group is blended into the
// other (ONE barrier per centroid, and the blend's arithmetic fills the issue slots the apply's LDS reads leave).  During
// the last apply of a group the raw registers are free again, so the loads of the NEXT group's rows are issued there and
// their L2 round trip is hidden behind that apply.
template <int NG, int T, int SPL, int PART, bool FUSE, bool COMPACT>
__global__ __launch_bounds__(T) __attribute__((amdgpu_waves_per_eu(PART == 0 ? 2 : 3))) void accumulate_cell_kernel(
    const float *__restrict__ G, const int2 *__restrict__ span, int pitch,
    const GeoRec *__restrict__ recs, const int *__restrict__ cent_ofs, int isrc0, int nrec,
    const RecvDev *__restrict__ recv, float *__restrict__ syn, size_t syn_stride, int ntiles,
    const int *__restrict__ tab, const float *__restrict__ coefs, FuseParams fp, const int *__restrict__ pairflag, const int *__restrict__ synrow,
    const int *__restrict__ fam_ofs, const int *__restrict__ fam_list)
{
    constexpr bool compact = COMPACT;
    constexpr int NP = SPL / 2;
    constexpr int TILE = SPL * T;
    constexpr int LDS_TILE = TILE + kHalo;
    static_assert(LDS_TILE % 64 == 0, "ds_read2st64 offsets");
    typedef CellPart<NG, PART> P;
    static_assert(16 * P::n <= T, "one halo chunk per lane");
    __shared__ __attribute__((aligned(16))) float tiles[2][P::n][LDS_TILE];
    const int s = (int)blockIdx.x;                        // source index fastest (see accumulate_grouped_kernel)
    const int tile = blockIdx.y % ntiles, r = blockIdx.y / ntiles;
    const RecvDev &rv = recv[r];
    if (!rv.enabled) return;
    if (tile * TILE >= rv.wlen) return;
    if (!cell_pair(rv, pairflag, s, nrec, r)) return;
    if (synrow && synrow[s] != s) return;
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int t_tile0 = rv.wbeg + tile * TILE;
    const int cb = cent_ofs[isrc0], c0 = cent_ofs[isrc0 + s], nc = cent_ofs[isrc0 + s + 1] - c0;
    const GeoRec *__restrict__ rc = recs + ((size_t)(c0 - cb) * nrec + (size_t)r * nc);
    const int *__restrict__ tc = tab + ((size_t)(c0 - cb) * nrec + (size_t)r * nc) * (compact ? 4 : 128);
    const float sd = rv.sd;
    const int u0 = SPL * (tid & ~63) + lane;             // this lane's first tile sample (the others: + 64 q)
    // halo: lane q < 16 n owns the 4-sample chunk q / n of the part's component q % n beyond the tile.  Chunk-major: a
    // group needs the first few chunks only (its shift range plus 8 samples), so the active lanes are the first ones and
    // the waves behind them skip the halo's blend
    const int hloc = tid % P::n, hph = TILE + 4 * (tid / P::n);
    int hig = P::ig(0);
#pragma unroll
    for (int i = 1; i < P::n; i++) if (hloc == i) hig = P::ig(i);
    const bool hslot = tid < 16 * P::n;

    f2v ar1[NP], ar2[NP], dz[NP];
#pragma unroll
    for (int h = 0; h < NP; h++) { ar1[h] = f2v{ 0.f, 0.f }; ar2[h] = f2v{ 0.f, 0.f }; dz[h] = f2v{ 0.f, 0.f }; }
    typename RawVec<SPL>::type raw[P::n][4];             // raw rows of the current group over the tile's main chunk
    HaloRegs hraw;                                       // ... and over the halo chunk of this lane

    // issue the loads of the group with head fields (pad, ishift) and descriptors ta_ / tb_
#define CELL_LOAD(head_row0, head_pad, head_ishift, ta_, tb_) do { \
        const int smax_ = (head_ishift) + (((head_pad) >> 8) & 0xff), smin_ = (head_ishift) - (((head_pad) >> 16) & 0xff); \
        const int jb_ = t_tile0 - smax_ - 1, npos_ = TILE + (smax_ - smin_) + 8; \
        const float *__restrict__ Gg_ = G + (size_t)(head_row0) * (size_t)pitch;     /* descriptors are relative to it (write_tab) */ \
        /* every row of the cell holds the whole tile: rows start at or before it and end behind it */ \
        const bool inside_ = (REC_I(ta_, 52) + jb_ >= 0) && (REC_I(ta_, 53) + jb_ + SPL * (T - 1) <= pitch - 4); \
        if (inside_) raw_issue<NG, PART, SPL, true>(raw, SPL * tid, jb_, Gg_, pitch, ta_, tb_); \
        else         raw_issue<NG, PART, SPL, false>(raw, SPL * tid, jb_, Gg_, pitch, ta_, tb_); \
        hraw = halo_issue<true, false>(hslot && hph < npos_, hig, hph, jb_, Gg_, pitch, ta_, tb_); \
    } while (0)
    // blend the registers with the weights in lanes 4..7 of record `rec_` into tile set `buf_`
#define CELL_BLEND(rec_, buf_, npos_) do { \
        GeoRec gw_; \
        gw_.w[0] = REC_F(rec_, 4); gw_.w[1] = REC_F(rec_, 5); gw_.w[2] = REC_F(rec_, 6); gw_.w[3] = REC_F(rec_, 7); \
        float *tile0_ = &tiles[buf_][0][0]; \
        raw_blend_store<NG, PART, SPL>(raw, tile0_, LDS_TILE, SPL * tid, gw_.w[0], gw_.w[1], gw_.w[2], gw_.w[3]); \
        halo_finish<true>(hslot && hph < (npos_), hraw, tile0_, LDS_TILE, hloc, hph, gw_); \
    } while (0)

    // One load site inside the loop (the NEXT group's rows, issued in front of the last apply of the group, when the raw
    // registers are free: their L2 round trip hides behind that apply) and one in front of it for the first group.  The last
    // centroid of a group is peeled off the loop over its centroids so that this redefinition of the raw registers is
    // straight-line code: as a conditional inside the loop it cost ~130 register copies per group.  (Pairs with skipped
    // centroids, row < 0, are not cell pairs: accumulate_grouped_kernel has them.)
    int c = 0;
    int cur = rec_load(rc, 0, nc, lane);                 // record c, lane-distributed; nx1: record c + 1
    int nx1 = rec_load(rc, 1, nc, lane);
    int ta = 0, tb = 0;                                  // load descriptors of record c (none for a source without centroids)
    if (nc > 0) {
        if (compact) desc_expand<true>(off4_load(tc, 0, lane), cur, lane, pitch, ta, tb);
        else { ta = tc[lane]; tb = tc[64 + lane]; }
        CELL_LOAD(REC_I(cur, 0), REC_I(cur, 19), REC_I(cur, 8), ta, tb);
    }
    // apply centroid cc_ of the group from tile set bsel (as accumulate_grouped_kernel); its record is `cur`
#define CELL_APPLY(cc_) do { \
        const int flags = REC_I(cur, 18); \
        const int ishift = REC_I(cur, 8); \
        const float cl = REC_F(cur, 16), sl = REC_F(cur, 17); \
        const int e = smax - ishift; \
        const TileBase chunk0 = tile_base(&tiles[bsel][0][e + u0]); \
        const int jl = jb + e + u0; \
        const bool tail = (jb + e + TILE) > jend_min; \
        if (!tail) { const int nojend[P::n] = {}; cell_apply<NG, PART, LDS_TILE, false, NP>(ar1, ar2, dz, chunk0, jl, nojend, flags, cw, cur, sd, cl, sl); } \
        else { \
            int jend[P::n];                     /* end indices: the tail rule only (kept out of the scalar registers otherwise) */ \
            _Pragma("unroll") for (int i = 0; i < P::n; i++) jend[i] = REC_I(tg, 40 + P::ig(i)); \
            cell_apply<NG, PART, LDS_TILE, true, NP>(ar1, ar2, dz, chunk0, jl, jend, flags, cw, cur, sd, cl, sl); \
        } \
    } while (0)
    // the coefficient line of centroid cc_ (scalar loads), issued at the top of the centroid's step: in front of the blend of
    // the next centroid, whose arithmetic covers its round trip (the table comes from HBM).  Not a step earlier: scalar loads
    // share the counter of the LDS operations, and the drain in front of the barrier would wait for them
#define CELL_COEF(cc_) do { \
        const float *__restrict__ coef_ = coef_grp + (size_t)((cc_) - c) * kCoefLine; \
        _Pragma("unroll") for (int i = 0; i < 2 * P::n; i++) cw[i] = coef_[i]; \
    } while (0)
    while (c < nc) {
        const int pad0 = REC_I(cur, 19), ishift0 = REC_I(cur, 8);
        const int cend = c + (pad0 & 0xff);
        const int smax = ishift0 + ((pad0 >> 8) & 0xff), smin = ishift0 - ((pad0 >> 16) & 0xff);
        const int jb = t_tile0 - smax - 1;               // LDS position p holds blended trace sample jb + p
        const int npos = TILE + (smax - smin) + 8;
        const int tg = ta;                               // this group's descriptor row (end indices for the tail rule)
        const int jend_min = PART == 0 ? min(REC_I(ta, 50), REC_I(ta, 51)) : REC_I(ta, PART == 1 ? 50 : 51);
        // descriptors of the NEXT group
        int ta_n = 0, tb_n = 0;
        if (cend < nc) { if (compact) ta_n = off4_load(tc, cend, lane); else { ta_n = tc[(size_t)cend * 128 + lane]; tb_n = tc[(size_t)cend * 128 + 64 + lane]; } }
        const size_t crow = ((size_t)(c0 - cb) * nrec + (size_t)r * nc + c) * kCoefLine;
        const unsigned clo = __builtin_amdgcn_readfirstlane((unsigned)crow), chi = __builtin_amdgcn_readfirstlane((unsigned)(crow >> 32));
        const float *__restrict__ coef_grp = coefs + (((size_t)chi << 32) | clo);
        float cw[2 * P::n];
        // ---- first centroid of the group: its tile goes into set 0 (every set is free after the barrier that ended the last group)
        CELL_BLEND(cur, 0, npos);
        __syncthreads();
        int bsel = 0;
        for (int cc = c; cc + 1 < cend; cc++) {
            const int nx2 = rec_load(rc, cc + 2, nc, lane);      // two records ahead: the next one is needed for its weights now
            // ---- centroid cc + 1 of the group into the other tile set (a centroid at the point of its predecessor keeps the tile)
            const bool blend_next = !(REC_I(nx1, 18) & 4);
            CELL_COEF(cc);
            if (blend_next) CELL_BLEND(nx1, bsel ^ 1, npos);
            CELL_APPLY(cc);
            __syncthreads();     // set bsel may be overwritten, set bsel ^ 1 is complete
            if (blend_next) bsel ^= 1;
            cur = nx1; nx1 = nx2;
        }
        {
            // ---- last centroid of the group: the raw registers are free, the next group's rows can be on their way
            const int nx2 = rec_load(rc, cend + 1, nc, lane);
            CELL_COEF(cend - 1);
            if (compact && cend < nc) desc_expand<true>(ta_n, nx1, lane, pitch, ta_n, tb_n);       // (nx1: the next group's head record)
            if (cend < nc) CELL_LOAD(REC_I(nx1, 0), REC_I(nx1, 19), REC_I(nx1, 8), ta_n, tb_n);
            CELL_APPLY(cend - 1);
            __syncthreads();
            cur = nx1; nx1 = nx2;
        }
        ta = ta_n; tb = tb_n;
        c = cend;
    }
#undef CELL_APPLY
#undef CELL_COEF
#undef CELL_LOAD
#undef CELL_BLEND
    // ---- rotation to N/E, signs, store or fused comparator (seismogram.f90:256-283), as accumulate_grouped_kernel; with the
    // fused comparator also for the sources that share these synthetics (fam_list), each with its own moment
    const int nfam = (FUSE && fam_ofs) ? fam_ofs[s + 1] - fam_ofs[s] : 0;
    for (int qf = -1; qf < nfam; qf++) {
        const int js = qf < 0 ? s : fam_list[fam_ofs[s] + qf];
        const int tl = tile * TILE + u0;
        if (!FUSE && tl >= rv.wlen) return;
        float *__restrict__ so = syn + (size_t)js * syn_stride + tl;
        float a1[SPL], a2[SPL], ad[SPL];
#pragma unroll
        for (int h = 0; h < NP; h++) {
            a1[2 * h] = ar1[h].x; a1[2 * h + 1] = ar1[h].y; a2[2 * h] = ar2[h].x; a2[2 * h + 1] = ar2[h].y;
            ad[2 * h] = dz[h].x; ad[2 * h + 1] = dz[h].y;
        }
        float mom = 0.f;
        if constexpr (FUSE) mom = fp.moment[fp.isrc0 + js];
        const bool unit = (fp.syn_factor == 1.f);
        for (int k = 0; k < rv.ncomp; k++) {
            if (PART != 0 && (rv.comp[k] == 3) != (PART == 2)) continue;      // the vertical trace belongs to the PART 2 workgroup
            const float sg = rv.sign[k];
            float o[SPL];
#pragma unroll
            for (int i = 0; i < SPL; i++) {
                switch (rv.comp[k]) {
                case 1: o[i] = a1[i] * sg; break;
                case 2: o[i] = a2[i] * sg; break;
                case 3: o[i] = ad[i]; break;
                case 4: o[i] = (rv.cl0 * a1[i] - rv.sl0 * a2[i]) * sg; break;
                default: o[i] = (rv.cl0 * a2[i] + rv.sl0 * a1[i]) * sg; break;
                }
            }
            if constexpr (!FUSE) {
#pragma unroll
                for (int i = 0; i < SPL; i++)
                    if (tl + 64 * i < rv.wlen) so[rv.synofs[k] + 64 * i] = o[i];
                continue;
            }
            double acc = 0.0;
            const float *__restrict__ rt = fp.reft + rv.refofs[k] + tl, *__restrict__ tp = fp.tw + rv.refofs[k] + tl;
#pragma unroll
            for (int i = 0; i < SPL; i++) {
                if (tl + 64 * i >= rv.wlen) break;
                const float v = o[i] * mom;
                const float vt = v * tp[64 * i];
                const float a = rt[64 * i];
                switch (fp.method) {
                case 1: { const float d = unit ? (a - vt) : (1.f * a - fp.syn_factor * vt); acc = sq_acc(acc, d); break; }
                case 2: { const float d = unit ? fabsf(a - vt) : fabsf(1.f * a - fp.syn_factor * vt); acc += (double)d; break; }
                case 5: acc += unit ? (double)(a * vt) : (double)(a * 1.f * vt * fp.syn_factor); break;
                default: { const double x = (double)(1.f * a), y = (double)(fp.syn_factor * vt); acc = fmax(acc, sqrt(x * x + y * y)); break; }
                }
            }
            acc = wave_reduce_f64(acc, fp.method == 6);                 // total in lane 63
            if (lane == 63)
                fp.partial[((size_t)js * fp.nmis + rv.slot0 + k) * fp.nparts + tile * (T / 64) + (tid >> 6)] = acc;
        }
    }
}

// ------------------------------------------------------------------------------------------------
// accumulate, cell groups, a tile per WAVE (r03)
//
// accumulate_cell_kernel shares its tile among the four waves of the workgroup: a barrier per centroid, at which three
// waves wait for the slowest (measured: 10 % of the kernel), and every wave in the same phase at the same time.  Here a wave
// owns the 128 output samples it computes AND the blended samples they need: it blends positions 0 .. 127 of its tile from
// the raw rows in its registers plus the few positions behind them that the group's shifts reach (one 2-sample chunk of one
// component per lane, lanes 0 .. 59: groups are cut at a shift range of kCellwRange), and reads them back itself.  LDS
// operations of one wave execute in order, so there is no barrier anywhere in the loop, and ONE tile set is enough: per
// component the step reads what the apply of centroid k needs, then writes the blend of centroid k + 1 over it, then does
// the arithmetic of both.  Waves drift apart and fill each other's stalls (loads of the next group's rows, the first blend of
// a group, LDS round trips).  Per output sample the operations and their order are those of accumulate_cell_kernel.
constexpr int kCellwRow = 192;      // floats per component row of a wave's tile: 128 + halo, a multiple of 64 (ds_read2st64 offsets)
constexpr int kCellwChunk = 2;      // samples of a lane's halo chunk
constexpr int kCellwRange = 11;     // largest shift range of a group: 12 positions behind the 128 = six 2-sample chunks x 10 components = 60 lanes
                                    // (23 with 4-sample chunks until round 5; of 3118 cfg4 runs none has a range above 10, 83 % have <= 3)

// One step of a wave: apply centroid k (record `rec`, coefficients cw, tile position `pos` = e + lane) and, BLEND, put centroid
// k + 1 (weights w0 .. w3) into the tile -- component by component, the write of a component's row behind the read of it.
template <int NG, bool TAIL, bool BLEND>
__device__ __forceinline__ void cellw_step(f2v (&ar1)[1], f2v (&ar2)[1], f2v (&dz)[1], float *__restrict__ wt, int pos,
                                           const RawArr<NG, 0, 2> &raw, float w0, float w1, float w2, float w3, int pl,
                                           bool hact, const HaloRegs2 &hraw, int hloc, int hph,
                                           int jl, const int (&jend)[CellPart<NG, 0>::n], int flags,
                                           const float (&cw)[2 * CellPart<NG, 0>::n], int rec, float sd, float cl, float sl)
{
    typedef CellPart<NG, 0> P;
    constexpr int nH1 = (NG == 10) ? 4 : 3;      // components summed into the radial trace
    constexpr int nH = (NG == 10) ? 6 : 5;       // horizontal block
    float fac[P::n];
#pragma unroll
    for (int i = 0; i < P::n; i++) fac[i] = 0.f;
    if constexpr (TAIL) {                         // the tail rule needs the plain factors (sparse_trace.f90:698-703)
        const float f0 = REC_F(rec, 10), f1 = REC_F(rec, 11), f2 = REC_F(rec, 12), f3 = REC_F(rec, 13), f4 = REC_F(rec, 14), f5 = REC_F(rec, 15);
        const float all10[10] = { f0, f1, f2, f5, f3, f4, f0 * sd, f1 * sd, f2 * sd, f5 * sd };
        const float all8[8] = { f0, f1, f2, f3, f4, f0 * sd, f1 * sd, f2 * sd };
#pragma unroll
        for (int i = 0; i < P::n; i++) fac[i] = (NG == 10) ? all10[i] : all8[i];
    }
    const TileBase chunk0 = tile_base(wt + pos);
#if defined(KIWI_EXPLICIT_FMA)
    constexpr int kAhead = KIWI_CELLW_AHEAD;      // (fused: 6 packed instructions per component -- more reads in flight to cover the LDS round trip)
#else
    constexpr int kAhead = 2;
#endif
    TileRegsN<1> tr[P::n];
#pragma unroll
    for (int i = 0; i < kAhead && i < P::n; i++) tr[i] = tile_load<1>(chunk0, i * kCellwRow);
    const bool rot = (flags & 2) != 0;           // seismogram.f90:160-203 vs :205-231
    f2v t1[1], t2[1];
    t1[0] = rot ? f2v{ 0.f, 0.f } : ar1[0]; t2[0] = rot ? f2v{ 0.f, 0.f } : ar2[0];
#pragma unroll
    for (int i = 0; i < P::n; i++) {
        if (i + kAhead < P::n) tr[i + kAhead] = tile_load<1>(chunk0, (i + kAhead) * kCellwRow);
        __builtin_amdgcn_sched_barrier(0);
        if constexpr (BLEND) {                    // row i has been read (kAhead iterations ago): its next content may go in
            f2u b = w0 * raw[i][0];               // gfdb.f90:946-949, summed in this order
            b = kiwi_mad(b, w1, raw[i][1]);
            b = kiwi_mad(b, w2, raw[i][2]);
            b = kiwi_mad(b, w3, raw[i][3]);
            *(float2 *)(wt + i * kCellwRow + pl) = make_float2(b.x, b.y);
        }
        if (i < nH1)     tile_fma<TAIL, 1>(t1, tr[i], jl, jend[i], fac[i], cw[coef_wl<NG>(i)], cw[coef_wr<NG>(i)]);
        else if (i < nH) tile_fma<TAIL, 1>(t2, tr[i], jl, jend[i], fac[i], cw[coef_wl<NG>(i)], cw[coef_wr<NG>(i)]);
        else             tile_fma<TAIL, 1>(dz, tr[i], jl, jend[i], fac[i], cw[coef_wl<NG>(i)], cw[coef_wr<NG>(i)]);
        if (i == nH - 1) {
            if (rot) {
                ar1[0] = kiwi_mad(kiwi_mad(ar1[0], cl, t1[0]), -sl, t2[0]);
                ar2[0] = kiwi_mad(kiwi_mad(ar2[0], cl, t2[0]), sl, t1[0]);
            } else {
                ar1[0] = t1[0]; ar2[0] = t2[0];
            }
        }
#if defined(KIWI_EXPLICIT_FMA)
        // (with four instructions of blend per component the instruction selector otherwise emits all ten applies below the last
        // blend -- forty registers of tile samples alive at once, 28 bytes of scratch per lane.  Arithmetic has no place in the
        // order of side effects, an empty volatile statement that takes the accumulator has: the apply of a component stays in its
        // iteration)
        if (i < nH1)     asm volatile("" : "+v"(t1[0]));
        else if (i < nH) asm volatile("" : "+v"(t2[0]));
        else             asm volatile("" : "+v"(dz[0]));
        __builtin_amdgcn_sched_barrier(0);
#endif
    }
    if constexpr (BLEND) halo_finish2(hact, hraw, wt, kCellwRow, hloc, hph, w0, w1, w2, w3);      // behind every read of this step
}

template <int NG, bool FUSE, bool COMPACT>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(3))) void accumulate_cellw_kernel(
    const float *__restrict__ G, const int2 *__restrict__ span, int pitch,
    const GeoRec *__restrict__ recs, const int *__restrict__ cent_ofs, int isrc0, int nrec,
    const RecvDev *__restrict__ recv, float *__restrict__ syn, size_t syn_stride, int ntiles,
    const int *__restrict__ tab, const float *__restrict__ coefs, FuseParams fp, const int *__restrict__ pairflag, const int *__restrict__ synrow,
    const int *__restrict__ fam_ofs, const int *__restrict__ fam_list)
{
    constexpr bool compact = COMPACT;
    constexpr int T = 256, SPL = 2, TILE = SPL * T;
    typedef CellPart<NG, 0> P;
    __shared__ __attribute__((aligned(16))) float tiles[T / 64][P::n][kCellwRow];
    const int s = (int)blockIdx.x;                        // source index fastest (see accumulate_grouped_kernel)
    const int tile = blockIdx.y % ntiles, r = blockIdx.y / ntiles;
    const RecvDev &rv = recv[r];
    if (!rv.enabled) return;
    if (tile * TILE >= rv.wlen) return;
    if (!cell_pair(rv, pairflag, s, nrec, r)) return;
    if (synrow && synrow[s] != s) return;
    const int tid = threadIdx.x;
    // (the wave's index is uniform: told so, everything derived from it -- its tile, its first sample, the tail test of a step --
    // stays in scalar registers and the tail branch is a scalar branch; until round 6 it was a divergent one, with both step variants
    // behind exec masks and the accumulators copied through at the loop's end)
    const int lane = tid & 63, wv = __builtin_amdgcn_readfirstlane(tid >> 6);
    float *__restrict__ wt = &tiles[wv][0][0];            // this wave's tile
    const int t_tile0 = rv.wbeg + tile * TILE;
    const int cb = cent_ofs[isrc0], c0 = cent_ofs[isrc0 + s], nc = cent_ofs[isrc0 + s + 1] - c0;
    const GeoRec *__restrict__ rc = recs + ((size_t)(c0 - cb) * nrec + (size_t)r * nc);
    const int *__restrict__ tc = tab + ((size_t)(c0 - cb) * nrec + (size_t)r * nc) * (compact ? 4 : 128);
    const float sd = rv.sd;
    const int w0s = 128 * wv;                             // first sample of the wave inside the workgroup's 512
    const int u0 = w0s + lane;                            // this lane's first output sample (the other: + 64)
    const int pl = 2 * lane;                              // the two tile positions this lane blends
    // halo: lane q owns the 2-sample chunk q / n of component q % n behind the wave's 128 positions
    const int hloc = lane % P::n, hch = lane / P::n, hph = 128 + kCellwChunk * hch;
    int hig = P::ig(0);
#pragma unroll
    for (int i = 1; i < P::n; i++) if (hloc == i) hig = P::ig(i);

    f2v ar1[1], ar2[1], dz[1];
    ar1[0] = f2v{ 0.f, 0.f }; ar2[0] = f2v{ 0.f, 0.f }; dz[0] = f2v{ 0.f, 0.f };
    f2u raw[P::n][4];                                     // raw rows of the current group over the wave's 128 positions
    HaloRegs2 hraw;                                       // ... and over the halo chunk of this lane

    // issue the loads of the group with head fields (pad, ishift) and descriptors ta_ / tb_
#define CELLW_LOAD(head_row0, head_pad, head_ishift, ta_, tb_) do { \
        const int smax_ = (head_ishift) + (((head_pad) >> 8) & 0xff), smin_ = (head_ishift) - (((head_pad) >> 16) & 0xff); \
        const int jb_ = t_tile0 - smax_ - 1; \
        const float *__restrict__ Gg_ = G + (size_t)(head_row0) * (size_t)pitch;     /* descriptors are relative to it (write_tab) */ \
        /* every row of the cell holds the whole tile: rows start at or before it and end behind it */ \
        const bool inside_ = (REC_I(ta_, 52) + jb_ >= 0) && (REC_I(ta_, 53) + jb_ + SPL * (T - 1) <= pitch - 4); \
        if (inside_ && REC_I(ta_, 54)) raw_issue<NG, 0, SPL, true, true>(raw, SPL * tid, jb_, Gg_, pitch, ta_, tb_); \
        else if (inside_) raw_issue<NG, 0, SPL, true>(raw, SPL * tid, jb_, Gg_, pitch, ta_, tb_); \
        else         raw_issue<NG, 0, SPL, false>(raw, SPL * tid, jb_, Gg_, pitch, ta_, tb_); \
        hraw = halo_issue2<false>(kCellwChunk * hch <= smax_ - smin_, hig, w0s + hph, jb_, Gg_, pitch, ta_, tb_); \
    } while (0)
#define CELLW_COEF(cc_) do { \
        const float *__restrict__ coef_ = coef_grp + (size_t)((cc_) - c) * kCoefLine; \
        _Pragma("unroll") for (int i = 0; i < 2 * P::n; i++) cw[i] = coef_[i]; \
    } while (0)
    // one step: apply centroid `cur` from the tile and (blend_) put centroid nx1 into it
#define CELLW_STEP(blend_) do { \
        const int flags = REC_I(cur, 18); \
        const int ishift = REC_I(cur, 8); \
        const float cl = REC_F(cur, 16), sl = REC_F(cur, 17); \
        const int e = smax - ishift; \
        const int jl = jb + e + u0; \
        const bool tail = (jb + e + w0s + 128) > jend_min; \
        const float bw0 = REC_F(nx1, 4), bw1 = REC_F(nx1, 5), bw2 = REC_F(nx1, 6), bw3 = REC_F(nx1, 7); \
        if (!tail) { \
            const int nojend[P::n] = {}; \
            if (blend_) cellw_step<NG, false, true>(ar1, ar2, dz, wt, e + lane, raw, bw0, bw1, bw2, bw3, pl, hact, hraw, hloc, hph, jl, nojend, flags, cw, cur, sd, cl, sl); \
            else        cellw_step<NG, false, false>(ar1, ar2, dz, wt, e + lane, raw, bw0, bw1, bw2, bw3, pl, hact, hraw, hloc, hph, jl, nojend, flags, cw, cur, sd, cl, sl); \
        } else { \
            int jend[P::n];                     /* end indices: the tail rule only (kept out of the scalar registers otherwise) */ \
            _Pragma("unroll") for (int i = 0; i < P::n; i++) jend[i] = REC_I(tg, 40 + P::ig(i)); \
            if (blend_) cellw_step<NG, true, true>(ar1, ar2, dz, wt, e + lane, raw, bw0, bw1, bw2, bw3, pl, hact, hraw, hloc, hph, jl, jend, flags, cw, cur, sd, cl, sl); \
            else        cellw_step<NG, true, false>(ar1, ar2, dz, wt, e + lane, raw, bw0, bw1, bw2, bw3, pl, hact, hraw, hloc, hph, jl, jend, flags, cw, cur, sd, cl, sl); \
        } \
    } while (0)

    int c = 0;
    int cur = rec_load(rc, 0, nc, lane);                 // record c, lane-distributed; nx1: record c + 1
    int nx1 = rec_load(rc, 1, nc, lane);
    int ta = 0, tb = 0;                                  // load descriptors of record c (none for a source without centroids)
    if (nc > 0) {
        if (compact) desc_expand<true>(off4_load(tc, 0, lane), cur, lane, pitch, ta, tb);
        else { ta = tc[lane]; tb = tc[64 + lane]; }
        CELLW_LOAD(REC_I(cur, 0), REC_I(cur, 19), REC_I(cur, 8), ta, tb);
    }
    while (c < nc) {
        const int pad0 = REC_I(cur, 19), ishift0 = REC_I(cur, 8);
        const int cend = c + (pad0 & 0xff);
        const int smax = ishift0 + ((pad0 >> 8) & 0xff), smin = ishift0 - ((pad0 >> 16) & 0xff);
        const int jb = t_tile0 - smax - 1;               // tile position q of this wave holds blended trace sample jb + 128 wv + q
        const bool hact = kCellwChunk * hch <= smax - smin;        // positions 128 .. 128 + (smax - smin) are read
        const int tg = ta;                               // this group's descriptor row (end indices for the tail rule)
        const int jend_min = min(REC_I(ta, 50), REC_I(ta, 51));
        // descriptors of the NEXT group
        int ta_n = 0, tb_n = 0;
        if (cend < nc) { if (compact) ta_n = off4_load(tc, cend, lane); else { ta_n = tc[(size_t)cend * 128 + lane]; tb_n = tc[(size_t)cend * 128 + 64 + lane]; } }
        const size_t crow = ((size_t)(c0 - cb) * nrec + (size_t)r * nc + c) * kCoefLine;
        const unsigned clo = __builtin_amdgcn_readfirstlane((unsigned)crow), chi = __builtin_amdgcn_readfirstlane((unsigned)(crow >> 32));
        const float *__restrict__ coef_grp = coefs + (((size_t)chi << 32) | clo);
        float cw[2 * P::n];
        {   // ---- first centroid of the group into the tile (behind the reads of the last step: LDS operations of a wave run in order)
            GeoRec gw;
            gw.w[0] = REC_F(cur, 4); gw.w[1] = REC_F(cur, 5); gw.w[2] = REC_F(cur, 6); gw.w[3] = REC_F(cur, 7);
            raw_blend_store<NG, 0, SPL>(raw, wt, kCellwRow, pl, gw.w[0], gw.w[1], gw.w[2], gw.w[3]);
            halo_finish2(hact, hraw, wt, kCellwRow, hloc, hph, gw.w[0], gw.w[1], gw.w[2], gw.w[3]);
        }
        __builtin_amdgcn_s_setprio(0);
        for (int cc = c; cc + 1 < cend; cc++) {
            const int nx2 = rec_load(rc, cc + 2, nc, lane);      // two records ahead: the next one is needed for its weights now
            const bool blend_next = !(REC_I(nx1, 18) & 4);       // (a centroid at the point of its predecessor keeps the tile)
            CELLW_COEF(cc);
            CELLW_STEP(blend_next);
            cur = nx1; nx1 = nx2;
        }
        {
            // ---- last centroid of the group: the raw registers are free, the next group's rows can be on their way
            const int nx2 = rec_load(rc, cend + 1, nc, lane);
            CELLW_COEF(cend - 1);
            // from here to the first blend of the next run this wave waits for memory: it goes first whenever it can issue
            // (accumulate_multi_kernel's rule; cfg4 171.5 -> 168.6 ms)
            __builtin_amdgcn_s_setprio(1);
            if (compact && cend < nc) desc_expand<true>(ta_n, nx1, lane, pitch, ta_n, tb_n);       // (nx1: the next group's head record)
            if (cend < nc) CELLW_LOAD(REC_I(nx1, 0), REC_I(nx1, 19), REC_I(nx1, 8), ta_n, tb_n);
            CELLW_STEP(false);
            cur = nx1; nx1 = nx2;
        }
        ta = ta_n; tb = tb_n;
        c = cend;
    }
#undef CELLW_LOAD
#undef CELLW_COEF
#undef CELLW_STEP
    // ---- rotation to N/E, signs, store or fused comparator (seismogram.f90:256-283), as accumulate_cell_kernel
    const int nfam = (FUSE && fam_ofs) ? fam_ofs[s + 1] - fam_ofs[s] : 0;
    for (int qf = -1; qf < nfam; qf++) {
        const int js = qf < 0 ? s : fam_list[fam_ofs[s] + qf];
        const int tl = tile * TILE + u0;
        if (!FUSE && tl >= rv.wlen) return;
        float *__restrict__ so = syn + (size_t)js * syn_stride + tl;
        const float a1[SPL] = { ar1[0].x, ar1[0].y }, a2[SPL] = { ar2[0].x, ar2[0].y }, ad[SPL] = { dz[0].x, dz[0].y };
        float mom = 0.f;
        if constexpr (FUSE) mom = fp.moment[fp.isrc0 + js];
        const bool unit = (fp.syn_factor == 1.f);
        for (int k = 0; k < rv.ncomp; k++) {
            const float sg = rv.sign[k];
            float o[SPL];
#pragma unroll
            for (int i = 0; i < SPL; i++) {
                switch (rv.comp[k]) {
                case 1: o[i] = a1[i] * sg; break;
                case 2: o[i] = a2[i] * sg; break;
                case 3: o[i] = ad[i]; break;
                case 4: o[i] = (rv.cl0 * a1[i] - rv.sl0 * a2[i]) * sg; break;
                default: o[i] = (rv.cl0 * a2[i] + rv.sl0 * a1[i]) * sg; break;
                }
            }
            if constexpr (!FUSE) {
#pragma unroll
                for (int i = 0; i < SPL; i++)
                    if (tl + 64 * i < rv.wlen) so[rv.synofs[k] + 64 * i] = o[i];
                continue;
            }
            double acc = 0.0;
            const float *__restrict__ rt = fp.reft + rv.refofs[k] + tl, *__restrict__ tp = fp.tw + rv.refofs[k] + tl;
#pragma unroll
            for (int i = 0; i < SPL; i++) {
                if (tl + 64 * i >= rv.wlen) break;
                const float v = o[i] * mom;
                const float vt = v * tp[64 * i];
                const float a = rt[64 * i];
                switch (fp.method) {
                case 1: { const float d = unit ? (a - vt) : (1.f * a - fp.syn_factor * vt); acc = sq_acc(acc, d); break; }
                case 2: { const float d = unit ? fabsf(a - vt) : fabsf(1.f * a - fp.syn_factor * vt); acc += (double)d; break; }
                case 5: acc += unit ? (double)(a * vt) : (double)(a * 1.f * vt * fp.syn_factor); break;
                default: { const double x = (double)(1.f * a), y = (double)(fp.syn_factor * vt); acc = fmax(acc, sqrt(x * x + y * y)); break; }
                }
            }
            acc = wave_reduce_f64(acc, fp.method == 6);                 // total in lane 63
            if (lane == 63)
                fp.partial[((size_t)js * fp.nmis + rv.slot0 + k) * fp.nparts + tile * (T / 64) + wv] = acc;
        }
    }
}

