// kiwi_outer.hpp -- outer misfit of every trial source under B receiver weightings and the best source of each
// (seismosizer.py:843-922 make_global_misfits, gridsearch.py:199-289 the bootstrap over the receivers).  Included by
// kiwi_hip.hip after the context, so it is compiled with that object's -ffp-contract=off: every fp64 product, sum,
// quotient and root below is rounded on its own, and tests/outer_restatement.py restates each step in the same order
// (the GPU tests ask for bit identity).
//
// Order of work, per chunk of sources (bounded by KIWI_HIP_CHUNK_MB):
//   prepare   per (source s, receiver r): the receiver's slots folded (l1norm: sums; l2norm: roots of sums of squares),
//             the receiver weight (anarchy: w / norm, clipped at zero), a = M rw, b = N rw (squared under l2norm),
//             stored receiver-major, a[r][s], so that the draw pass reads them coalesced over the sources
//   draw      a workgroup owns 256 sources x 8 draws, keeps the 8 weight rows c[d][0..nrec) in LDS and every thread
//             one source with 2 x 8 accumulators: ms = sum_r a c, ns = sum_r b c (r ascending, from zero),
//             g = ms / ns (root under l2norm); the (value, source index) minimum over the workgroup's sources goes to a
//             [tile][draw] slab -- the [source][draw] matrix is never written.  The g of ONE chosen draw may be written.
//   reduce    one thread per draw folds the slab's tiles into the running best of the call.
// No float atomics: nothing depends on arrival order.  Among equal values the LOWEST source index wins at every level
// (numpy's nanargmin), the order (excluded last, then value, then index) is total, so the answer does not depend on the
// tile shape, the chunking, or how a list is cut into shards.  Excluded: ns <= 0, g < 0, g NaN.
//
// The host path multiplies the receiver weight by sqrt(c) before squaring under l2norm; here the square is multiplied
// by c -- a difference of a few ulp.

namespace outer {

constexpr int kTileS = 256;          // sources per workgroup, one per thread
constexpr int kTileD = 8;            // draws per workgroup: 16 fp64 accumulators per thread
constexpr int kMaxRec = 512;         // receivers: the tile's weight rows, kMaxRec x kTileD doubles = 32 KiB of LDS

// (excluded last, value ascending, index ascending): is (v1, i1) before (v2, i2)?  NaN marks "no candidate"
__device__ __forceinline__ bool before(double v1, int i1, double v2, int i2)
{
    if (v1 != v1) return false;
    if (v2 != v2) return true;
    return v1 < v2 || (v1 == v2 && i1 < i2);
}

__global__ __launch_bounds__(256) void outer_prepare_kernel(const float *__restrict__ mis, const float *__restrict__ nor,
                                                            const int *__restrict__ rec_first, const double *__restrict__ w,
                                                            int ns, int nmis, int nrec, int l2, int anarchy,
                                                            double *__restrict__ a, double *__restrict__ b)
{
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= (long long)ns * nrec) return;
    const int s = (int)(i / nrec), r = (int)(i % nrec);
    const float *m = mis + (size_t)s * nmis, *n = nor + (size_t)s * nmis;
    double M = 0.0, N = 0.0;
    for (int k = rec_first[r]; k < rec_first[r + 1]; k++) {
        const double mv = (double)m[k], nv = (double)n[k];
        if (l2) { M = M + mv * mv; N = N + nv * nv; }
        else { M = M + mv; N = N + nv; }
    }
    if (l2) { M = sqrt(M); N = sqrt(N); }
    double rw = w[r];
    if (anarchy) {
        const double q = rw / (N != 0.0 ? N : -1.0);
        rw = (q > 0.0 || q != q) ? q : 0.0;              // numpy's maximum(q, 0): a NaN stays
    }
    double av = M * rw, bv = N * rw;
    if (l2) { av = av * av; bv = bv * bv; }
    a[(size_t)r * ns + s] = av;
    b[(size_t)r * ns + s] = bv;
}

// slab_v / slab_i: [ntiles][ndraw]; src0: index of the chunk's first source in the whole list; gout: [ns] of this chunk
__global__ __launch_bounds__(256) void outer_draw_kernel(const double *__restrict__ a, const double *__restrict__ b,
                                                         const double *__restrict__ cw, int ns, int nrec, int ndraw, int ngroups,
                                                         int l2, int src0, double *__restrict__ slab_v, int *__restrict__ slab_i,
                                                         int which_draw, double *__restrict__ gout)
{
    __shared__ double cs[kMaxRec * kTileD];              // [r][j]
    __shared__ double red_v[kTileS / 64][kTileD];
    __shared__ int red_i[kTileS / 64][kTileD];
    const int tile = (int)(blockIdx.x / (unsigned)ngroups), grp = (int)(blockIdx.x % (unsigned)ngroups);
    const int d0 = grp * kTileD, tid = (int)threadIdx.x;
    for (int i = tid; i < nrec * kTileD; i += kTileS) {
        const int j = i / nrec, r = i - j * nrec;
        cs[r * kTileD + j] = d0 + j < ndraw ? cw[(size_t)(d0 + j) * nrec + r] : 0.0;
    }
    __syncthreads();
    const int s = tile * kTileS + tid;
    const bool live = s < ns;
    double ms[kTileD], nn[kTileD];
#pragma unroll
    for (int j = 0; j < kTileD; j++) { ms[j] = 0.0; nn[j] = 0.0; }
    if (live) {
        const double *ap = a + s, *bp = b + s;
        for (int r = 0; r < nrec; r++) {
            const double av = ap[(size_t)r * ns], bv = bp[(size_t)r * ns];
            const double *c = cs + r * kTileD;
#pragma unroll
            for (int j = 0; j < kTileD; j++) {
                const double cj = c[j];
                ms[j] = ms[j] + av * cj;
                nn[j] = nn[j] + bv * cj;
            }
        }
    }
    const double nan = __longlong_as_double(0x7ff8000000000000LL);
    const int lane = tid & 63, wave = tid >> 6;
#pragma unroll
    for (int j = 0; j < kTileD; j++) {
        double g = nan;
        if (live && nn[j] > 0.0) {
            g = ms[j] / nn[j];
            if (l2) g = sqrt(g);
            if (!(g >= 0.0)) g = nan;                    // negative or NaN: excluded, as the host turns it into NaN
        }
        if (live && gout && d0 + j == which_draw) gout[s] = g;
        double v = g;
        int idx = src0 + s;
        for (int off = 32; off > 0; off >>= 1) {
            const double v2 = __shfl_down(v, off, 64);
            const int i2 = __shfl_down(idx, off, 64);
            if (before(v2, i2, v, idx)) { v = v2; idx = i2; }
        }
        if (lane == 0) { red_v[wave][j] = v; red_i[wave][j] = idx; }
    }
    __syncthreads();
    if (tid < kTileD && d0 + tid < ndraw) {
        double v = red_v[0][tid];
        int idx = red_i[0][tid];
        for (int wv = 1; wv < kTileS / 64; wv++)
            if (before(red_v[wv][tid], red_i[wv][tid], v, idx)) { v = red_v[wv][tid]; idx = red_i[wv][tid]; }
        slab_v[(size_t)tile * ndraw + d0 + tid] = v;
        slab_i[(size_t)tile * ndraw + d0 + tid] = (v != v) ? 0 : idx;
    }
}

// best_v / best_i [ndraw]: the running best of the call (NaN / 0 before the first chunk)
__global__ __launch_bounds__(256) void outer_reduce_kernel(const double *__restrict__ slab_v, const int *__restrict__ slab_i,
                                                           int ntiles, int ndraw, double *__restrict__ best_v,
                                                           int *__restrict__ best_i)
{
    const int d = (int)(blockIdx.x * 256 + threadIdx.x);
    if (d >= ndraw) return;
    double v = best_v[d];
    int idx = best_i[d];
    for (int t = 0; t < ntiles; t++) {
        const double v2 = slab_v[(size_t)t * ndraw + d];
        const int i2 = slab_i[(size_t)t * ndraw + d];
        if (before(v2, i2, v, idx)) { v = v2; idx = i2; }
    }
    best_v[d] = v;
    best_i[d] = (v != v) ? 0 : idx;
}

__global__ __launch_bounds__(256) void outer_init_kernel(double *__restrict__ best_v, int *__restrict__ best_i, int ndraw)
{
    const int d = (int)(blockIdx.x * 256 + threadIdx.x);
    if (d >= ndraw) return;
    best_v[d] = __longlong_as_double(0x7ff8000000000000LL);
    best_i[d] = 0;
}

// the whole call on host arrays; ms[3]: upload, kernels, download of this call (HIP events on the context's stream)
static void run(kiwi_hip_ctx *c, int nsrc, int nmis, int nrec, const int *slot_receiver, const float *misfit, const float *norm,
                int outer_norm, const double *receiver_weights, int anarchy, int ndraw, const double *draw_weights,
                double *best_value, int *best_index, int which_draw, double *global_of_draw)
{
    if (nsrc < 0 || nmis < 0 || nrec < 0 || ndraw < 0) throw std::runtime_error("outer_misfits: negative count");
    if (outer_norm != 1 && outer_norm != 2) throw std::runtime_error("outer_misfits: unknown norm method (1 l1norm, 2 l2norm)");
    if (nrec > kMaxRec)
        throw std::runtime_error("outer_misfits: " + std::to_string(nrec) + " receivers; the draw tile keeps 8 weight rows in LDS and takes at most " +
                                 std::to_string(kMaxRec));
    if (nmis > 0 && !slot_receiver) throw std::runtime_error("outer_misfits: null slot_receiver");
    if (nsrc > 0 && nmis > 0 && (!misfit || !norm)) throw std::runtime_error("outer_misfits: null misfit or norm array");
    if (ndraw > 0 && (!best_value || !best_index || (nrec > 0 && !draw_weights))) throw std::runtime_error("outer_misfits: null draw array");
    if (global_of_draw && (which_draw < 0 || which_draw >= ndraw)) throw std::runtime_error("outer_misfits: which_draw out of range");
    std::vector<int> rec_first((size_t)nrec + 1, 0);
    for (int k = 0; k < nmis; k++) {
        const int r = slot_receiver[k];
        if (r < 0 || r >= nrec) throw std::runtime_error("outer_misfits: slot_receiver out of range at slot " + std::to_string(k + 1));
        if (k > 0 && r < slot_receiver[k - 1]) throw std::runtime_error("outer_misfits: slot_receiver not ascending at slot " + std::to_string(k + 1));
        rec_first[(size_t)r + 1]++;
    }
    for (int r = 0; r < nrec; r++) rec_first[(size_t)r + 1] += rec_first[r];
    c->outer_ms[0] = c->outer_ms[1] = c->outer_ms[2] = 0.f;
    const double nan = std::numeric_limits<double>::quiet_NaN();
    for (int d = 0; d < ndraw; d++) { best_value[d] = nan; best_index[d] = 0; }
    if (global_of_draw) for (int s = 0; s < nsrc; s++) global_of_draw[s] = nan;
    if (ndraw == 0 || nsrc == 0) return;

    const int ngroups = (ndraw + kTileD - 1) / kTileD;
    // per source of a chunk: two float rows up, a and b, the chosen draw's g, and its share of the slab
    const size_t per_src = (size_t)nmis * 2 * sizeof(float) + (size_t)nrec * 2 * sizeof(double) + sizeof(double) +
                           ((size_t)ndraw * (sizeof(double) + sizeof(int)) + kTileS - 1) / kTileS;
    long long chunk = (long long)std::max<size_t>(1, c->chunk_bytes_limit / per_src);
    const long long max_tiles = std::max<long long>(1, ((long long)1 << 30) / ngroups);     // the grid is tiles x draw groups
    chunk = std::min<long long>(chunk, max_tiles * kTileS);
    if (chunk >= kTileS) chunk -= chunk % kTileS;
    chunk = std::min<long long>(chunk, nsrc);
    const int ntiles_max = (int)((chunk + kTileS - 1) / kTileS);

    std::vector<double> ones;
    if (!receiver_weights) { ones.assign((size_t)nrec, 1.0); receiver_weights = ones.data(); }
    DevBuf<float> m_d, n_d;
    DevBuf<double> a_d, b_d, w_d, cw_d, slabv_d, bestv_d, g_d;
    DevBuf<int> first_d, slabi_d, besti_d;
    m_d.alloc((size_t)chunk * nmis, &c->dev_bytes); n_d.alloc((size_t)chunk * nmis, &c->dev_bytes);
    a_d.alloc((size_t)chunk * nrec, &c->dev_bytes); b_d.alloc((size_t)chunk * nrec, &c->dev_bytes);
    w_d.alloc((size_t)nrec, &c->dev_bytes); cw_d.alloc((size_t)ndraw * nrec, &c->dev_bytes);
    first_d.alloc((size_t)nrec + 1, &c->dev_bytes);
    slabv_d.alloc((size_t)ntiles_max * ndraw, &c->dev_bytes); slabi_d.alloc((size_t)ntiles_max * ndraw, &c->dev_bytes);
    bestv_d.alloc((size_t)ndraw, &c->dev_bytes); besti_d.alloc((size_t)ndraw, &c->dev_bytes);
    if (global_of_draw) g_d.alloc((size_t)chunk, &c->dev_bytes);

    const PooledEvents<4> ev(c);
    HIPCHECK(hipEventRecord(ev[0], c->stream));
    if (nrec > 0) {
        HIPCHECK(hipMemcpyAsync(w_d.p, receiver_weights, (size_t)nrec * sizeof(double), hipMemcpyHostToDevice, c->stream));
        HIPCHECK(hipMemcpyAsync(cw_d.p, draw_weights, (size_t)ndraw * nrec * sizeof(double), hipMemcpyHostToDevice, c->stream));
    }
    HIPCHECK(hipMemcpyAsync(first_d.p, rec_first.data(), ((size_t)nrec + 1) * sizeof(int), hipMemcpyHostToDevice, c->stream));
    HIPCHECK(hipEventRecord(ev[1], c->stream));
    hipLaunchKernelGGL(outer_init_kernel, dim3((unsigned)((ndraw + 255) / 256)), dim3(256), 0, c->stream, bestv_d.p, besti_d.p, ndraw);
    HIPCHECK(hipGetLastError());
    HIPCHECK(hipEventRecord(ev[2], c->stream));
    HIPCHECK(hipStreamSynchronize(c->stream));
    ev.add_elapsed(c->outer_ms, 0, 0, 1);
    ev.add_elapsed(c->outer_ms, 1, 1, 2);
    for (long long s0 = 0; s0 < nsrc; s0 += chunk) {
        const int ns = (int)std::min<long long>(chunk, nsrc - s0);
        const int ntiles = (ns + kTileS - 1) / kTileS;
        HIPCHECK(hipEventRecord(ev[0], c->stream));
        if (nmis > 0) {
            HIPCHECK(hipMemcpyAsync(m_d.p, misfit + (size_t)s0 * nmis, (size_t)ns * nmis * sizeof(float), hipMemcpyHostToDevice, c->stream));
            HIPCHECK(hipMemcpyAsync(n_d.p, norm + (size_t)s0 * nmis, (size_t)ns * nmis * sizeof(float), hipMemcpyHostToDevice, c->stream));
        }
        HIPCHECK(hipEventRecord(ev[1], c->stream));
        if (nrec > 0) {
            const long long total = (long long)ns * nrec;
            hipLaunchKernelGGL(outer_prepare_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, c->stream, m_d.p, n_d.p,
                               first_d.p, w_d.p, ns, nmis, nrec, outer_norm == 2, anarchy ? 1 : 0, a_d.p, b_d.p);
            HIPCHECK(hipGetLastError());
        }
        hipLaunchKernelGGL(outer_draw_kernel, dim3((unsigned)((long long)ntiles * ngroups)), dim3(kTileS), 0, c->stream, a_d.p, b_d.p,
                           cw_d.p, ns, nrec, ndraw, ngroups, outer_norm == 2, (int)s0, slabv_d.p, slabi_d.p,
                           global_of_draw ? which_draw : -1, global_of_draw ? g_d.p : (double *)nullptr);
        HIPCHECK(hipGetLastError());
        hipLaunchKernelGGL(outer_reduce_kernel, dim3((unsigned)((ndraw + 255) / 256)), dim3(256), 0, c->stream, slabv_d.p, slabi_d.p,
                           ntiles, ndraw, bestv_d.p, besti_d.p);
        HIPCHECK(hipGetLastError());
        HIPCHECK(hipEventRecord(ev[2], c->stream));
        if (global_of_draw)
            HIPCHECK(hipMemcpyAsync(global_of_draw + s0, g_d.p, (size_t)ns * sizeof(double), hipMemcpyDeviceToHost, c->stream));
        HIPCHECK(hipEventRecord(ev[3], c->stream));
        HIPCHECK(hipStreamSynchronize(c->stream));
        ev.add_elapsed(c->outer_ms, 0, 0, 1);
        ev.add_elapsed(c->outer_ms, 1, 1, 2);
        ev.add_elapsed(c->outer_ms, 2, 2, 3);
    }
    HIPCHECK(hipEventRecord(ev[0], c->stream));
    HIPCHECK(hipMemcpyAsync(best_value, bestv_d.p, (size_t)ndraw * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIPCHECK(hipMemcpyAsync(best_index, besti_d.p, (size_t)ndraw * sizeof(int), hipMemcpyDeviceToHost, c->stream));
    HIPCHECK(hipEventRecord(ev[1], c->stream));
    HIPCHECK(hipStreamSynchronize(c->stream));
    ev.add_elapsed(c->outer_ms, 2, 0, 1);
}

} // namespace outer
