// kiwi_gfk.hpp -- Gulunay f-k densification of an installed database (set_database dbpath nipx nipz; gfdb.f90:1109-1310,
// interpolation.f90:29-311).  Included by kiwi_hip.hip after the context, so it is compiled with that object's
// -ffp-contract=off: every fp32 product and sum below is rounded on its own, and tests/gfk_restatement.py restates each
// step in the same order (the GPU tests ask for bit identity).
//
// Order of work: the stored database is installed through kiwi_hip_set_gfdb; the densification reads its padded rows
// (kRowPad zeros | samples | repeated end value), which hold exactly what trace_multiply_add_nogrow puts into a block's
// field; the dense traces are downloaded and installed through kiwi_hip_set_gfdb again (one install path).
//
// Per block (128 distances x 32 depths, overlaps 32 / 8; an axis with factor 1 has block 1) and component the field is
// gathered over the block's time window, then one or two gulunay passes run over a batch of fields of equal window
// length:
//   taper (cosine tables made on the host from glibc cosf, as written) -> time transforms of the input columns, length T
//   (B) and l*T zero-padded (C, D), rows 0..T/2 kept -> B, C, D spread over the fine grid (zeros where the reference
//   inserts zero traces or leaves its work arrays unset) -> depth and distance transforms -> noise floor on D from the
//   maximum of row T/2, operator C/D, clip, B*Op/N -> inverse distance and depth transforms -> Hermitian extension,
//   inverse time transform, real part.
// Transforms are radix-2 Stockham passes over global memory, batched over every line of every field, twiddles from an
// fp64 table rounded to fp32.  Magnitudes are a scaled hypot and divisions Smith's formula: the synthetic databases
// carry amplitudes near 1e-20, where re*re+im*im underflows.

namespace gfk {

constexpr int kBlockX = 128, kOverlapX = 32;     // gfdb.f90:31-33
constexpr int kBlockZ = 32, kOverlapZ = 8;       // gfdb.f90:35-37
constexpr float kPi = 3.14159265358979f;         // constants.f90:21 (a default real)

__device__ __forceinline__ float habs(float re, float im)
{
    const float a = fabsf(re), b = fabsf(im);
    const float mx = fmaxf(a, b), mn = fminf(a, b);
    if (mx == 0.f) return 0.f;
    const float r = mn / mx;
    return mx * sqrtf(1.f + r * r);
}

__device__ __forceinline__ float2 smith_div(float2 n, float2 d)
{
    float2 o;
    if (fabsf(d.x) >= fabsf(d.y)) {
        const float r = d.y / d.x, den = d.x + d.y * r;
        o.x = (n.x + n.y * r) / den;
        o.y = (n.y - n.x * r) / den;
    } else {
        const float r = d.x / d.y, den = d.x * r + d.y;
        o.x = (n.x * r + n.y) / den;
        o.y = (n.y * r - n.x) / den;
    }
    return o;
}

// field_orig of a batch of (block, component) fields, A[f][x][z][t]: the stored neighbour of every local position
// (edges repeated) read over the window [w0, w0+T): zeros before the trace, its end value after it, zeros for a trace
// that is not stored
__global__ void gather_kernel(float *__restrict__ A, const float *__restrict__ G, const int2 *__restrict__ span, int pitch,
                              const int *__restrict__ fblk, const int *__restrict__ fig, const int *__restrict__ bnode,
                              const int *__restrict__ bw0, int ng, int Sx, int Sz, int T, long long total)
{
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= total) return;
    const int t = (int)(i % T);
    long long r = i / T;
    const int z = (int)(r % Sz); r /= Sz;
    const int x = (int)(r % Sx);
    const int f = (int)(r / Sx);
    const int b = fblk[f];
    const long long row = (long long)bnode[((long long)b * Sx + x) * Sz + z] * ng + fig[f];
    const int2 sp = span[row];
    const int n = sp.y - sp.x + 1;
    const int k = bw0[b] + t - sp.x;
    float v = 0.f;
    if (n > 0 && k >= 0) v = G[row * pitch + kRowPad + (k < n ? k : n - 1)];
    A[i] = 0.f + v;
}

// tapers (distance, depth, time; each a multiply, then / 2) and the complex inputs of the time transforms:
// XB[col][0..T) and XC[col][0..l*T) zero-padded, col = (f*Sx + x)*Sz + z
__global__ void load_kernel(const float *__restrict__ A, float2 *__restrict__ XB, float2 *__restrict__ XC,
                            const float *__restrict__ tap, int Sx, int Sz, int T, int l, int cx, int cz, int ct,
                            long long total)
{
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= total) return;
    const int t = (int)(i % T);
    const long long col = i / T;
    const int z = (int)(col % Sz);
    const int x = (int)((col / Sz) % Sx);
    const float *wxs = tap, *wxe = tap + Sx, *wzs = tap + 2 * Sx, *wze = wzs + Sz, *wts = wzs + 2 * Sz, *wte = wts + T;
    float a = A[i];
    if (x < cx) a = (a * wxs[x]) / 2.f;
    if (x >= Sx - cx) a = (a * wxe[x]) / 2.f;
    if (z < cz) a = (a * wzs[z]) / 2.f;
    if (z >= Sz - cz) a = (a * wze[z]) / 2.f;
    if (t < ct) a = (a * wts[t]) / 2.f;
    if (t >= T - ct) a = (a * wte[t]) / 2.f;
    XB[i] = make_float2(a, 0.f);
    float2 *c = XC + col * (long long)l * T;
    c[t] = make_float2(a, 0.f);
    for (int j = t + T; j < l * T; j += T) c[j] = make_float2(0.f, 0.f);
}

// one radix-2 Stockham pass over lines of length N with element stride S (line = outer*N*S + inner):
// a = x[q+s*p], b = x[q+s*(p+N/(2s))]; y[q+s*2p] = a+b, y[q+s*(2p+1)] = (a-b)*w^(p*s)
__global__ void fft_pass_kernel(const float2 *__restrict__ in, float2 *__restrict__ out, const float2 *__restrict__ tw,
                                int N, int m, int s, long long S, float wsign, long long total)
{
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= total) return;
    const long long inner = i % S;
    long long r = i / S;
    const int q = (int)(r % s); r /= s;
    const int p = (int)(r % m);
    const long long outer = r / m;
    const long long base = outer * N * S + inner;
    const float2 a = in[base + (long long)(q + s * p) * S];
    const float2 b = in[base + (long long)(q + s * (p + m)) * S];
    const float2 w = tw[p * s];
    const float wr = w.x, wi = w.y * wsign;
    const float dr = a.x - b.x, di = a.y - b.y;
    out[base + (long long)(q + 2 * s * p) * S] = make_float2(a.x + b.x, a.y + b.y);
    out[base + (long long)(q + s * (2 * p + 1)) * S] = make_float2(dr * wr - di * wi, dr * wi + di * wr);
}

// B, C, D on the fine grid, rows 0..T/2: [f][x][z][r]
__global__ void spread_kernel(const float2 *__restrict__ XB, const float2 *__restrict__ XC, float2 *__restrict__ fB,
                              float2 *__restrict__ fC, float2 *__restrict__ fD, int Sx, int Sz, int lx, int lz, int T,
                              long long total)
{
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= total) return;
    const int H = T / 2 + 1, Kx = Sx * lx, Kz = Sz * lz, l = lx > lz ? lx : lz;
    const int rr = (int)(i % H);
    long long r = i / H;
    const int z = (int)(r % Kz); r /= Kz;
    const int x = (int)(r % Kx);
    const long long f = r / Kx;
    const float2 zero = make_float2(0.f, 0.f);
    const bool on = (x % lx == 0) && (z % lz == 0), in = x < Sx && z < Sz;
    fB[i] = on ? XB[((f * Sx + x / lx) * Sz + z / lz) * T + rr] : zero;
    const float2 c = in ? XC[((f * Sx + x) * Sz + z) * (long long)l * T + rr] : zero;
    fC[i] = c;
    fD[i] = (in && on) ? c : zero;
}

// max |fD(T/2, :, :)| of every field (one workgroup per field; max is exact, so the order does not matter)
__global__ __launch_bounds__(256) void nyquist_max_kernel(const float2 *__restrict__ fD, float *__restrict__ mx, int KxKz, int H)
{
    __shared__ float red[256];
    const long long f = blockIdx.x;
    float m = 0.f;
    for (int j = threadIdx.x; j < KxKz; j += 256) {
        const float2 d = fD[(f * KxKz + j) * H + H - 1];
        m = fmaxf(m, habs(d.x, d.y));
    }
    red[threadIdx.x] = m;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w) red[threadIdx.x] = fmaxf(red[threadIdx.x], red[threadIdx.x + w]);
        __syncthreads();
    }
    if (threadIdx.x == 0) mx[f] = red[0];
}

// noise floor, operator, clip, product and scale (interpolation.f90:117-146, :270-300); the result replaces fB
__global__ void operator_kernel(float2 *__restrict__ fB, const float2 *__restrict__ fC, const float2 *__restrict__ fD,
                                const float *__restrict__ mx, long long per_field, float clip, float N, long long total)
{
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= total) return;
    const float m = 0.01f * mx[i / per_field];
    float2 d = fD[i];
    float a = habs(d.x, d.y);
    if (a < m / 1000.f) d.x = m;
    a = habs(d.x, d.y);
    if (a < m) { const float r = m / a; d.x = r * d.x; d.y = r * d.y; }
    // a zero denominator survives the noise floor when m == 0 (a band-limited field whose row T/2 rounds to exact zeros):
    // such a bin, and a quotient that overflows, gets no operator -- the reference's fC/fD would be 0/0 or x/0 there
    float2 op = make_float2(0.f, 0.f);
    if (d.x != 0.f || d.y != 0.f) {
        op = smith_div(fC[i], d);
        if (!isfinite(op.x) || !isfinite(op.y)) op = make_float2(0.f, 0.f);
    }
    a = habs(op.x, op.y);
    if (a > clip) { const float r = clip / a; op.x = r * op.x; op.y = r * op.y; }
    a = habs(op.x, op.y);
    if (a < clip * 0.5f) op = make_float2(0.f, 0.f);
    const float2 b = fB[i];
    fB[i] = make_float2((b.x * op.x - b.y * op.y) / N, (b.x * op.y + b.y * op.x) / N);
}

// half spectrum in time -> full Hermitian spectrum: [line][0..T)
__global__ void hermitian_kernel(const float2 *__restrict__ h, float2 *__restrict__ full, int T, long long total)
{
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= total) return;
    const int H = T / 2 + 1;
    const int k = (int)(i % T);
    const long long line = i / T;
    if (k < H) full[i] = h[line * H + k];
    else { const float2 v = h[line * H + (T - k)]; full[i] = make_float2(v.x, -v.y); }
}

__global__ void real_part_kernel(const float2 *__restrict__ in, float *__restrict__ out, long long total)
{
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < total) out[i] = in[i].x;
}

// unequal factors: the horizontal inputs, one field per (field, stored depth row): H[(f*Sz + z)][x][t] = A[f][x][z][t]
__global__ void hslice_kernel(const float *__restrict__ A, float *__restrict__ Hin, int Sx, int Sz, int T, long long total)
{
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= total) return;
    const int t = (int)(i % T);
    long long r = i / T;
    const int x = (int)(r % Sx); r /= Sx;
    const int z = (int)(r % Sz);
    const long long f = r / Sz;
    Hin[i] = A[((f * Sx + x) * Sz + z) * T + t];
}

// ... and the vertical inputs, one field per (field, output column): the stored column ix_in when mod(ix_in-1,nipx) == 0
// (gfdb.f90:1301, imitated), else the horizontally interpolated column: V[(f*Kx + xo)][z][t]
__global__ void vselect_kernel(const float *__restrict__ A, const float *__restrict__ Hout, float *__restrict__ V, int Sx,
                               int Sz, int Kx, int nipx, int T, long long total)
{
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= total) return;
    const int t = (int)(i % T);
    long long r = i / T;
    const int z = (int)(r % Sz); r /= Sz;
    const int xo = (int)(r % Kx);
    const long long f = r / Kx;
    const int xi = xo / nipx;
    V[i] = (xi % nipx == 0) ? A[((f * Sx + xi) * Sz + z) * T + t] : Hout[((f * Sz + z) * Kx + xo) * T + t];
}

struct WriteRec { long long src, dst; int n, pad; };

// payload traces into the dense rows (one workgroup per trace)
__global__ __launch_bounds__(256) void writeback_kernel(const float *__restrict__ out, float *__restrict__ dense,
                                                        const WriteRec *__restrict__ w)
{
    const WriteRec r = w[blockIdx.x];
    for (int k = threadIdx.x; k < r.n; k += 256) dense[r.dst + k] = out[r.src + k];
}

// ------------------------------------------------------------------------------------------------ host side

inline unsigned nblocks_for(long long total) { return (unsigned)((total + 255) / 256); }

inline std::string check_factors(int nipx, int nipz)
{
    if (nipx < 1 || nipz < 1) return "set_database: nipx and nipz must be positive";     // minimizer.f90:143-146
    auto bad = [](int v, int top) { return v > top || (v & (v - 1)) != 0; };
    // gulunay2d dies unless the coarse block width divides the fine one (interpolation.f90:55,191)
    if (bad(nipx, kBlockX)) return "set_database: nipx must be a power of two up to 128 (the interpolation block is 128 traces wide)";
    if (bad(nipz, kBlockZ)) return "set_database: nipz must be a power of two up to 32 (the interpolation block is 32 traces wide)";
    return "";
}

// gfdb.f90:1313-1339 in default reals
inline int next_power_of_two(int n)
{
    const float q = logf((float)n) / logf(2.f);
    return 1 << (int)std::ceil(q);
}

struct Write { int ixd, izd, lx, lz, d0, d1; };      // dense 0-based position, local position, data span
struct Block {
    int ixfirst = 0, izfirst = 0;                    // 1-based dense, gfdb.f90:1127-1135
    int w0 = 0, T = 0, ntmargin = 0;
    std::vector<int> node;                           // [Sx][Sz] coarse node (cx*nz + cz) of each stored local position
    std::vector<Write> writes;
};

struct Plan {
    int nx, nz, ng, nipx, nipz, NX, NZ;
    int bx, px, ox, bz, pz, oz, Sx, Sz;
    std::vector<Block> blocks;
};

inline Plan make_plan(int nx, int nz, int ng, int nipx, int nipz, const int *first, const int *nsamp)
{
    Plan P{};
    P.nx = nx; P.nz = nz; P.ng = ng; P.nipx = nipx; P.nipz = nipz; P.NX = nx * nipx; P.NZ = nz * nipz;
    if (nipx != 1) { P.bx = kBlockX; P.ox = kOverlapX; } else { P.bx = 1; P.ox = 0; }
    if (nipz != 1) { P.bz = kBlockZ; P.oz = kOverlapZ; } else { P.bz = 1; P.oz = 0; }
    P.px = P.bx - P.ox; P.pz = P.bz - P.oz;
    P.Sx = P.bx / nipx; P.Sz = P.bz / nipz;
    auto coarse = [](int i, int n, int nip) { return (std::min(std::max(i, 1), n) - 1) / nip; };   // gfdb.f90:1141-1142
    const int nbx = (P.NX + P.px - 1) / P.px, nbz = (P.NZ + P.pz - 1) / P.pz;
    for (int ibx = 0; ibx < nbx; ibx++)
        for (int ibz = 0; ibz < nbz; ibz++) {
            Block b;
            b.ixfirst = ibx * P.px + 1 - P.ox / 2;
            b.izfirst = ibz * P.pz + 1 - P.oz / 2;
            b.node.resize((size_t)P.Sx * P.Sz);
            // spans(:,iz,ix) keeps the last component's span (the component loop overwrites it, gfdb.f90:1147-1156)
            std::vector<int2> sp((size_t)P.Sx * P.Sz);
            std::vector<char> has((size_t)P.Sx * P.Sz, 0);
            long long lo = LLONG_MAX, hi = LLONG_MIN;
            for (int x = 0; x < P.Sx; x++)
                for (int z = 0; z < P.Sz; z++) {
                    const int cx = coarse(b.ixfirst + x * nipx, P.NX, nipx), cz = coarse(b.izfirst + z * nipz, P.NZ, nipz);
                    const int node = cx * nz + cz;
                    b.node[(size_t)x * P.Sz + z] = node;
                    for (int ig = 0; ig < ng; ig++) {
                        const size_t row = (size_t)node * ng + ig;
                        if (nsamp[row] <= 0) continue;       // missing: nothing to the union (decision b)
                        lo = std::min<long long>(lo, first[row]);
                        hi = std::max<long long>(hi, (long long)first[row] + nsamp[row] - 1);
                    }
                    const size_t last = (size_t)node * ng + ng - 1;
                    if (nsamp[last] > 0) { has[(size_t)x * P.Sz + z] = 1; sp[(size_t)x * P.Sz + z] = make_int2(first[last], first[last] + nsamp[last] - 1); }
                }
            if (lo != LLONG_MAX) {
                // allowed_span(span, min(64, int(1.2*(span(2)-span(1))))), gfdb.f90:1159
                const int s1 = (int)lo, s2 = (int)hi;
                const int minlen = std::min(64, (int)((float)(s2 - s1) * 1.2f));
                int length = s2 - s1 + 1;
                if (length < minlen) length = minlen;
                const int lp = next_power_of_two(length);
                b.w0 = s1 - (lp - length) / 2;
                b.T = lp;
                b.ntmargin = (int)(0.1f * (float)(lp - 1));
            }
            if (b.T > 1) {                                   // gfdb.f90:1163
                for (int lz = P.oz / 2; lz < P.bz - P.oz / 2; lz++)
                    for (int lx = P.ox / 2; lx < P.bx - P.ox / 2; lx++) {
                        const int ix = b.ixfirst + lx, iz = b.izfirst + lz;
                        if ((ix - 1) % nipx == 0 && (iz - 1) % nipz == 0) continue;
                        if (ix < 1 || ix > P.NX || iz < 1 || iz > P.NZ) continue;
                        const int ax = (lx / nipx) * nipx, az = (lz / nipz) * nipz;
                        int d0 = INT_MAX, d1 = INT_MIN;
                        auto take = [&](int x, int z) {
                            const size_t k = (size_t)(x / nipx) * P.Sz + z / nipz;
                            if (!has[k]) return;
                            d0 = std::min(d0, sp[k].x); d1 = std::max(d1, sp[k].y);
                        };
                        take(ax, az);
                        if (ax + nipx < P.bx) take(ax + nipx, az);
                        if (az + nipz < P.bz) take(ax, az + nipz);
                        if (ax + nipx < P.bx && az + nipz < P.bz) take(ax + nipx, az + nipz);
                        if (d0 == INT_MAX) continue;             // every neighbour missing: stays missing
                        b.writes.push_back(Write{ ix - 1, iz - 1, lx, lz, d0, d1 });
                    }
            }
            P.blocks.push_back(std::move(b));
        }
    return P;
}

// cosine taper tables of one axis of length S (interpolation.f90:67-81): start and end weights
inline void taper_table(int S, int margin, int l, float *ws, float *we, int &cnt)
{
    cnt = margin / l;
    for (int i = 0; i < S; i++) { ws[i] = 1.f; we[i] = 1.f; }
    auto w = [&](int i) {
        const float den = (2.f * (float)margin) / (float)l;
        const float q = (float)i / den;
        return 1.f - cosf((2.f * kPi) * q);
    };
    for (int x = 1; x <= cnt; x++) if (x <= S) ws[x - 1] = w(x - 1);
    for (int x = S - cnt + 1; x <= S; x++) if (x >= 1) we[x - 1] = w(S - x);
}

struct Work {
    kiwi_hip_ctx *c;
    std::map<int, DevBuf<float2>> tw;
    DevBuf<float2> XB, XC, fB, fC, fD, tmp, full;
    DevBuf<float> tap, mx;

    const float2 *twiddles(int N)
    {
        auto it = tw.find(N);
        if (it != tw.end()) return it->second.p;
        std::vector<float2> h(std::max(1, N / 2));
        for (int k = 0; k < (int)h.size(); k++) {
            const double a = 2.0 * M_PI * (double)k / (double)N;
            h[k] = make_float2((float)std::cos(a), (float)(-std::sin(a)));
        }
        DevBuf<float2> &d = tw[N];
        d.alloc(h.size(), &c->dev_bytes);
        HIPCHECK(hipMemcpyAsync(d.p, h.data(), h.size() * sizeof(float2), hipMemcpyHostToDevice, c->stream));
        return d.p;
    }

    // in-place transform of `lines` lines of length N, element stride S, batched (result back in buf)
    void fft(float2 *buf, long long elems, int N, long long S, bool inverse)
    {
        if (N <= 1) return;
        tmp.ensure((size_t)elems, &c->dev_bytes);
        const float2 *w = twiddles(N);
        float2 *a = buf, *b = tmp.p;
        const long long nbf = elems / 2;
        for (int n = N, s = 1; n > 1; n /= 2, s *= 2) {
            hipLaunchKernelGGL(fft_pass_kernel, dim3(nblocks_for(nbf)), dim3(256), 0, c->stream, a, b, w, N, n / 2, s, S,
                               inverse ? -1.f : 1.f, nbf);
            std::swap(a, b);
        }
        if (a != buf) HIPCHECK(hipMemcpyAsync(buf, a, (size_t)elems * sizeof(float2), hipMemcpyDeviceToDevice, c->stream));
    }

    // one gulunay2d (lx or lz == 1) or gulunay3d (lx == lz) call on F fields A[f][x][z][t] -> out[f][lx*x][lz*z][t]
    void pass(const float *A, float *out, long long F, int Sx, int Sz, int T, int lx, int lz, int mx_, int mz_, int mt)
    {
        const int l = std::max(lx, lz), Kx = Sx * lx, Kz = Sz * lz, H = T / 2 + 1;
        std::vector<float> th(2 * (size_t)Sx + 2 * (size_t)Sz + 2 * (size_t)T);
        int cx = 0, cz = 0, ct = 0;
        float *p = th.data();
        if (lx > 1) taper_table(Sx, mx_, l, p, p + Sx, cx); else for (int i = 0; i < 2 * Sx; i++) p[i] = 1.f;
        p += 2 * Sx;
        if (lz > 1) taper_table(Sz, mz_, l, p, p + Sz, cz); else for (int i = 0; i < 2 * Sz; i++) p[i] = 1.f;
        p += 2 * Sz;
        taper_table(T, mt, l, p, p + T, ct);
        tap.ensure(th.size(), &c->dev_bytes);
        HIPCHECK(hipMemcpyAsync(tap.p, th.data(), th.size() * sizeof(float), hipMemcpyHostToDevice, c->stream));
        HIPCHECK(hipStreamSynchronize(c->stream));           // th leaves scope below

        const long long nin = F * Sx * Sz * T, nfine = F * Kx * Kz * H, nfull = F * Kx * Kz * T;
        XB.ensure((size_t)nin, &c->dev_bytes);
        XC.ensure((size_t)(nin * l), &c->dev_bytes);
        fB.ensure((size_t)nfine, &c->dev_bytes);
        fC.ensure((size_t)nfine, &c->dev_bytes);
        fD.ensure((size_t)nfine, &c->dev_bytes);
        mx.ensure((size_t)F, &c->dev_bytes);
        hipLaunchKernelGGL(load_kernel, dim3(nblocks_for(nin)), dim3(256), 0, c->stream, A, XB.p, XC.p, tap.p, Sx, Sz, T, l,
                           cx, cz, ct, nin);
        fft(XB.p, nin, T, 1, false);
        fft(XC.p, nin * l, l * T, 1, false);
        hipLaunchKernelGGL(spread_kernel, dim3(nblocks_for(nfine)), dim3(256), 0, c->stream, XB.p, XC.p, fB.p, fC.p, fD.p,
                           Sx, Sz, lx, lz, T, nfine);
        for (float2 *a : { fB.p, fC.p, fD.p }) {
            fft(a, nfine, Kz, H, false);
            fft(a, nfine, Kx, (long long)Kz * H, false);
        }
        hipLaunchKernelGGL(nyquist_max_kernel, dim3((unsigned)F), dim3(256), 0, c->stream, fD.p, mx.p, Kx * Kz, H);
        hipLaunchKernelGGL(operator_kernel, dim3(nblocks_for(nfine)), dim3(256), 0, c->stream, fB.p, fC.p, fD.p, mx.p,
                           (long long)Kx * Kz * H, (float)(lx * lz), (float)((long long)T * Kx * Kz), nfine);
        fft(fB.p, nfine, Kx, (long long)Kz * H, true);
        fft(fB.p, nfine, Kz, H, true);
        full.ensure((size_t)nfull, &c->dev_bytes);
        hipLaunchKernelGGL(hermitian_kernel, dim3(nblocks_for(nfull)), dim3(256), 0, c->stream, fB.p, full.p, T, nfull);
        fft(full.p, nfull, T, 1, true);
        hipLaunchKernelGGL(real_part_kernel, dim3(nblocks_for(nfull)), dim3(256), 0, c->stream, full.p, out, nfull);
    }
};

struct Dense {
    int NX, NZ, L;
    std::vector<float> G;
    std::vector<int> first, nsamp;
};

// Densify the database installed in c (whose host arrays are G/first/nsamp, L samples per row) by (nipx, nipz)
inline Dense densify(kiwi_hip_ctx *c, int nipx, int nipz, int L, const float *G, const int *first, const int *nsamp)
{
    const int nx = c->gm.nx, nz = c->gm.nz, ng = c->gm.ng;
    const Plan P = make_plan(nx, nz, ng, nipx, nipz, first, nsamp);
    Dense D;
    D.NX = P.NX; D.NZ = P.NZ;
    const size_t nrows = (size_t)P.NX * P.NZ * ng;
    D.first.assign(nrows, 0);
    D.nsamp.assign(nrows, 0);
    int lmax = 1;
    for (size_t i = 0; i < (size_t)nx * nz * ng; i++) lmax = std::max(lmax, nsamp[i]);
    for (const Block &b : P.blocks)
        for (const Write &w : b.writes) lmax = std::max(lmax, w.d1 - w.d0 + 1);
    D.L = lmax;
    auto drow = [&](int ixd, int izd, int ig) { return ((size_t)ixd * P.NZ + izd) * ng + ig; };
    for (const Block &b : P.blocks)
        for (const Write &w : b.writes)
            for (int ig = 0; ig < ng; ig++) { D.first[drow(w.ixd, w.izd, ig)] = w.d0; D.nsamp[drow(w.ixd, w.izd, ig)] = w.d1 - w.d0 + 1; }

    Work W{ c };
    DevBuf<float> dense, Abuf, Obuf, Hin, Hout, Vin, Mid;
    dense.alloc(nrows * (size_t)lmax, &c->dev_bytes);
    HIPCHECK(hipMemsetAsync(dense.p, 0, nrows * (size_t)lmax * sizeof(float), c->stream));
    const int Kx = P.bx, Kz = P.bz, Sx = P.Sx, Sz = P.Sz;
    // fields of equal window length are batched; the workspace of one field is about 12 complex fine fields
    std::map<int, std::vector<int>> by_T;
    for (int i = 0; i < (int)P.blocks.size(); i++)
        if (!P.blocks[i].writes.empty()) by_T[P.blocks[i].T].push_back(i);
    const size_t budget = std::max<size_t>(c->chunk_bytes_limit / 4, 1);
    for (auto &kv : by_T) {
        const int T = kv.first;
        const size_t per_field = (size_t)12 * Kx * Kz * T * sizeof(float2);
        const long long fmax = std::max<long long>(1, (long long)(budget / per_field));
        std::vector<std::pair<int, int>> fields;             // (block, component)
        for (int bi : kv.second) for (int ig = 0; ig < ng; ig++) fields.push_back({ bi, ig });
        for (size_t f0 = 0; f0 < fields.size(); f0 += (size_t)fmax) {
            const long long F = std::min<long long>(fmax, (long long)(fields.size() - f0));
            std::vector<int> fblk(F), fig(F), bnode, bw0, blist;
            std::map<int, int> local;
            for (long long f = 0; f < F; f++) {
                const int bi = fields[f0 + f].first;
                auto it = local.find(bi);
                if (it == local.end()) {
                    it = local.emplace(bi, (int)blist.size()).first;
                    blist.push_back(bi);
                    bnode.insert(bnode.end(), P.blocks[bi].node.begin(), P.blocks[bi].node.end());
                    bw0.push_back(P.blocks[bi].w0);
                }
                fblk[f] = it->second;
                fig[f] = fields[f0 + f].second;
            }
            DevBuf<int> fblk_d, fig_d, bnode_d, bw0_d;
            fblk_d.alloc(F, &c->dev_bytes); fig_d.alloc(F, &c->dev_bytes);
            bnode_d.alloc(bnode.size(), &c->dev_bytes); bw0_d.alloc(bw0.size(), &c->dev_bytes);
            HIPCHECK(hipMemcpyAsync(fblk_d.p, fblk.data(), F * sizeof(int), hipMemcpyHostToDevice, c->stream));
            HIPCHECK(hipMemcpyAsync(fig_d.p, fig.data(), F * sizeof(int), hipMemcpyHostToDevice, c->stream));
            HIPCHECK(hipMemcpyAsync(bnode_d.p, bnode.data(), bnode.size() * sizeof(int), hipMemcpyHostToDevice, c->stream));
            HIPCHECK(hipMemcpyAsync(bw0_d.p, bw0.data(), bw0.size() * sizeof(int), hipMemcpyHostToDevice, c->stream));
            const long long nA = F * Sx * Sz * T, nO = F * Kx * Kz * T;
            Abuf.ensure((size_t)nA, &c->dev_bytes);
            Obuf.ensure((size_t)nO, &c->dev_bytes);
            hipLaunchKernelGGL(gather_kernel, dim3(nblocks_for(nA)), dim3(256), 0, c->stream, Abuf.p, c->G.p, c->span.p,
                               c->gm.pitch, fblk_d.p, fig_d.p, bnode_d.p, bw0_d.p, ng, Sx, Sz, T, nA);
            const int ntm = P.blocks[blist[0]].ntmargin, mx = P.ox / 2, mz = P.oz / 2;
            // interpolate3d's dispatch (gfdb.f90:1267-1310)
            if (nipz == 1) W.pass(Abuf.p, Obuf.p, F, Sx, Sz, T, nipx, 1, mx, 0, ntm);
            else if (nipx == 1) W.pass(Abuf.p, Obuf.p, F, Sx, Sz, T, 1, nipz, 0, mz, ntm);
            else if (nipx == 4 && nipz == 4) {
                Mid.ensure((size_t)(F * 2 * Sx * 2 * Sz * T), &c->dev_bytes);
                W.pass(Abuf.p, Mid.p, F, Sx, Sz, T, 2, 2, mx / 2, mz / 2, ntm);
                W.pass(Mid.p, Obuf.p, F, 2 * Sx, 2 * Sz, T, 2, 2, mx, mz, ntm);
            } else if (nipx == nipz) W.pass(Abuf.p, Obuf.p, F, Sx, Sz, T, nipx, nipz, mx, mz, ntm);
            else {
                // horizontal pass per stored depth row, vertical pass per output column -- with the distance margin
                // (gfdb.f90:1306, imitated)
                Hin.ensure((size_t)nA, &c->dev_bytes);
                Hout.ensure((size_t)(F * Sz * Kx * T), &c->dev_bytes);
                Vin.ensure((size_t)(F * Kx * Sz * T), &c->dev_bytes);
                hipLaunchKernelGGL(hslice_kernel, dim3(nblocks_for(nA)), dim3(256), 0, c->stream, Abuf.p, Hin.p, Sx, Sz, T, nA);
                W.pass(Hin.p, Hout.p, F * Sz, Sx, 1, T, nipx, 1, mx, 0, ntm);
                const long long nV = F * Kx * Sz * T;
                hipLaunchKernelGGL(vselect_kernel, dim3(nblocks_for(nV)), dim3(256), 0, c->stream, Abuf.p, Hout.p, Vin.p, Sx,
                                   Sz, Kx, nipx, T, nV);
                W.pass(Vin.p, Obuf.p, F * Kx, 1, Sz, T, 1, nipz, 0, mx, ntm);
            }
            // write-back (gfdb.f90:1188-1226)
            std::vector<WriteRec> wr;
            for (long long f = 0; f < F; f++) {
                const Block &b = P.blocks[blist[fblk[f]]];
                for (const Write &w : b.writes)
                    wr.push_back(WriteRec{ ((f * Kx + w.lx) * Kz + w.lz) * (long long)T + (w.d0 - b.w0),
                                           (long long)drow(w.ixd, w.izd, fig[f]) * lmax, w.d1 - w.d0 + 1, 0 });
            }
            if (!wr.empty()) {
                DevBuf<WriteRec> wr_d;
                wr_d.alloc(wr.size(), &c->dev_bytes);
                HIPCHECK(hipMemcpyAsync(wr_d.p, wr.data(), wr.size() * sizeof(WriteRec), hipMemcpyHostToDevice, c->stream));
                hipLaunchKernelGGL(writeback_kernel, dim3((unsigned)wr.size()), dim3(256), 0, c->stream, Obuf.p, dense.p, wr_d.p);
                HIPCHECK(hipGetLastError());
                HIPCHECK(hipStreamSynchronize(c->stream));     // the small tables above leave scope
            }
            HIPCHECK(hipStreamSynchronize(c->stream));
        }
    }
    D.G.resize(nrows * (size_t)lmax);
    HIPCHECK(hipMemcpyAsync(D.G.data(), dense.p, D.G.size() * sizeof(float), hipMemcpyDeviceToHost, c->stream));
    HIPCHECK(hipStreamSynchronize(c->stream));
    // a non-finite interpolated sample (non-finite input) is refused rather than installed
    for (const Block &b : P.blocks)
        for (const Write &w : b.writes)
            for (int ig = 0; ig < ng; ig++) {
                const float *v = D.G.data() + drow(w.ixd, w.izd, ig) * lmax;
                for (int k = 0; k <= w.d1 - w.d0; k++)
                    if (!std::isfinite(v[k]))
                        throw std::runtime_error("set_database: the interpolation gave a non-finite sample at ix=" +
                                                 std::to_string(w.ixd + 1) + " iz=" + std::to_string(w.izd + 1) + " ig=" +
                                                 std::to_string(ig + 1) + " (non-finite input traces?)");
            }
    // stored traces stay bit-identical (gfdb.f90:1193-1194)
    for (int ix = 0; ix < nx; ix++)
        for (int iz = 0; iz < nz; iz++)
            for (int ig = 0; ig < ng; ig++) {
                const size_t s = ((size_t)ix * nz + iz) * ng + ig, d = drow(ix * nipx, iz * nipz, ig);
                D.first[d] = first[s];
                D.nsamp[d] = nsamp[s];
                std::memcpy(D.G.data() + d * lmax, G + s * (size_t)L, (size_t)std::max(0, nsamp[s]) * sizeof(float));
            }
    return D;
}

} // namespace gfk
