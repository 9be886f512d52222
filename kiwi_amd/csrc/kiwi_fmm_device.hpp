// kiwi_fmm_device.hpp -- batches of independent fast-marching solves on the device, ONE SOLVE PER WAVEFRONT, each of them the
// reference's sequential march: fast_marching_plain (kiwi_host_fmm.hpp; eikonal.f90:29-199 with heap.f90's index heap) statement
// by statement in what decides the result -- every comparison of heap keys, every swap of heap entries (the order among equal
// keys), update_neighbor with every fp32 operation rounded on its own (this file is part of kiwi_hip.o: -ffp-contract=off, IEEE
// division and square root, denormals kept), min / max as std::min / std::max behave, and the `discard` rule.
//
// Layout.  The march is a chain of dependent loads; what hides it is the number of solves in flight, nothing inside one solve:
//   * the heap (the front only: 537-1005 entries measured on cfg4's 1200 x 360 grid) lives in LDS, kHeapCap entries of 8 bytes = 32 KB per
//     solve, so five solves share a CU; a solve that outgrows it ends with status 1, never writes past it, and is solved again by
//     the host's routine (counted);
//   * node times and back pointers are one 8-byte record per node in a global workspace sized by the batch;
//   * lane 0 keeps the heap.  The four neighbours of an accepted node read disjoint sets of times, so lanes 0..3 take one each:
//     their records are fetched behind ONE global round trip, their neighbours' times and speeds behind a second one, the four
//     times computed side by side, and only then the heap operations done on lane 0 in the reference's order (left, right, up,
//     down).  The back pointers of the four nodes are tracked in registers while the heap moves entries, so no third round trip
//     is needed to find an entry whose key changed;
//   * the 64 lanes together fill the workspace, count the nodes the march has to accept, and copy the times out.
// Every loop is bounded by the input's size: at most nx*ny pops, sifts by the heap's depth; no atomics, no waiting on other solves.
#pragma once
#include <hip/hip_runtime.h>

namespace kiwi {
namespace fmmdev {

constexpr int kHeapCap = 4096;                    // heap entries per solve in LDS
constexpr int kFarAway = -1, kAlive = 0;          // back-pointer states of eikonal.f90 (positions are >= 1)

struct Solve {
    long long ofs;            // of its speeds, node records and times inside the launch's buffers
    int nx, ny, ix, iy;       // grid, start cell (1-based, clamped: computed by the host exactly as fast_marching_plain does)
    float dx, dy, discard;
    int pad;
};
struct Node { float t; int bp; };
struct Entry { float key; int idx; };

__device__ __forceinline__ float hmin(float a, float b) { return (b < a) ? b : a; }      // std::min
__device__ __forceinline__ float hmax(float a, float b) { return (a < b) ? b : a; }      // std::max

__global__ __launch_bounds__(64) void fmm_batch_kernel(const Solve *__restrict__ solves, const float *__restrict__ speed_all,
                                                       Node *__restrict__ nodes_all, float *__restrict__ times_all,
                                                       int *__restrict__ status, int *__restrict__ hiwater_out)
{
    __shared__ Entry h[kHeapCap];                 // heap position p (1-based) at h[p - 1]
    const Solve sv = solves[blockIdx.x];
    const int lane = threadIdx.x;
    const int nx = sv.nx, ny = sv.ny;
    const int nn = nx * ny;
    const float *__restrict__ speed = speed_all + sv.ofs;
    Node *nodes = nodes_all + sv.ofs;
    float *__restrict__ times = times_all + sv.ofs;
    const float inf = 3.4028234663852886e+38f * 0.1f;
    const float dx = sv.dx, dy = sv.dy, discard = sv.discard;

    int cnt = 0;
    for (int k = lane; k < nn; k += 64) {
        nodes[k] = Node{ inf, kFarAway };
        cnt += speed[k] != discard;
    }
    for (int m = 32; m >= 1; m >>= 1) cnt += __shfl_xor(cnt, m);
    __syncthreads();

    // heap state: lane 0's copy is the one that counts
    int n = 0, hiwater = 0, st = 0;
    int ti[4] = { 0, 0, 0, 0 }, tbp[4] = { 0, 0, 0, 0 };      // the four neighbours being updated and where their entries are
    auto place = [&](int pos, Entry e) {
        h[pos - 1] = e;
        nodes[e.idx - 1].bp = pos;
#pragma unroll
        for (int k = 0; k < 4; k++) if (ti[k] == e.idx) tbp[k] = pos;
    };
    auto up = [&](int v) {                                      // upheap, heap.f90:205-229
        const Entry e = h[v - 1];
        while (v > 1) {
            const int u = (v - 2) / 2 + 1;
            const Entry p = h[u - 1];
            if (p.key <= e.key) break;
            place(v, p);
            v = u;
        }
        place(v, e);
    };
    auto down = [&](int v) {                                    // downheap, heap.f90:172-203
        const Entry e = h[v - 1];
        int w = 2 * (v - 1) + 2;
        while (w <= n) {
            Entry c = h[w - 1];
            if (w + 1 <= n) { const Entry c1 = h[w]; if (c1.key < c.key) { c = c1; w++; } }
            if (e.key <= c.key) break;
            place(v, c);
            v = w;
            w = 2 * (v - 1) + 2;
        }
        place(v, e);
    };
    auto push = [&](int idx, float key) -> bool {               // pushheap, heap.f90:76-101
        if (n >= kHeapCap) { st = 1; return false; }
        n++;
        hiwater = n > hiwater ? n : hiwater;
        place(n, Entry{ key, idx });
        up(n);
        return true;
    };

    const int i0 = (sv.iy - 1) * nx + sv.ix;
    if (!(nx == 1 && ny == 1)) {
        int wanted = cnt;                                        // (every lane holds the count)
        if (speed[i0 - 1] != discard) wanted--;
        if (lane == 0) {
            const int ix = sv.ix, iy = sv.iy;
            nodes[i0 - 1] = Node{ 0.f, kAlive };
            const bool l = 1 < ix, r = ix < nx, u = 1 < iy, d = iy < ny;
            float tl = 0.f, tr = 0.f, tu = 0.f, td = 0.f;
            if (l) { tl = dx / speed[i0 - 2]; nodes[i0 - 2].t = tl; }                  // eikonal.f90:92-95
            if (r) { tr = dx / speed[i0]; nodes[i0].t = tr; }
            if (u) { tu = dy / speed[i0 - 1 - nx]; nodes[i0 - 1 - nx].t = tu; }
            if (d) { td = dy / speed[i0 - 1 + nx]; nodes[i0 - 1 + nx].t = td; }
            if (l) push(i0 - 1, tl);                                                 // :97-100 (four entries: always room)
            if (r) push(i0 + 1, tr);
            if (u) push(i0 - nx, tu);
            if (d) push(i0 + nx, td);
        }
        const float dx2 = dx * dx, dy2 = dy * dy, dxy2 = dx2 * dy2, dsum = dx2 + dy2;
        // at most nn pops (`nalive <= nx*ny`, eikonal.f90:104)
        for (int nalive = 1; nalive <= nn; nalive++) {
            int imin = 0;
            if (lane == 0 && n > 0) {                            // popheap, heap.f90:103-131
                const Entry top = h[0];
                h[0] = h[n - 1];
                nodes[top.idx - 1].bp = kAlive;                  // (the reference writes 0 in popheap and ALIVE = 0 right after)
                n--;
                if (n >= 1) down(1);
                imin = top.idx;
            }
            // lane 0's stores become visible to the lanes that read the records below (one wavefront: program order)
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            imin = __builtin_amdgcn_readfirstlane(imin);
            if (imin == 0) break;
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
            const int ix = (imin - 1) % nx + 1, iy = (imin - 1) / nx + 1;
            // update_neighbor :121-186 of the four neighbours, one per lane 0..3 (left, right, up, down); they read disjoint
            // sets of times.  First round trip: the neighbour's record (and the speed that decides whether the march ends here)
            const int k4 = lane & 3;
            const int x = ix + (k4 == 0 ? -1 : (k4 == 1 ? 1 : 0)), y = iy + (k4 == 2 ? -1 : (k4 == 3 ? 1 : 0));
            const bool valid = lane < 4 && x >= 1 && x <= nx && y >= 1 && y <= ny;
            const int ni = valid ? (y - 1) * nx + x : imin;
            const float spmin = speed[imin - 1];
            const Node nd = nodes[ni - 1];
            if (spmin != discard && --wanted == 0) break;
            // second round trip: the times around it and its speed
            const bool act = valid && nd.bp != kAlive;
            const bool ha = act && 1 < x, hb = act && x < nx, hc = act && 1 < y, hd = act && y < ny;
            const float va = nodes[(ha ? ni - 1 : ni) - 1].t, vb = nodes[(hb ? ni + 1 : ni) - 1].t;
            const float vc = nodes[(hc ? ni - nx : ni) - 1].t, vd = nodes[(hd ? ni + nx : ni) - 1].t;
            const float s_ = speed[ni - 1];
            const float A = ha ? va : inf, B = hb ? vb : inf, C = hc ? vc : inf, D = hd ? vd : inf;
            const float hx = dx / s_, hy = dy / s_;            // (the reference divides anew at every use: same operands, same quotient)
            float t = 0.f;
            const float aa = hmin(A, B), cc = hmin(C, D);
            if (hmax(aa, cc) != inf) {
                const float q = (aa - cc) * s_;
                const float s = dxy2 * (dsum - q * q);
                if (s >= 0.f) t = hmax(t, ((aa * dy2 + cc * dx2) * s_ + sqrtf(s)) / (s_ * dsum));
            }
            if (cc == inf) {
                if (A < inf) t = hmax(t, A + hx);
                if (B < inf) t = hmax(t, B + hx);
            }
            if (aa == inf) {
                if (C < inf) t = hmax(t, C + hy);
                if (D < inf) t = hmax(t, D + hy);
            }
            if (t == 0.f) {
                t = inf;
                if (A < inf) t = hmin(t, A + hx);
                if (B < inf) t = hmin(t, B + hx);
                if (C < inf) t = hmin(t, C + hy);
                if (D < inf) t = hmin(t, D + hy);
            }
            // the heap operations on lane 0, in the reference's order
            int act4[4], ni4[4], bp4[4];
            float told4[4], t4[4];
#pragma unroll
            for (int k = 0; k < 4; k++) {
                act4[k] = __builtin_amdgcn_readlane((int)act, k);
                ni4[k] = __builtin_amdgcn_readlane(ni, k);
                bp4[k] = __builtin_amdgcn_readlane(nd.bp, k);
                told4[k] = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(nd.t), k));
                t4[k] = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(t), k));
            }
            if (lane == 0) {
#pragma unroll
                for (int k = 0; k < 4; k++) { ti[k] = act4[k] ? ni4[k] : 0; tbp[k] = bp4[k]; }
#pragma unroll
                for (int k = 0; k < 4; k++) {
                    if (!act4[k] || st != 0) continue;
                    const float told = told4[k], tk = t4[k];
                    if (bp4[k] == kFarAway && !push(ni4[k], told)) break;
                    if (tk != 0.f && told != tk) {                   // updateheap, heap.f90:133-156
                        nodes[ni4[k] - 1].t = tk;
                        h[tbp[k] - 1].key = tk;
                        if (tk < told) up(tbp[k]);
                        if (tk > told) down(tbp[k]);
                    }
                }
            }
            if (__builtin_amdgcn_readfirstlane(st) != 0) break;
        }
    } else if (lane == 0) nodes[i0 - 1].t = 0.f;
    if (lane == 0) {
        status[blockIdx.x] = st;
        hiwater_out[blockIdx.x] = hiwater;
    }
    __syncthreads();
    for (int k = lane; k < nn; k += 64) times[k] = nodes[k].t;
}

} // namespace fmmdev
} // namespace kiwi
