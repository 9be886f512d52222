// wave_exec.hpp -- runs the text of a HIP kernel on the host, one workgroup at a time: every lane of the workgroup in flight is
// a host thread (a pool of them, kept over the launches), the workgroups of a grid run one after the other.  What the lanes of
// a wavefront or of a workgroup do together -- shuffles, ballot, read-lane, the DPP moves of kiwi_common.hpp, __syncthreads --
// is a rendezvous: every lane that has not yet left the kernel must arrive with the SAME operation and the same count of
// operations behind it (the kernels call them in uniform control flow; the executor aborts with a message where they do not),
// then each takes what it needs from what the others brought.  A lane that has returned from the kernel no longer takes part,
// as on the device; what is read from it is 0.  Atomics are plain reads and writes under one lock.
//
// For sanitizer runs of kernel text (tests/host_kernels/linfit_path_host.cpp): the buffers a kernel gets are ordinary heap
// allocations of exactly the size the library asks of the device, so AddressSanitizer sees every index the text forms.
// Included by the hip/hip_runtime.h of this folder; nothing here knows the project's kernels.
#pragma once
#include <atomic>
#include <condition_variable>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <mutex>
#include <thread>
#include <vector>

#include <climits>
#include <linux/futex.h>
#include <sys/syscall.h>
#include <unistd.h>

struct dim3 {
    unsigned x, y, z;
    dim3(unsigned a = 1, unsigned b = 1, unsigned c = 1) : x(a), y(b), z(c) {}
};
inline thread_local dim3 threadIdx, blockIdx, blockDim, gridDim;

namespace hostexec {

constexpr int kWave = 64, kMaxThreads = 1024;

enum Op { OP_SYNCTHREADS = 1, OP_WAVE_BARRIER, OP_SHFL, OP_SHFL_DOWN, OP_SHFL_UP, OP_BALLOT, OP_READLANE, OP_READFIRSTLANE, OP_DPP };

// the lanes of one wavefront, or of the whole workgroup: who is still inside the kernel, who has arrived, what they brought
struct Rendezvous {
    std::mutex m;                           // arrivals and departures; the wait itself is on `gen` (a futex: no lock to queue for on the way out)
    int active = 0, arrived = 0;
    std::atomic<unsigned> gen{ 1 };         // the rendezvous in progress
    int op = 0;                             // ... and what the first lane to arrive came for
    unsigned long long seq = 0;
    uint64_t slot[2][kWave];                // by generation parity: a lane can be one rendezvous ahead of a reader, never two
    unsigned stamp[2][kWave];               // generation in which the slot was filled (0: never)
    void reset(int n)
    {
        active = n; arrived = 0; gen.store(1); op = 0; seq = 0;
        std::memset(stamp, 0, sizeof(stamp));
    }
};

struct Lane {
    int tid = 0, lane = 0, wave = 0;
    unsigned long long wave_seq = 0, group_seq = 0;
};
inline thread_local Lane me;

[[noreturn]] inline void divergence(const char *what, int op, int first_op, unsigned long long seq, unsigned long long first_seq)
{
    std::fprintf(stderr, "hostexec: %s in non-uniform control flow: thread %d arrives with operation %d (number %llu), another lane with %d (number %llu)\n",
                 what, me.tid, op, seq, first_op, first_seq);
    std::abort();
}

struct Executor {
    std::mutex atomics;                     // every atomic of a kernel
    Rendezvous group, waves[kMaxThreads / kWave];
    // the pool
    std::mutex m;
    std::condition_variable cv_job, cv_done;
    std::vector<std::thread> pool;
    unsigned long long job = 0;
    int job_threads = 0, done = 0;
    bool quit = false;
    const std::function<void()> *fn = nullptr;
    dim3 job_block, job_grid, job_dim;
    unsigned long long launches = 0, groups_run = 0;
    std::atomic<unsigned long long> rendezvous{ 0 };

    ~Executor()
    {
        { std::lock_guard<std::mutex> lk(m); quit = true; job++; }
        cv_job.notify_all();
        for (auto &t : pool) t.join();
    }

    // ---- rendezvous
    // returns the generation the lanes met in; `r.slot[gen & 1]` holds what they brought until the NEXT rendezvous completes
    unsigned meet(Rendezvous &r, int idx, int op, unsigned long long seq, uint64_t mine, const char *what)
    {
        unsigned g;
        bool last;
        {
            std::lock_guard<std::mutex> lk(r.m);
            g = r.gen.load(std::memory_order_relaxed);
            if (r.arrived == 0) { r.op = op; r.seq = seq; }
            else if (r.op != op || r.seq != seq) divergence(what, op, r.op, seq, r.seq);
            r.slot[g & 1][idx] = mine;
            r.stamp[g & 1][idx] = g;
            last = ++r.arrived == r.active;
            if (last) { r.arrived = 0; r.gen.store(g + 1, std::memory_order_release); rendezvous++; }
        }
        if (last) wake(r);
        else while (r.gen.load(std::memory_order_acquire) == g) syscall(SYS_futex, (unsigned *)&r.gen, FUTEX_WAIT_PRIVATE, g, nullptr, nullptr, 0);
        return g;
    }
    static void wake(Rendezvous &r) { syscall(SYS_futex, (unsigned *)&r.gen, FUTEX_WAKE_PRIVATE, INT_MAX, nullptr, nullptr, 0); }
    void leave(Rendezvous &r)
    {
        bool last;
        {
            std::lock_guard<std::mutex> lk(r.m);
            r.active--;
            last = r.active > 0 && r.arrived == r.active;
            if (last) { r.arrived = 0; r.gen.store(r.gen.load(std::memory_order_relaxed) + 1, std::memory_order_release); rendezvous++; }
        }
        if (last) wake(r);
    }
    // what lane `src` of my wavefront brought to generation g (0 and *had = false where it did not take part)
    uint64_t brought(unsigned g, int src, bool *had = nullptr)
    {
        Rendezvous &r = waves[me.wave];
        const bool ok = src >= 0 && src < kWave && r.stamp[g & 1][src] == g;
        if (had) *had = ok;
        return ok ? r.slot[g & 1][src] : 0;
    }
    unsigned wave_meet(int op, uint64_t mine, const char *what) { return meet(waves[me.wave], me.lane, op, ++me.wave_seq, mine, what); }
    void syncthreads() { meet(group, 0, OP_SYNCTHREADS, ++me.group_seq, 0, "__syncthreads"); }

    // ---- launches
    void worker(int index)
    {
        unsigned long long seen = 0;
        for (;;) {
            const std::function<void()> *f;
            {
                std::unique_lock<std::mutex> lk(m);
                cv_job.wait(lk, [&] { return job != seen; });
                seen = job;
                if (quit) return;
                if (index >= job_threads) continue;
                f = fn;
                threadIdx = dim3((unsigned)index % job_dim.x, ((unsigned)index / job_dim.x) % job_dim.y, (unsigned)index / (job_dim.x * job_dim.y));
                blockIdx = job_block; blockDim = job_dim; gridDim = job_grid;
            }
            me = Lane{ index, index % kWave, index / kWave, 0, 0 };
            (*f)();
            leave(waves[me.wave]);
            leave(group);
            {
                std::lock_guard<std::mutex> lk(m);
                if (++done == job_threads) cv_done.notify_one();
            }
        }
    }

    // kernel(args...) over the grid: the workgroups in the device's order (x fastest), each to its end before the next starts
    template <class F> void launch(dim3 grid, dim3 block, F &&kernel)
    {
        const int n = (int)(block.x * block.y * block.z);
        if (n < 1 || n > kMaxThreads) { std::fprintf(stderr, "hostexec: workgroup of %d threads\n", n); std::abort(); }
        while ((int)pool.size() < n) { const int i = (int)pool.size(); pool.emplace_back([this, i] { worker(i); }); }
        const std::function<void()> f = kernel;
        launches++;
        for (unsigned z = 0; z < grid.z; z++)
            for (unsigned y = 0; y < grid.y; y++)
                for (unsigned x = 0; x < grid.x; x++) {
                    group.reset(n);
                    for (int w = 0; w * kWave < n; w++) waves[w].reset(std::min(kWave, n - w * kWave));
                    {
                        std::lock_guard<std::mutex> lk(m);
                        fn = &f; job_threads = n; done = 0; job_block = dim3(x, y, z); job_grid = grid; job_dim = block;
                        job++;
                    }
                    cv_job.notify_all();
                    std::unique_lock<std::mutex> lk(m);
                    cv_done.wait(lk, [&] { return done == n; });
                    groups_run++;
                }
    }
};

inline Executor &exec()
{
    static Executor e;
    return e;
}

template <class T> inline uint64_t bits_of(T v)
{
    static_assert(sizeof(T) <= 8, "cross-lane operations move at most 64 bits");
    uint64_t b = 0;
    std::memcpy(&b, &v, sizeof(T));
    return b;
}
template <class T> inline T from_bits(uint64_t b)
{
    T v;
    std::memcpy(&v, &b, sizeof(T));
    return v;
}

} // namespace hostexec

// ------------------------------------------------------------------------------------------------ what the kernels call
inline void __syncthreads() { hostexec::exec().syncthreads(); }
inline void __builtin_amdgcn_wave_barrier() { hostexec::exec().wave_meet(hostexec::OP_WAVE_BARRIER, 0, "wave_barrier"); }
inline void __builtin_amdgcn_fence(int, const char *) {}       // (every rendezvous goes through a lock: nothing to order)

// width 64 only: the kernels name it
template <class T> inline T __shfl(T v, int src, int width = 64)
{
    (void)width;
    auto &e = hostexec::exec();
    const unsigned g = e.wave_meet(hostexec::OP_SHFL, hostexec::bits_of(v), "__shfl");
    return hostexec::from_bits<T>(e.brought(g, src & 63));
}
template <class T> inline T __shfl_down(T v, int off, int width = 64)
{
    (void)width;
    auto &e = hostexec::exec();
    const unsigned g = e.wave_meet(hostexec::OP_SHFL_DOWN, hostexec::bits_of(v), "__shfl_down");
    const int src = hostexec::me.lane + off;
    return src < 64 ? hostexec::from_bits<T>(e.brought(g, src)) : v;      // (past the end of the wave: the lane's own value)
}
template <class T> inline T __shfl_up(T v, int off, int width = 64)
{
    (void)width;
    auto &e = hostexec::exec();
    const unsigned g = e.wave_meet(hostexec::OP_SHFL_UP, hostexec::bits_of(v), "__shfl_up");
    const int src = hostexec::me.lane - off;
    return src >= 0 ? hostexec::from_bits<T>(e.brought(g, src)) : v;
}
inline unsigned long long __builtin_amdgcn_ballot_w64(bool p)
{
    auto &e = hostexec::exec();
    const unsigned g = e.wave_meet(hostexec::OP_BALLOT, p ? 1 : 0, "ballot");
    unsigned long long b = 0;
    for (int l = 0; l < 64; l++) if (e.brought(g, l)) b |= 1ull << l;
    return b;
}
inline int __builtin_amdgcn_readlane(int v, int lane)
{
    auto &e = hostexec::exec();
    const unsigned g = e.wave_meet(hostexec::OP_READLANE, hostexec::bits_of(v), "readlane");
    return hostexec::from_bits<int>(e.brought(g, lane & 63));
}
inline int __builtin_amdgcn_readfirstlane(int v)
{
    auto &e = hostexec::exec();
    const unsigned g = e.wave_meet(hostexec::OP_READFIRSTLANE, hostexec::bits_of(v), "readfirstlane");
    for (int l = 0; l < 64; l++) {
        bool had;
        const uint64_t b = e.brought(g, l, &had);
        if (had) return hostexec::from_bits<int>(b);
    }
    return v;
}
// the forms kiwi_common.hpp uses (wave_reduce_f64): row_shr:1 .. 15 (0x111 .. 0x11f), row_bcast:15 (0x142), row_bcast:31 (0x143),
// all banks, bound_ctrl.  A lane whose row the mask leaves out, or whose source lies outside its row, gets `old` (bound_ctrl: 0
// for the shifts)
inline int __builtin_amdgcn_update_dpp(int old, int src, int ctrl, int row_mask, int bank_mask, bool bound_ctrl)
{
    auto &e = hostexec::exec();
    const unsigned g = e.wave_meet(hostexec::OP_DPP, hostexec::bits_of(src), "update_dpp");
    const int lane = hostexec::me.lane, row = lane >> 4;
    if (bank_mask != 0xf) { std::fprintf(stderr, "hostexec: update_dpp with bank mask %#x\n", bank_mask); std::abort(); }
    if (!((row_mask >> row) & 1)) return old;
    if (ctrl >= 0x111 && ctrl <= 0x11f) {
        const int n = ctrl & 15;
        if ((lane & 15) < n) return bound_ctrl ? 0 : old;
        return hostexec::from_bits<int>(e.brought(g, lane - n));
    }
    if (ctrl == 0x142) return row >= 1 ? hostexec::from_bits<int>(e.brought(g, 16 * row - 1)) : old;
    if (ctrl == 0x143) return row >= 2 ? hostexec::from_bits<int>(e.brought(g, 31)) : old;
    std::fprintf(stderr, "hostexec: update_dpp control %#x is not one of the forms provided\n", ctrl);
    std::abort();
}

inline int atomicOr(int *p, int v) { std::lock_guard<std::mutex> lk(hostexec::exec().atomics); const int o = *p; *p = o | v; return o; }
inline int atomicMin(int *p, int v) { std::lock_guard<std::mutex> lk(hostexec::exec().atomics); const int o = *p; *p = o < v ? o : v; return o; }
inline int atomicMax(int *p, int v) { std::lock_guard<std::mutex> lk(hostexec::exec().atomics); const int o = *p; *p = o > v ? o : v; return o; }
inline int atomicAdd(int *p, int v) { std::lock_guard<std::mutex> lk(hostexec::exec().atomics); const int o = *p; *p = o + v; return o; }
inline unsigned atomicAdd(unsigned *p, unsigned v) { std::lock_guard<std::mutex> lk(hostexec::exec().atomics); const unsigned o = *p; *p = o + v; return o; }
