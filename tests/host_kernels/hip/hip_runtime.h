// <hip/hip_runtime.h> for a HOST build of the kernels' text (tests/host_kernels): found in front of ROCm's through
// -I tests/host_kernels, so that kiwi_common.hpp and what includes it compile unchanged with a plain C++ compiler.  The
// qualifiers are empty, `__shared__` is storage shared by the lanes of the ONE workgroup in flight (wave_exec.hpp runs them
// one after the other), the vector types are plain structs, the intrinsics are the handful the plain-C++ kernels use
// (kiwi_geometry.hpp, kiwi_misfit.hpp, kiwi_linfit.hpp; kiwi_accum.inc with its assembly statements is not for this).
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>

#define __global__
#define __device__
#define __host__
#define __forceinline__ inline
#define __launch_bounds__(...)
#define __shared__ static
// dynamic shared memory (kiwi_misfit.hpp KIWI_DYNAMIC_SHARED): `extern` and `static` exclude each other, so the in-LDS transform
// kernels, which nothing here launches, get a fixed array of the largest size the library asks for (4 << kFusedFftMaxLog2 bytes)
#define KIWI_DYNAMIC_SHARED(T, name) static __attribute__((aligned(16))) T name[(4 << 14) / sizeof(T)]

#include "../wave_exec.hpp"

struct int2 { int x, y; };
struct alignas(16) int4 { int x, y, z, w; };
struct float2 { float x, y; };
struct alignas(16) float4 { float x, y, z, w; };
inline int2 make_int2(int a, int b) { return { a, b }; }
inline int4 make_int4(int a, int b, int c, int d) { return { a, b, c, d }; }
inline float2 make_float2(float a, float b) { return { a, b }; }
inline float4 make_float4(float a, float b, float c, float d) { return { a, b, c, d }; }

using std::max;
using std::min;

typedef void *hipStream_t;
typedef void *hipEvent_t;

inline int __popcll(unsigned long long v) { return __builtin_popcountll(v); }
inline int __clz(int v) { return v == 0 ? 32 : __builtin_clz((unsigned)v); }
inline unsigned __brev(unsigned v)
{
    unsigned r = 0;
    for (int i = 0; i < 32; i++) r |= ((v >> i) & 1u) << (31 - i);
    return r;
}
inline double __longlong_as_double(long long v) { double d; std::memcpy(&d, &v, 8); return d; }
inline float __int_as_float(int v) { float f; std::memcpy(&f, &v, 4); return f; }
inline int __float_as_int(float f) { int v; std::memcpy(&v, &f, 4); return v; }
inline int __double2loint(double d) { long long v; std::memcpy(&v, &d, 8); return (int)(unsigned)(v & 0xffffffffll); }
inline int __double2hiint(double d) { long long v; std::memcpy(&v, &d, 8); return (int)(unsigned)((unsigned long long)v >> 32); }
inline double __hiloint2double(int hi, int lo)
{
    const unsigned long long v = ((unsigned long long)(unsigned)hi << 32) | (unsigned)lo;
    double d;
    std::memcpy(&d, &v, 8);
    return d;
}
inline int __builtin_amdgcn_frexp_expf(float v) { int e = 0; if (v != 0.f && std::isfinite(v)) (void)std::frexp(v, &e); return e; }
inline float __builtin_amdgcn_sqrtf(float v) { return std::sqrt(v); }
