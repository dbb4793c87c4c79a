// Shared helpers for libclasspose_hip (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include "../../include/classpose_hip.h"

extern thread_local char cpx_err_buf[256];

#define CPX_CHECK_LAUNCH()                                                        \
    do {                                                                          \
        hipError_t e__ = hipGetLastError();                                       \
        if (e__ != hipSuccess) {                                                  \
            snprintf(cpx_err_buf, sizeof(cpx_err_buf), "%s:%d: %s", __FILE__,     \
                     __LINE__, hipGetErrorString(e__));                           \
            return CPX_EHIP;                                                      \
        }                                                                         \
    } while (0)

#define CPX_HIP(call)                                                             \
    do {                                                                          \
        hipError_t e__ = (call);                                                  \
        if (e__ != hipSuccess) {                                                  \
            snprintf(cpx_err_buf, sizeof(cpx_err_buf), "%s:%d: %s", __FILE__,     \
                     __LINE__, hipGetErrorString(e__));                           \
            return CPX_EHIP;                                                      \
        }                                                                         \
    } while (0)

#define CPX_REQUIRE(cond)                                                         \
    do {                                                                          \
        if (!(cond)) {                                                            \
            snprintf(cpx_err_buf, sizeof(cpx_err_buf), "%s:%d: invalid argument: %s", \
                     __FILE__, __LINE__, #cond);                                  \
            return CPX_EINVAL;                                                    \
        }                                                                         \
    } while (0)

// A/B, ablation and diagnostic switches (include/classpose_hip_debug.h) exist only in the debug build
// (-DCPX_DEBUG -> libclasspose_hip_debug.so, what tools/*.py and the variant tests load).  In the product library
// each switch is a compile-time constant at its production value: no setter is exported, no non-production kernel
// is instantiated, and there is no mutable process-global state that could alter results.
#ifdef CPX_DEBUG
#define CPX_SWITCH(name, value) static int name = (value)
#else
#define CPX_SWITCH(name, value) [[maybe_unused]] static constexpr int name = (value)
#endif

static inline size_t cpx_align_up(size_t x, size_t a) { return (x + a - 1) / a * a; }
static inline int cpx_cdiv(long long a, long long b) { return (int)((a + b - 1) / b); }
// every workspace layout: consecutive requests at 256-byte boundaries; take() returns the request's offset, o ends as the total
struct CpxArena { size_t o = 0; size_t take(size_t bytes) { const size_t r = o; o = cpx_align_up(o + bytes, 256); return r; } };

// bf16 helpers (round-to-nearest-even, NaN preserved via the compiler's cast)
typedef __bf16 bf16_t;
__device__ __forceinline__ float bf16_to_f32(unsigned short u) {
    return __uint_as_float(((unsigned int)u) << 16);
}
__device__ __forceinline__ unsigned short f32_to_bf16(float f) {
    bf16_t b = (bf16_t)f;
    return *reinterpret_cast<unsigned short *>(&b);
}

// inclusive sum over a workgroup of 256 threads, every thread calling; *total = the sum of all 256 values.  s_w: 4 ints of LDS.
__device__ __forceinline__ int cpx_block_scan256(int v, int *s_w, int *total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int incl = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int up = __shfl_up(incl, o);
        if (lane >= o) incl += up;
    }
    if (lane == 63) s_w[wave] = incl;
    __syncthreads();
    int off = 0, tot = 0;
#pragma unroll
    for (int w = 0; w < 4; ++w) {
        if (w < wave) off += s_w[w];
        tot += s_w[w];
    }
    __syncthreads();
    *total = tot;
    return incl + off;
}
