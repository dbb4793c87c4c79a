// eval(diameter=): the output side of the 30 / diameter rescale on gfx950.
//   cpx_resize_linear_f32  cv2.resize(..., INTER_LINEAR) on the float32 planes of dP / cellprob / y_class
//   cpx_resize_nearest     cv2.resize(..., INTER_NEAREST) on the uint16 id maps and uint8 class maps
// Arithmetic follows tests/resize_reference.py (numpy float32, one rounding per product and per sum); built with
// -ffp-contract=off, so no expression below may fuse into an FMA.
#include "cpx_common.h"

#define NTHR 256
#define XPL 4          // destination elements per lane
typedef float v4f __attribute__((ext_vector_type(4)));
#define PPT 8          // planes per lane: taps, weights and the 16 source offsets are computed once and reused for every plane

// cv::resize's source coordinate of destination index d: float32 of the double (d + 0.5) * scale - 0.5, split into
// floor and fraction.  Horizontally the fraction is zeroed where the tap pair leaves the row (xmin / xmax handling of
// resizeGeneric_); vertically only the two row indices are clipped and the weight stays what it is.
__device__ __forceinline__ void lin_tap(int d, double scale, int slen, bool clamp_weight, int &s0, int &s1, float &f) {
    f = (float)(((double)d + 0.5) * scale - 0.5);
    int s = (int)floorf(f);
    f -= (float)s;
    if (clamp_weight) {
        if (s < 0) { f = 0.f; s = 0; }
        if (s >= slen - 1) { f = 0.f; s = slen - 1; }
    }
    s0 = min(max(s, 0), slen - 1);
    s1 = min(max(s + 1, 0), slen - 1);
}

// Bilinear.  A workgroup covers NTHR consecutive destination x of XPL consecutive destination rows, lane t taking column t of
// each row: the 64 lanes of a wave take 64 consecutive destination x, so every store instruction writes 256 contiguous bytes and
// every load instruction reads one short contiguous run of a source row, and the XPL rows of a lane share most of their source
// rows in the cache.  The lane then walks the planes blockIdx.y, blockIdx.y + gridDim.y, ... with the same taps: per plane only
// the 16 loads at precomputed 32-bit byte offsets, the 36 float operations and the 4 stores remain.  The stores are
// non-temporal: the destination is far larger than the caches and is not read again by this kernel, and keeping it out of
// them leaves the source rows there.  Measured at 104 planes 683^2 -> 1024^2 (tools/bench_resize_fields.py has the end-to-end
// figures): four CONSECUTIVE x per lane with one 16-byte store 400 us (the taps of neighbouring lanes lie 4 * scale elements apart
// and every load instruction touches three times as many cache lines); lane-consecutive x with elements NTHR apart in one
// row 228 us; this layout 184 us, and 114 us with the non-temporal stores.  Downscaling (1536^2 -> 1024^2) is bound by the
// source reads and took 345 - 355 us in every layout.
__global__ __launch_bounds__(NTHR) void k_resize_linear_f32(const float *__restrict__ src, int n_planes, int sh, int sw,
                                                            float *__restrict__ dst, int dh, int dw, int nbx, double scale_x,
                                                            double scale_y) {
    const int by = blockIdx.x / nbx, bx = blockIdx.x - by * nbx;
    const int x = bx * NTHR + threadIdx.x, y = by * XPL;
    const int ny = x < dw ? min(XPL, dh - y) : 0;          // rows this lane stores (lanes right of the image compute the last column's taps and store nothing)
    uint32_t o00[XPL], o01[XPL], o10[XPL], o11[XPL];       // byte offsets of the four taps inside a plane (sh * sw < 2^30)
    float fx, gx, fy[XPL], gy[XPL];
    int x0, x1;
    lin_tap(min(x, dw - 1), scale_x, sw, true, x0, x1, fx);
    gx = 1.f - fx;
#pragma unroll
    for (int k = 0; k < XPL; ++k) {
        int y0, y1;
        lin_tap(min(y + k, dh - 1), scale_y, sh, false, y0, y1, fy[k]);
        gy[k] = 1.f - fy[k];
        o00[k] = (uint32_t)(y0 * sw + x0) * 4u, o01[k] = (uint32_t)(y0 * sw + x1) * 4u;
        o10[k] = (uint32_t)(y1 * sw + x0) * 4u, o11[k] = (uint32_t)(y1 * sw + x1) * 4u;
    }
    for (int p = blockIdx.y; p < n_planes; p += gridDim.y) {
        const char *b = reinterpret_cast<const char *>(src + (size_t)p * sh * sw);
        float *o = dst + ((size_t)p * dh + y) * dw + x;
#pragma unroll
        for (int k = 0; k < XPL; ++k) {
            const float s00 = *reinterpret_cast<const float *>(b + o00[k]), s01 = *reinterpret_cast<const float *>(b + o01[k]);
            const float s10 = *reinterpret_cast<const float *>(b + o10[k]), s11 = *reinterpret_cast<const float *>(b + o11[k]);
            const float h0 = s00 * gx + s01 * fx;                        // horizontal pass of both rows,
            const float h1 = s10 * gx + s11 * fx;
            const float v = h0 * gy[k] + h1 * fy[k];                     // then the vertical one
            if (k < ny) __builtin_nontemporal_store(v, o + (size_t)k * dw);
        }
    }
}

// Exact 2 x 2 decimation.  One lane = XPL consecutive destination x of one destination row = 2 * XPL consecutive source x of
// two source rows; consecutive lanes take consecutive groups, so a wave reads two contiguous runs and stores one.
// VEC: dw % 4 == 0 and both bases 16-byte aligned (host-checked): 16-byte loads and stores.
template <bool VEC>
__global__ __launch_bounds__(NTHR) void k_resize_area_f32(const float *__restrict__ src, int n_planes, int sh, int sw,
                                                          float *__restrict__ dst, int dh, int dw, int ngx) {
    const int item = blockIdx.x * NTHR + threadIdx.x;
    if (item >= dh * ngx) return;
    const int y = item / ngx, x = (item - y * ngx) * XPL;
    const int nx = min(XPL, dw - x);
    for (int p = blockIdx.y; p < n_planes; p += gridDim.y) {
        const float *r0 = src + ((size_t)p * sh + 2 * y) * sw + 2 * x, *r1 = r0 + sw;
        float *o = dst + ((size_t)p * dh + y) * dw + x;
        if (VEC) {          // sw = 2 dw is a multiple of 8: both rows start 16-byte aligned
            const float4 a0 = *reinterpret_cast<const float4 *>(r0), a1 = *reinterpret_cast<const float4 *>(r0 + 4);
            const float4 b0 = *reinterpret_cast<const float4 *>(r1), b1 = *reinterpret_cast<const float4 *>(r1 + 4);
            const v4f v = {((a0.x + a0.y) + (b0.x + b0.y)) * 0.25f, ((a0.z + a0.w) + (b0.z + b0.w)) * 0.25f,
                           ((a1.x + a1.y) + (b1.x + b1.y)) * 0.25f, ((a1.z + a1.w) + (b1.z + b1.w)) * 0.25f};
            __builtin_nontemporal_store(v, reinterpret_cast<v4f *>(o));
        } else {
#pragma unroll
            for (int k = 0; k < XPL; ++k)
                if (k < nx) __builtin_nontemporal_store(((r0[2 * k] + r0[2 * k + 1]) + (r1[2 * k] + r1[2 * k + 1])) * 0.25f, o + k);
        }
    }
}

extern "C" int cpx_resize_linear_f32(const float *src, int n_planes, int sh, int sw, float *dst, int dh, int dw, void *stream) {
    CPX_REQUIRE(src && dst && n_planes > 0 && sh > 0 && sw > 0 && dh > 0 && dw > 0);
    CPX_REQUIRE((long long)dh * dw < (1ll << 31) && (long long)(dh + XPL) * (dw + NTHR) < (1ll << 31) && (long long)sh * sw < (1ll << 30));
    hipStream_t s = (hipStream_t)stream;
    if (sh == dh && sw == dw) {
        CPX_HIP(hipMemcpyAsync(dst, src, (size_t)n_planes * sh * sw * sizeof(float), hipMemcpyDeviceToDevice, s));
        return CPX_OK;
    }
    // cv::resize: inv_scale = dsize / ssize in double, scale = 1 / inv_scale
    const double scale_x = 1.0 / ((double)dw / (double)sw), scale_y = 1.0 / ((double)dh / (double)sh);
    const int gy = min(cpx_cdiv(n_planes, PPT), 65535);
    if (sw == 2 * dw && sh == 2 * dh) {
        const bool vec = dw % XPL == 0 && ((uintptr_t)src | (uintptr_t)dst) % 16 == 0;
        const int ngx = cpx_cdiv(dw, XPL);
        hipLaunchKernelGGL(vec ? k_resize_area_f32<true> : k_resize_area_f32<false>, dim3(cpx_cdiv((long long)dh * ngx, NTHR), gy),
                           dim3(NTHR), 0, s, src, n_planes, sh, sw, dst, dh, dw, ngx);
    } else {
        const int nbx = cpx_cdiv(dw, NTHR);
        hipLaunchKernelGGL(k_resize_linear_f32, dim3(nbx * cpx_cdiv(dh, XPL), gy), dim3(NTHR), 0, s, src, n_planes, sh, sw, dst, dh, dw,
                           nbx, scale_x, scale_y);
    }
    CPX_CHECK_LAUNCH();
    return CPX_OK;
}

// cv::resize INTER_NEAREST (resizeNN): sx = min(cvFloor(x * (1 / inv_scale_x)), sw - 1), likewise in y
template <typename T>
__global__ __launch_bounds__(NTHR) void k_resize_nearest(const T *__restrict__ src, int n_planes, int sh, int sw, T *__restrict__ dst,
                                                         int dh, int dw, double scale_x, double scale_y) {
    const int i = blockIdx.x * NTHR + threadIdx.x;
    if (i >= dh * dw) return;
    const int y = i / dw, x = i - y * dw;
    const int sx = min((int)floor((double)x * scale_x), sw - 1), sy = min((int)floor((double)y * scale_y), sh - 1);
    for (int p = blockIdx.y; p < n_planes; p += gridDim.y)
        dst[(size_t)p * dh * dw + i] = src[((size_t)p * sh + sy) * sw + sx];
}

extern "C" int cpx_resize_nearest(const void *src, int elem_bytes, int n_planes, int sh, int sw, void *dst, int dh, int dw,
                                  void *stream) {
    CPX_REQUIRE(src && dst && (elem_bytes == 1 || elem_bytes == 2) && n_planes > 0 && sh > 0 && sw > 0 && dh > 0 && dw > 0);
    CPX_REQUIRE((long long)dh * dw < (1ll << 31) - NTHR && (long long)sh * sw < (1ll << 31));
    hipStream_t s = (hipStream_t)stream;
    if (sh == dh && sw == dw) {
        CPX_HIP(hipMemcpyAsync(dst, src, (size_t)n_planes * sh * sw * elem_bytes, hipMemcpyDeviceToDevice, s));
        return CPX_OK;
    }
    const double scale_x = 1.0 / ((double)dw / (double)sw), scale_y = 1.0 / ((double)dh / (double)sh);
    const dim3 grid(cpx_cdiv((long long)dh * dw, NTHR), min(n_planes, 65535));
    if (elem_bytes == 1)
        hipLaunchKernelGGL(k_resize_nearest<uint8_t>, grid, dim3(NTHR), 0, s, (const uint8_t *)src, n_planes, sh, sw, (uint8_t *)dst,
                           dh, dw, scale_x, scale_y);
    else
        hipLaunchKernelGGL(k_resize_nearest<uint16_t>, grid, dim3(NTHR), 0, s, (const uint16_t *)src, n_planes, sh, sw,
                           (uint16_t *)dst, dh, dw, scale_x, scale_y);
    CPX_CHECK_LAUNCH();
    return CPX_OK;
}
