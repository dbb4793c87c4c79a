// Training-time augmentation on gfx950 (t2, t4):
//   stain jitter of uint8 patches in the HED colour space (HEDTransform.transform)
//   affine warp of images (bilinear, constant border 0) and class maps (nearest)
//   the same two fused over a device-resident pool of whole images of any size (t4): the random 256 x 256 window that the
//   reference's loader cuts out of the whole image every epoch (dataset.py:23-56), one launch per batch
//   exact percentile normalisation of float32 planes (normalize_img -> normalize99 after the warp)
// None of these is a throughput kernel: one thread per output pixel, planar stores, LDS histograms.
// Built with -ffp-contract=off: the warp's coordinates equal numpy's float64 a * x + b * y + c, and the lerps and the
// quantile arithmetic are the unfused float32 operations of tests/augment_reference.py.
#include "cpx_common.h"

#define NTHR 256

// ---------------------------------------------------------------------------
// stain jitter
// ---------------------------------------------------------------------------
// float32(scipy.linalg.inv(RGB_FROM_HED)) of the reference (tests/golden/reference_augment.npz: HED_FROM_RGB) and
// float32 RGB_FROM_HED, row-major [from][to]
__constant__ float c_hed_from_rgb[9] = {1.87798285f,    -1.00767875f, -0.556115806f, -0.0659080595f, 1.13473034f,
                                        -0.135521799f,  -0.601907432f, -0.480414152f, 1.57358813f};
__constant__ float c_rgb_from_hed[9] = {0.65f, 0.70f, 0.29f, 0.07f, 0.99f, 0.11f, 0.27f, 0.57f, 0.78f};

__device__ __forceinline__ uint32_t byte_sum(uint32_t u) {
    return (u & 0xffu) + ((u >> 8) & 0xffu) + ((u >> 16) & 0xffu) + (u >> 24);
}
// the exact integer sum of p[0 .. count) over a workgroup of 1024 threads; thread 0 returns the total.  Bytes up to the first 16-byte
// boundary (3 * px_off is odd for many image sizes), then 16 per load, then the tail.
__device__ __forceinline__ unsigned long long block_byte_sum(const uint8_t *__restrict__ p, long long count) {
    __shared__ unsigned long long part[16];
    unsigned long long s = 0;
    const long long head = min(count, (long long)((16 - ((uintptr_t)p & 15)) & 15));
    const long long nvec = (count - head) / 16;
    const uint4 *v = reinterpret_cast<const uint4 *>(p + head);
    for (long long i = threadIdx.x; i < head; i += 1024) s += p[i];
    for (long long i = threadIdx.x; i < nvec; i += 1024) {
        const uint4 q = v[i];
        s += byte_sum(q.x) + byte_sum(q.y) + byte_sum(q.z) + byte_sum(q.w);
    }
    for (long long i = head + nvec * 16 + threadIdx.x; i < count; i += 1024) s += p[i];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) s += __shfl_down(s, o);
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = s;
    __syncthreads();
    unsigned long long tot = 0;
    if (threadIdx.x == 0)
        for (int w = 0; w < 16; ++w) tot += part[w];
    return tot;
}

// one workgroup per image: the exact integer sum of its bytes, then the reference's cut-off test in double
__global__ void __launch_bounds__(1024) k_hed_decide(const uint8_t *__restrict__ img, long long count, double lo, double hi,
                                                     int32_t *__restrict__ applied) {
    const unsigned long long tot = block_byte_sum(img + (size_t)blockIdx.x * count, count);
    if (threadIdx.x == 0) {
        const double mean = ((double)tot / (double)count) / 255.0;      // np.mean(patch) / 255.0
        applied[blockIdx.x] = (lo <= mean && mean <= hi) ? 1 : 0;
    }
}


// HEDTransform.transform of one uint8 pixel with the stain draws sigma[3] / bias[3] of its image
__device__ __forceinline__ void hed_pixel(const uint8_t *__restrict__ px, const float *__restrict__ sigma,
                                          const float *__restrict__ bias, int simple_mode, uint8_t *o) {
    float l[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        float v = (float)((double)px[c] / 255.0);                       // (patch / 255.0).astype(float32)
        if (simple_mode) v = fminf(fmaxf(v, 1e-6f), 1.0f);
        else v = v + 1.0f;                                              // shift = 1: the minimum of a uint8 patch is >= 0
        l[c] = -logf(v);
    }
    float h[3];
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        float s = l[0] * c_hed_from_rgb[j] + l[1] * c_hed_from_rgb[3 + j] + l[2] * c_hed_from_rgb[6 + j];
        s = s * (1.0f + sigma[j]) + bias[j];
        h[j] = -s;
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        float x = expf(h[0] * c_rgb_from_hed[c] + h[1] * c_rgb_from_hed[3 + c] + h[2] * c_rgb_from_hed[6 + c]);
        if (!simple_mode) {
            x = x - 1.0f;
            x = fminf(fmaxf(x, -1.0f), 1.0f);                           // rescale_intensity(in_range=(-1, 1)) onto (-1, 1)
            x = (x - (-1.0f)) / 2.0f * 2.0f + (-1.0f);
        }
        x = fminf(fmaxf(x, 0.0f), 1.0f);
        o[c] = (uint8_t)(int)(x * 255.0f);                              // astype(uint8): truncation
    }
}

__global__ void k_hed_jitter(const uint8_t *__restrict__ img, const float *__restrict__ sigma, const float *__restrict__ bias,
                             const int32_t *__restrict__ applied, int HW, int simple_mode, uint8_t *__restrict__ out) {
    const int p = blockIdx.x * NTHR + threadIdx.x;
    if (p >= HW) return;
    const size_t t = blockIdx.y;
    const uint8_t *px = img + (t * HW + p) * 3;
    uint8_t *o = out + (t * HW + p) * 3;
    if (!applied[t]) { o[0] = px[0]; o[1] = px[1]; o[2] = px[2]; return; }
    uint8_t r[3];
    hed_pixel(px, sigma + t * 3, bias + t * 3, simple_mode, r);
    o[0] = r[0]; o[1] = r[1]; o[2] = r[2];
}

extern "C" int cpx_hed_jitter_u8(const uint8_t *img, int n, int H, int W, const float *sigma, const float *bias,
                                 double cutoff_lo, double cutoff_hi, int simple_mode, uint8_t *out, int32_t *applied,
                                 void *stream) {
    CPX_REQUIRE(img && sigma && bias && out && applied && img != out && n > 0 && n <= 65535 && H > 0 && W > 0);
    CPX_REQUIRE((long long)H * W < (1ll << 29));
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(k_hed_decide, dim3(n), dim3(1024), 0, s, img, (long long)H * W * 3, cutoff_lo, cutoff_hi, applied);
    hipLaunchKernelGGL(k_hed_jitter, dim3(cpx_cdiv((long long)H * W, NTHR), n), dim3(NTHR), 0, s, img, sigma, bias, applied,
                       H * W, simple_mode ? 1 : 0, out);
    CPX_CHECK_LAUNCH();
    return CPX_OK;
}

// ---------------------------------------------------------------------------
// H&E stain-matrix perturbation (t5): augment_stains / stains_to_rgb of transforms/he_staining.py
// ---------------------------------------------------------------------------
// The stain basis is a per-image constant that the host fits once (NMF on the samples of cpx_stain_samples); the device
// re-renders.  float64 throughout, unfused.  The 256-entry density table max(-log(max(b, 1) / 255), 1e-6) comes from the host
// (numpy's own values) and sits in LDS: a byte-indexed, lane-divergent 8-byte read that a constant-address-space table would
// turn into a global gather.  The exp is the one double-precision transcendental per channel.
#define HE_NPAR 14      // per crop: Hinv [3][2], M [2][3], the two stain factors 1 + amount_stains * u_j

__device__ __forceinline__ void he_pixel(const uint8_t *__restrict__ px, const double *__restrict__ par,
                                         const double *dens, uint8_t *o) {
    const double d0 = dens[px[0]], d1 = dens[px[1]], d2 = dens[px[2]];
    double s[2];
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const double c = d0 * par[j] + d1 * par[2 + j] + d2 * par[4 + j];  // density @ Hinv
        s[j] = fmax(c * par[12 + j], 0.0);                                  // np.maximum(stains * (1 + amount * u), 0)
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const double x = s[0] * par[6 + c] + s[1] * par[9 + c];            // stains @ M
        const double v = fmin(fmax(255.0 * exp(-x), 0.0), 255.0);           // np.clip(255 * np.exp(-x), 0, 255)
        o[c] = (uint8_t)(int)v;                                             // astype(uint8): truncation
    }
}

__global__ void __launch_bounds__(NTHR) k_he_stain(const uint8_t *__restrict__ img, const double *__restrict__ params,
                                                   const int32_t *__restrict__ mode, const double *__restrict__ density, int HW,
                                                   uint8_t *__restrict__ out) {
    __shared__ double s_dens[256];
    s_dens[threadIdx.x] = density[threadIdx.x];
    __syncthreads();
    const int p = blockIdx.x * NTHR + threadIdx.x;
    if (p >= HW) return;
    const size_t t = blockIdx.y;
    const uint8_t *px = img + (t * HW + p) * 3;
    uint8_t *o = out + (t * HW + p) * 3;
    if (mode[t] != 2) { o[0] = px[0]; o[1] = px[1]; o[2] = px[2]; return; }
    uint8_t r[3];
    he_pixel(px, params + t * HE_NPAR, s_dens, r);
    o[0] = r[0]; o[1] = r[1]; o[2] = r[2];
}

extern "C" int cpx_he_stain_u8(const uint8_t *img, int n, int H, int W, const double *params, const int32_t *mode,
                               const double *density, uint8_t *out, void *stream) {
    CPX_REQUIRE(img && params && mode && density && out && img != out && n > 0 && n <= 65535 && H > 0 && W > 0);
    CPX_REQUIRE((long long)H * W < (1ll << 29));
    hipLaunchKernelGGL(k_he_stain, dim3(cpx_cdiv((long long)H * W, NTHR), n), dim3(NTHR), 0, (hipStream_t)stream, img, params,
                       mode, density, H * W, out);
    CPX_CHECK_LAUNCH();
    return CPX_OK;
}

// ---------------------------------------------------------------------------
// the colour stage of the pool kernels' taps
// ---------------------------------------------------------------------------
// one pixel: mode 0 none, 1 hed_pixel, 2 he_pixel.  The three bytes are loaded before the mode's branches: inside them every load
// waits for the one before it.
__device__ __forceinline__ void colour_pixel(const uint8_t *__restrict__ px, int m, const float *sg, const float *bs, int simple_mode,
                                             const double *par, const double *dens, uint8_t *r) {
    const uint8_t b[3] = {px[0], px[1], px[2]};
    if (m == 2) he_pixel(b, par, dens, r);
    else if (m == 1) hed_pixel(b, sg, bs, simple_mode, r);
    else { r[0] = b[0]; r[1] = b[1]; r[2] = b[2]; }
}

__device__ __forceinline__ bool tap_inside(int sh, int sw, int y, int x) { return (unsigned)y < (unsigned)sh && (unsigned)x < (unsigned)sw; }

// one tap of a crop's source [sh][sw][3]: zeros (not the colour stage of zeros) and false outside it, else colour_pixel of the pixel
__device__ __forceinline__ bool colour_tap(const uint8_t *__restrict__ img, int sh, int sw, int y, int x, int m, const float *sg,
                                           const float *bs, int simple_mode, const double *par, const double *dens, uint8_t *r) {
    if (!tap_inside(sh, sw, y, x)) { r[0] = r[1] = r[2] = 0; return false; }
    colour_pixel(img + ((long long)y * sw + x) * 3, m, sg, bs, simple_mode, par, dens, r);
    return true;
}

// the taps of cpx_warp_affine_pool_u8 (m = 0 / 1, no tables) and cpx_warp_affine_pool_stain_u8: the crop's mode m picks the per-pixel
// function.  The branch on m goes around the four taps, each then sees a constant: with the branch inside every tap
// k_warp_affine_pool measured 1 to 2 % slower where the jitter is on.
struct ColourTaps {
    int m;
    const float *sigma, *bias;
    int simple_mode;
    const double *params, *dens;
    __device__ __forceinline__ bool bytes(int mode, size_t t, const uint8_t *img, int sh, int sw, int y, int x, uint8_t *r) const {
        return colour_tap(img, sh, sw, y, x, mode, sigma + t * 3, bias + t * 3, simple_mode, params + t * HE_NPAR, dens, r);
    }
    __device__ __forceinline__ void tap(int mode, size_t t, const uint8_t *img, int sh, int sw, int y, int x, float *v) const {
        uint8_t r[3];
        v[0] = v[1] = v[2] = 0.f;
        if (bytes(mode, t, img, sh, sw, y, x, r)) { v[0] = (float)r[0]; v[1] = (float)r[1]; v[2] = (float)r[2]; }
    }
    __device__ __forceinline__ void four(int mode, size_t t, const uint8_t *img, int sh, int sw, int y0, int x0, float *a, float *b,
                                         float *d, float *e) const {
        tap(mode, t, img, sh, sw, y0, x0, a);
        tap(mode, t, img, sh, sw, y0, x0 + 1, b);
        tap(mode, t, img, sh, sw, y0 + 1, x0, d);
        tap(mode, t, img, sh, sw, y0 + 1, x0 + 1, e);
    }
    __device__ __forceinline__ void operator()(size_t t, const uint8_t *img, int sh, int sw, int y0, int x0, float *a, float *b,
                                               float *d, float *e) const {
        if (m == 2) four(2, t, img, sh, sw, y0, x0, a, b, d, e);
        else if (m == 1) four(1, t, img, sh, sw, y0, x0, a, b, d, e);
        else four(0, t, img, sh, sw, y0, x0, a, b, d, e);
    }
};

// ---------------------------------------------------------------------------
// affine warp
// ---------------------------------------------------------------------------
// where output pixel (x, y) samples an sh x sw source under the inverse map m[6]: source = m . (x, y, 1) in double
struct WarpGeom {
    double sx, sy;
    bool inside;            // floor(sx) in [-1, sw - 1] and floor(sy) in [-1, sh - 1], or every tap is outside (NaN lands here too)
    int x0, y0;             // the upper left of the four taps
    float wx, wy;           // the bilinear weights
    // the label rule: the nearest pixel (nx, ny) = floor(s + 0.5), false where it lies outside the source.  Left to the caller's label
    // branch, behind the taps: formed ahead of them it sat on every pixel's way to its loads (k_warp_affine_pool 1 % slower)
    __device__ __forceinline__ bool nearest(int sh, int sw, int *nx, int *ny) const {
        const double fx = floor(sx + 0.5), fy = floor(sy + 0.5);
        if (!(fx >= 0.0 && fx < (double)sw && fy >= 0.0 && fy < (double)sh)) return false;
        *nx = (int)fx; *ny = (int)fy;
        return true;
    }
};
__device__ __forceinline__ WarpGeom warp_geom(const double *__restrict__ m, int x, int y, int sh, int sw) {
    WarpGeom g = {};
    g.sx = m[0] * (double)x + m[1] * (double)y + m[2];
    g.sy = m[3] * (double)x + m[4] * (double)y + m[5];
    g.inside = g.sx >= -1.0 && g.sx < (double)sw && g.sy >= -1.0 && g.sy < (double)sh;
    if (g.inside) {
        const double fx = floor(g.sx), fy = floor(g.sy);
        g.x0 = (int)fx; g.y0 = (int)fy;
        g.wx = (float)(g.sx - fx); g.wy = (float)(g.sy - fy);
    }
    return g;
}
// taps a, b of row y0 and d, e of row y0 + 1
__device__ __forceinline__ float bilerp(float a, float b, float d, float e, float wx, float wy) {
    const float top = a + (b - a) * wx;
    const float bot = d + (e - d) * wx;
    return top + (bot - top) * wy;
}

// U8: src [n][sh][sw][3] uint8, else [n][3][sh][sw] float32.  A tap outside the source is 0 on its own.
template <bool U8>
__device__ __forceinline__ float warp_tap(const void *src, size_t t, int sh, int sw, int c, int y, int x) {
    if (!tap_inside(sh, sw, y, x)) return 0.f;
    if (U8) return (float)((const uint8_t *)src)[((t * sh + y) * sw + x) * 3 + c];
    return ((const float *)src)[((t * 3 + c) * sh + y) * sw + x];
}

template <bool U8>
__global__ void k_warp_affine(const void *__restrict__ src, const int16_t *__restrict__ lab, int sh, int sw,
                              const double *__restrict__ inv, int dh, int dw, int label_fill, float *__restrict__ out,
                              int16_t *__restrict__ lab_out) {
    const int p = blockIdx.x * NTHR + threadIdx.x;
    if (p >= dh * dw) return;
    const size_t t = blockIdx.y;
    const int y = p / dw, x = p - y * dw;
    const WarpGeom g = warp_geom(inv + t * 6, x, y, sh, sw);
    float v[3] = {0.f, 0.f, 0.f};
    if (g.inside) {
#pragma unroll
        for (int c = 0; c < 3; ++c)
            v[c] = bilerp(warp_tap<U8>(src, t, sh, sw, c, g.y0, g.x0), warp_tap<U8>(src, t, sh, sw, c, g.y0, g.x0 + 1),
                          warp_tap<U8>(src, t, sh, sw, c, g.y0 + 1, g.x0), warp_tap<U8>(src, t, sh, sw, c, g.y0 + 1, g.x0 + 1), g.wx, g.wy);
    }
    const size_t plane = (size_t)dh * dw;
#pragma unroll
    for (int c = 0; c < 3; ++c) out[(t * 3 + c) * plane + p] = v[c];
    if (lab) {
        int nx, ny;
        lab_out[t * plane + p] = (int16_t)(g.nearest(sh, sw, &nx, &ny) ? lab[(t * sh + ny) * sw + nx] : label_fill);
    }
}


template <bool U8>
static int warp_launch(const void *src, const int16_t *labels, int n, int sh, int sw, const double *inv, int dh, int dw,
                       int label_fill, float *out, int16_t *labels_out, void *stream) {
    CPX_REQUIRE(src && inv && out && n > 0 && n <= 65535 && sh > 0 && sw > 0 && dh > 0 && dw > 0);
    CPX_REQUIRE((labels == nullptr) == (labels_out == nullptr));
    CPX_REQUIRE((long long)sh * sw < (1ll << 29) && (long long)dh * dw < (1ll << 29));
    CPX_REQUIRE(label_fill >= -32768 && label_fill <= 32767);
    hipLaunchKernelGGL(k_warp_affine<U8>, dim3(cpx_cdiv((long long)dh * dw, NTHR), n), dim3(NTHR), 0, (hipStream_t)stream,
                       src, labels, sh, sw, inv, dh, dw, label_fill, out, labels_out);
    CPX_CHECK_LAUNCH();
    return CPX_OK;
}

extern "C" int cpx_warp_affine_u8(const uint8_t *src, const int16_t *labels, int n, int sh, int sw, const double *inv,
                                  int dh, int dw, int label_fill, float *out, int16_t *labels_out, void *stream) {
    return warp_launch<true>(src, labels, n, sh, sw, inv, dh, dw, label_fill, out, labels_out, stream);
}
extern "C" int cpx_warp_affine_f32(const float *src, const int16_t *labels, int n, int sh, int sw, const double *inv,
                                   int dh, int dw, int label_fill, float *out, int16_t *labels_out, void *stream) {
    CPX_REQUIRE((const void *)src != (const void *)out);
    return warp_launch<false>(src, labels, n, sh, sw, inv, dh, dw, label_fill, out, labels_out, stream);
}

// ---------------------------------------------------------------------------
// ragged image pool (t4): whole annotated images of any size, packed back to back
// ---------------------------------------------------------------------------
// image i: pool_u8 + 3 * px_off[i], hw[i] = {h, w}; a table entry that does not lie inside the pool's pool_px pixels is never read
__device__ __forceinline__ bool pool_entry_ok(long long off, int h, int w, long long pool_px) {
    return off >= 0 && h > 0 && w > 0 && off <= pool_px && (long long)h * w <= pool_px - off;
}


// crop t's source in the pool: bad = 1 for an image_of[t] outside the pool's images, 2 for a table entry outside the pool (nothing of
// the pool may be read for such a crop), else 0 with the image's pixel offset and size
struct PoolSource {
    int bad, sh, sw;
    long long off;
};
__device__ __forceinline__ PoolSource pool_source(const int64_t *__restrict__ px_off, const int32_t *__restrict__ hw, int nI,
                                                  long long pool_px, const int32_t *__restrict__ image_of, size_t t) {
    PoolSource s = {0, 0, 0, 0};
    const int im = image_of[t];
    if (im < 0 || im >= nI) s.bad = 1;
    else {
        s.off = px_off[im]; s.sh = hw[2 * im]; s.sw = hw[2 * im + 1];
        if (!pool_entry_ok(s.off, s.sh, s.sw, pool_px)) s.bad = 2;
    }
    return s;
}

// one workgroup per image: the exact integer sum of its bytes (what k_hed_decide forms per patch)
__global__ void __launch_bounds__(1024) k_pool_byte_sums(const uint8_t *__restrict__ pool, const int64_t *__restrict__ px_off,
                                                         const int32_t *__restrict__ hw, long long pool_px,
                                                         unsigned long long *__restrict__ sums, int32_t *__restrict__ status) {
    const int i = blockIdx.x;
    const long long off = px_off[i];
    const int h = hw[2 * i], w = hw[2 * i + 1];
    if (!pool_entry_ok(off, h, w, pool_px)) {                           // uniform over the workgroup
        if (threadIdx.x == 0) { sums[i] = 0; atomicOr(status, 2); }
        return;
    }
    const unsigned long long tot = block_byte_sum(pool + 3 * off, 3ll * h * w);
    if (threadIdx.x == 0) sums[i] = tot;
}


extern "C" int cpx_pool_byte_sums(const uint8_t *pool_u8, const int64_t *px_off, const int32_t *hw, int nI, long long pool_px,
                                  uint64_t *sums, int32_t *status, void *stream) {
    CPX_REQUIRE(pool_u8 && px_off && hw && sums && status && nI > 0 && pool_px > 0);
    hipStream_t s = (hipStream_t)stream;
    CPX_HIP(hipMemsetAsync(status, 0, sizeof(int32_t), s));
    hipLaunchKernelGGL(k_pool_byte_sums, dim3(nI), dim3(1024), 0, s, pool_u8, px_off, hw, pool_px,
                       reinterpret_cast<unsigned long long *>(sums), status);
    CPX_CHECK_LAUNCH();
    return CPX_OK;
}

// k_warp_affine<true> with a source per crop, image_of[t] of the pool, and a per-pixel colour transform folded into the taps:
// f(tap) of an in-source tap, 0 (not f(0)) outside -- bitwise the transform of the whole image followed by the warp.  `taps` fills
// the four neighbours a, b (row y0) and d, e (row y0 + 1) of crop t; the source lookup, the geometry and the label rule are shared
// by every pool kernel.
template <class Taps>
__device__ __forceinline__ void warp_pool_pixel(const uint8_t *__restrict__ pool, const int16_t *__restrict__ pool_lab,
                                                const int64_t *__restrict__ px_off, const int32_t *__restrict__ hw, int nI,
                                                long long pool_px, const int32_t *__restrict__ image_of,
                                                const double *__restrict__ inv, int dh, int dw, int label_fill,
                                                float *__restrict__ out, int16_t *__restrict__ lab_out,
                                                int32_t *__restrict__ status, const Taps &taps) {
    const int p = blockIdx.x * NTHR + threadIdx.x;
    if (p >= dh * dw) return;
    const size_t t = blockIdx.y;
    const size_t plane = (size_t)dh * dw;
    const PoolSource s = pool_source(px_off, hw, nI, pool_px, image_of, t);
    if (s.bad) {
#pragma unroll
        for (int c = 0; c < 3; ++c) out[(t * 3 + c) * plane + p] = 0.f;
        if (lab_out) lab_out[t * plane + p] = (int16_t)label_fill;
        if (p == 0) atomicOr(status, s.bad);
        return;
    }
    const int y = p / dw, x = p - y * dw;
    const WarpGeom g = warp_geom(inv + t * 6, x, y, s.sh, s.sw);
    float v[3] = {0.f, 0.f, 0.f};
    if (g.inside) {
        float a[3], b[3], d[3], e[3];
        taps(t, pool + 3 * s.off, s.sh, s.sw, g.y0, g.x0, a, b, d, e);
#pragma unroll
        for (int c = 0; c < 3; ++c) v[c] = bilerp(a[c], b[c], d[c], e[c], g.wx, g.wy);
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) out[(t * 3 + c) * plane + p] = v[c];
    if (lab_out) {
        int nx, ny;
        lab_out[t * plane + p] = (int16_t)(g.nearest(s.sh, s.sw, &nx, &ny) ? pool_lab[s.off + (long long)ny * s.sw + nx] : label_fill);
    }
}

// what the pool warps require of the arguments they share (pool: uint8 or float32); clears the status word
static int pool_warp_require(const void *pool, const int16_t *pool_lab, const int64_t *px_off, const int32_t *hw, int nI,
                             long long pool_px, const int32_t *image_of, const double *inv, int n, int dh, int dw, int label_fill,
                             const float *out, const int16_t *labels_out, int32_t *status, hipStream_t s) {
    CPX_REQUIRE(pool && px_off && hw && image_of && inv && out && status && nI > 0 && pool_px > 0);
    CPX_REQUIRE(n > 0 && n <= 65535 && dh > 0 && dw > 0 && (long long)dh * dw < (1ll << 29));
    CPX_REQUIRE((pool_lab == nullptr) == (labels_out == nullptr));
    CPX_REQUIRE(label_fill >= -32768 && label_fill <= 32767);
    CPX_HIP(hipMemsetAsync(status, 0, sizeof(int32_t), s));
    return CPX_OK;
}


__global__ void k_warp_affine_pool(const uint8_t *__restrict__ pool, const int16_t *__restrict__ pool_lab,
                                   const int64_t *__restrict__ px_off, const int32_t *__restrict__ hw, int nI, long long pool_px,
                                   const int32_t *__restrict__ image_of, const double *__restrict__ inv,
                                   const float *__restrict__ sigma, const float *__restrict__ bias,
                                   const int32_t *__restrict__ applied, int simple_mode, int dh, int dw, int label_fill,
                                   float *__restrict__ out, int16_t *__restrict__ lab_out, int32_t *__restrict__ status) {
    const int m = (sigma && applied[blockIdx.y]) ? 1 : 0;               // through hed_pixel where the crop's image is jittered
    warp_pool_pixel(pool, pool_lab, px_off, hw, nI, pool_px, image_of, inv, dh, dw, label_fill, out, lab_out, status,
                    ColourTaps{m, sigma, bias, simple_mode, nullptr, nullptr});
}

extern "C" int cpx_warp_affine_pool_u8(const uint8_t *pool_u8, const int16_t *pool_lab, const int64_t *px_off, const int32_t *hw,
                                       int nI, long long pool_px, const int32_t *image_of, const double *inv, int n,
                                       const float *sigma, const float *bias, const int32_t *applied, int simple_mode, int dh,
                                       int dw, int label_fill, float *out, int16_t *labels_out, int32_t *status, void *stream) {
    hipStream_t s = (hipStream_t)stream;
    CPX_REQUIRE((sigma == nullptr) == (bias == nullptr) && (sigma == nullptr) == (applied == nullptr));
    if (int rc = pool_warp_require(pool_u8, pool_lab, px_off, hw, nI, pool_px, image_of, inv, n, dh, dw, label_fill, out, labels_out,
                                   status, s))
        return rc;
    hipLaunchKernelGGL(k_warp_affine_pool, dim3(cpx_cdiv((long long)dh * dw, NTHR), n), dim3(NTHR), 0, s, pool_u8, pool_lab,
                       px_off, hw, nI, pool_px, image_of, inv, sigma, bias, applied, simple_mode ? 1 : 0, dh, dw, label_fill, out,
                       labels_out, status);
    CPX_CHECK_LAUNCH();
    return CPX_OK;
}

// t8: the flow-head targets (mask, flow Y, flow X), three float32 planes per image at float 3 * px_off[i], under the crop's map:
// the flow branch of cellpose transforms.random_rotate_and_resize (lbl[1:] warped bilinearly, the X flow of a flipped source
// negated, then the pair rotated by theta; restated from cellpose 4.0.x).  Source lookup, geometry and lerps are warp_pool_pixel's.
__device__ __forceinline__ float flow_tap(const float *__restrict__ plane, int sh, int sw, int y, int x) {
    return tap_inside(sh, sw, y, x) ? plane[(long long)y * sw + x] : 0.f;
}

__global__ void k_warp_affine_pool_flow(const float *__restrict__ pool_tgt, const int64_t *__restrict__ px_off,
                                        const int32_t *__restrict__ hw, int nI, long long pool_px,
                                        const int32_t *__restrict__ image_of, const double *__restrict__ inv,
                                        const double *__restrict__ vec, int dh, int dw, float *__restrict__ out,
                                        int32_t *__restrict__ status) {
    const int p = blockIdx.x * NTHR + threadIdx.x;
    if (p >= dh * dw) return;
    const size_t t = blockIdx.y;
    const size_t plane = (size_t)dh * dw;
    const PoolSource s = pool_source(px_off, hw, nI, pool_px, image_of, t);
    float v[3] = {0.f, 0.f, 0.f};
    if (s.bad) {
        if (p == 0) atomicOr(status, s.bad);
    } else {
        const long long spx = (long long)s.sh * s.sw;
        const int y = p / dw, x = p - y * dw;
        const WarpGeom g = warp_geom(inv + t * 6, x, y, s.sh, s.sw);
        if (g.inside) {
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const float *pl = pool_tgt + 3 * s.off + c * spx;
                v[c] = bilerp(flow_tap(pl, s.sh, s.sw, g.y0, g.x0), flow_tap(pl, s.sh, s.sw, g.y0, g.x0 + 1),
                              flow_tap(pl, s.sh, s.sw, g.y0 + 1, g.x0), flow_tap(pl, s.sh, s.sw, g.y0 + 1, g.x0 + 1), g.wx, g.wy);
            }
        }
        const double *r = vec + t * 4;
        const float r0 = (float)r[0], r1 = (float)r[1], r2 = (float)r[2], r3 = (float)r[3];
        const float y0p = r0 * v[1], y1p = r1 * v[2], x0p = r2 * v[1], x1p = r3 * v[2];     // (-ffp-contract=off: no fma)
        v[1] = y0p + y1p;
        v[2] = x0p + x1p;
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) out[(t * 3 + c) * plane + p] = v[c];
}

extern "C" int cpx_warp_affine_pool_flow_f32(const float *pool_tgt, const int64_t *px_off, const int32_t *hw, int nI,
                                             long long pool_px, const int32_t *image_of, const double *inv, const double *vec,
                                             int n, int dh, int dw, float *out, int32_t *status, void *stream) {
    hipStream_t s = (hipStream_t)stream;
    CPX_REQUIRE(vec);
    if (int rc = pool_warp_require(pool_tgt, nullptr, px_off, hw, nI, pool_px, image_of, inv, n, dh, dw, 0, out, nullptr, status, s))
        return rc;
    hipLaunchKernelGGL(k_warp_affine_pool_flow, dim3(cpx_cdiv((long long)dh * dw, NTHR), n), dim3(NTHR), 0, s, pool_tgt, px_off, hw,
                       nI, pool_px, image_of, inv, vec, dh, dw, out, status);
    CPX_CHECK_LAUNCH();
    return CPX_OK;
}

// cpx_warp_affine_pool_u8 with the crop's mode out of a table, and the density table of he_pixel in LDS
__global__ void __launch_bounds__(NTHR) k_warp_affine_pool_stain(
    const uint8_t *__restrict__ pool, const int16_t *__restrict__ pool_lab, const int64_t *__restrict__ px_off,
    const int32_t *__restrict__ hw, int nI, long long pool_px, const int32_t *__restrict__ image_of, const double *__restrict__ inv,
    const float *__restrict__ sigma, const float *__restrict__ bias, int simple_mode, const double *__restrict__ params,
    const double *__restrict__ density, const int32_t *__restrict__ mode, int dh, int dw, int label_fill, float *__restrict__ out,
    int16_t *__restrict__ lab_out, int32_t *__restrict__ status) {
    __shared__ double s_dens[256];
    s_dens[threadIdx.x] = density[threadIdx.x];
    __syncthreads();
    warp_pool_pixel(pool, pool_lab, px_off, hw, nI, pool_px, image_of, inv, dh, dw, label_fill, out, lab_out, status,
                    ColourTaps{mode[blockIdx.y], sigma, bias, simple_mode, params, s_dens});
}

extern "C" int cpx_warp_affine_pool_stain_u8(const uint8_t *pool_u8, const int16_t *pool_lab, const int64_t *px_off,
                                             const int32_t *hw, int nI, long long pool_px, const int32_t *image_of,
                                             const double *inv, int n, const float *sigma, const float *bias, int simple_mode,
                                             const double *stain_params, const double *density, const int32_t *mode, int dh,
                                             int dw, int label_fill, float *out, int16_t *labels_out, int32_t *status,
                                             void *stream) {
    hipStream_t s = (hipStream_t)stream;
    CPX_REQUIRE(sigma && bias && stain_params && density && mode);
    if (int rc = pool_warp_require(pool_u8, pool_lab, px_off, hw, nI, pool_px, image_of, inv, n, dh, dw, label_fill, out, labels_out,
                                   status, s))
        return rc;
    hipLaunchKernelGGL(k_warp_affine_pool_stain, dim3(cpx_cdiv((long long)dh * dw, NTHR), n), dim3(NTHR), 0, s, pool_u8, pool_lab,
                       px_off, hw, nI, pool_px, image_of, inv, sigma, bias, simple_mode ? 1 : 0, stain_params, density, mode, dh,
                       dw, label_fill, out, labels_out, status);
    CPX_CHECK_LAUNCH();
    return CPX_OK;
}


// ---------------------------------------------------------------------------
// tissue samples of every image of a pool: values = density[tissue_mask] (all pixels when the mask is empty), values[::128]
// when there are more than 128 (extract_stains, he_staining.py:74-93).  Density is a function of the byte, so the selected
// pixels' bytes are what comes back.  An ordered stream compaction with a stride pick, in three launches: tissue pixels per
// chunk of SS_CHUNK raster-ordered pixels (ballots), one workgroup per image scanning its chunk counts into exclusive prefixes
// and k_i, then every tissue pixel's global rank and the store of the selected ranks.  Integer counts only, no atomics on
// data: the result does not depend on the launch geometry.
// Chunk c of image i sits in slot px_off[i] / SS_CHUNK + i + c of the workspace: for images packed back to back these ranges do
// not overlap, and for every entry that lies inside the pool they end below pool_px / SS_CHUNK + nI + 1.  An image's
// workgroups read nothing but their own table entry, so a bad entry costs its own image only.
// ---------------------------------------------------------------------------
#define SS_CHUNK 1024
#define SS_IT (SS_CHUNK / NTHR)

__device__ __forceinline__ int stain_cap(long long px) { return (int)max(128ll, (px + 127) / 128); }
__device__ __forceinline__ bool stain_out_ok(long long oo, long long px, long long out_triples) {
    return oo >= 0 && oo <= out_triples && (long long)stain_cap(px) <= out_triples - oo;
}
__device__ __forceinline__ long long stain_slot_base(const int64_t *px_off, int i) { return px_off[i] / SS_CHUNK + i; }
__device__ __forceinline__ bool tissue_px(const uint8_t *px, const double *lin, double y_t) {
    return (0.212671 * lin[px[0]] + 0.715160 * lin[px[1]]) + 0.072169 * lin[px[2]] < y_t;
}

// workgroups (i, 0 .. gridDim.y - 1) share the chunks of image i, chunk c going to workgroup c % gridDim.y: the counts land per
// chunk, so the geometry shows nowhere in the result
__global__ void __launch_bounds__(NTHR) k_stain_count(const uint8_t *__restrict__ pool, const int64_t *__restrict__ px_off,
                                                      const int32_t *__restrict__ hw, long long pool_px,
                                                      const double *__restrict__ lin, double y_t,
                                                      unsigned long long *__restrict__ counts) {
    __shared__ double s_lin[256];
    __shared__ uint32_t part[NTHR / 64];
    const int i = blockIdx.x;
    const long long off = px_off[i];
    const int h = hw[2 * i], w = hw[2 * i + 1];
    if (!pool_entry_ok(off, h, w, pool_px)) return;                     // uniform over the workgroup
    const long long px = (long long)h * w, nch = (px + SS_CHUNK - 1) / SS_CHUNK;
    s_lin[threadIdx.x] = lin[threadIdx.x];
    __syncthreads();
    const uint8_t *img = pool + 3 * off;
    unsigned long long *cnt_out = counts + stain_slot_base(px_off, i);
    for (long long chunk = blockIdx.y; chunk < nch; chunk += gridDim.y) {
        uint32_t cnt = 0;
#pragma unroll
        for (int it = 0; it < SS_IT; ++it) {
            const long long p = chunk * SS_CHUNK + it * NTHR + threadIdx.x;
            const bool m = p < px && tissue_px(img + 3 * p, s_lin, y_t);
            cnt += (uint32_t)__popcll(__ballot(m));
        }
        if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = cnt;
        __syncthreads();
        if (threadIdx.x == 0) {
            uint32_t tot = 0;
            for (int k = 0; k < NTHR / 64; ++k) tot += part[k];
            cnt_out[chunk] = tot;
        }
        __syncthreads();
    }
}

// one workgroup per image: chunk counts -> exclusive prefixes in place, k_i; status bit 1 for a table entry outside the pool,
// bit 2 for an output range outside the sample buffer
__global__ void __launch_bounds__(1024) k_stain_scan(const int64_t *__restrict__ px_off, const int32_t *__restrict__ hw,
                                                     long long pool_px, const int64_t *__restrict__ out_off, long long out_triples,
                                                     unsigned long long *__restrict__ counts, int64_t *__restrict__ k_out,
                                                     int32_t *__restrict__ status) {
    __shared__ unsigned long long wtot[16];
    const int i = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const long long off = px_off[i];
    const int h = hw[2 * i], w = hw[2 * i + 1];
    if (!pool_entry_ok(off, h, w, pool_px)) {
        if (tid == 0) { k_out[i] = 0; atomicOr(status, 2); }
        return;
    }
    const long long px = (long long)h * w;
    if (!stain_out_ok(out_off[i], px, out_triples)) {
        if (tid == 0) { k_out[i] = 0; atomicOr(status, 4); }
        return;
    }
    const long long nch = (px + SS_CHUNK - 1) / SS_CHUNK;
    unsigned long long *cnt = counts + stain_slot_base(px_off, i);
    unsigned long long carry = 0;
    for (long long c0 = 0; c0 < nch; c0 += 1024) {
        const long long c = c0 + tid;
        const unsigned long long v = c < nch ? cnt[c] : 0ull;
        unsigned long long incl = v;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const unsigned long long up = __shfl_up(incl, o);
            if (lane >= o) incl += up;
        }
        if (lane == 63) wtot[wave] = incl;
        __syncthreads();
        unsigned long long before = 0, total = 0;
        for (int k = 0; k < 16; ++k) {
            const unsigned long long t = wtot[k];
            if (k < wave) before += t;
            total += t;
        }
        if (c < nch) cnt[c] = carry + before + incl - v;
        carry += total;
        __syncthreads();
    }
    if (tid == 0) k_out[i] = (int64_t)carry;
}

__global__ void __launch_bounds__(NTHR) k_stain_select(const uint8_t *__restrict__ pool, const int64_t *__restrict__ px_off,
                                                       const int32_t *__restrict__ hw, long long pool_px,
                                                       const double *__restrict__ lin, double y_t,
                                                       const unsigned long long *__restrict__ prefix,
                                                       const int64_t *__restrict__ k_in, const int64_t *__restrict__ out_off,
                                                       long long out_triples, uint8_t *__restrict__ samples) {
    __shared__ double s_lin[256];
    __shared__ uint32_t seg[SS_IT * (NTHR / 64)];
    const int i = blockIdx.x;
    const long long off = px_off[i];
    const int h = hw[2 * i], w = hw[2 * i + 1];
    if (!pool_entry_ok(off, h, w, pool_px)) return;                     // uniform over the workgroup, here and below
    const long long px = (long long)h * w, nch = (px + SS_CHUNK - 1) / SS_CHUNK;
    const long long oo = out_off[i];
    if (!stain_out_ok(oo, px, out_triples)) return;
    s_lin[threadIdx.x] = lin[threadIdx.x];
    __syncthreads();
    const long long k = k_in[i];
    const bool all = k == 0;                                            // no tissue pixel: every pixel is a value
    const long long N = all ? px : k;
    const bool stride = N > 128;
    const int cap = stain_cap(px), lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint8_t *img = pool + 3 * off;
    const unsigned long long *pre = prefix + stain_slot_base(px_off, i);
    for (long long chunk = blockIdx.y; chunk < nch; chunk += gridDim.y) {
        bool m[SS_IT];
        unsigned long long bal[SS_IT];
#pragma unroll
        for (int it = 0; it < SS_IT; ++it) {
            const long long p = chunk * SS_CHUNK + it * NTHR + threadIdx.x;
            m[it] = p < px && (all || tissue_px(img + 3 * p, s_lin, y_t));
            bal[it] = __ballot(m[it]);
            if (lane == 0) seg[it * (NTHR / 64) + wave] = (uint32_t)__popcll(bal[it]);
        }
        __syncthreads();
        const long long first = all ? chunk * SS_CHUNK : (long long)pre[chunk];
#pragma unroll
        for (int it = 0; it < SS_IT; ++it) {
            if (!m[it]) continue;
            long long r = first;                                        // the pixel's rank among the image's values
            for (int q = 0; q < it * (NTHR / 64) + wave; ++q) r += seg[q];
            r += __popcll(bal[it] & ((1ull << lane) - 1ull));
            if (stride && (r & 127)) continue;
            const long long slot = stride ? (r >> 7) : r;
            if (slot >= cap) continue;                                  // cannot happen with a consistent table
            const uint8_t *px3 = img + 3 * (chunk * SS_CHUNK + it * NTHR + threadIdx.x);
            uint8_t *o = samples + 3 * (oo + slot);
            o[0] = px3[0]; o[1] = px3[1]; o[2] = px3[2];
        }
        __syncthreads();
    }
}

extern "C" size_t cpx_stain_samples_workspace_bytes(int nI, long long pool_px) {
    if (nI <= 0 || pool_px <= 0) return 0;
    return (size_t)(pool_px / SS_CHUNK + nI + 1) * sizeof(unsigned long long);
}

extern "C" int cpx_stain_samples(const uint8_t *pool_u8, const int64_t *px_off, const int32_t *hw, int nI, long long pool_px,
                                 const double *lin, double y_t, const int64_t *out_off, long long out_triples, int64_t *k,
                                 uint8_t *samples, int32_t *status, void *workspace, size_t workspace_bytes, void *stream) {
    CPX_REQUIRE(pool_u8 && px_off && hw && lin && out_off && k && samples && status && workspace);
    CPX_REQUIRE(nI > 0 && nI <= (1 << 24) && pool_px > 0 && out_triples > 0);
    CPX_REQUIRE(workspace_bytes >= cpx_stain_samples_workspace_bytes(nI, pool_px) && ((uintptr_t)workspace & 7) == 0);
    hipStream_t s = (hipStream_t)stream;
    unsigned long long *counts = reinterpret_cast<unsigned long long *>(workspace);
    // workgroups per image: twice the mean chunk count, so that images of about one size get a workgroup per chunk
    const long long mean_chunks = (pool_px / SS_CHUNK) / nI + 1;
    const unsigned per_image = (unsigned)(2 * mean_chunks < 1024 ? 2 * mean_chunks : 1024);
    CPX_HIP(hipMemsetAsync(status, 0, sizeof(int32_t), s));
    hipLaunchKernelGGL(k_stain_count, dim3(nI, per_image), dim3(NTHR), 0, s, pool_u8, px_off, hw, pool_px, lin, y_t, counts);
    hipLaunchKernelGGL(k_stain_scan, dim3(nI), dim3(1024), 0, s, px_off, hw, pool_px, out_off, out_triples, counts, k, status);
    hipLaunchKernelGGL(k_stain_select, dim3(nI, per_image), dim3(NTHR), 0, s, pool_u8, px_off, hw, pool_px, lin, y_t, counts, k,
                       out_off, out_triples, samples);
    CPX_CHECK_LAUNCH();
    return CPX_OK;
}

// ---------------------------------------------------------------------------
// float32 percentile normalisation
// ---------------------------------------------------------------------------
// order-preserving 32-bit key of a float; -0.0 and 0.0 share one key
__device__ __forceinline__ uint32_t f32_key(float x) {
    if (x == 0.f) x = 0.f;
    const uint32_t u = __float_as_uint(x);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float key_f32(uint32_t k) {
    return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k);
}
__device__ __forceinline__ float np_lerp_f32(float a, float b, float t) {      // numpy _lerp in float32
    const float diff = b - a;
    float r = a + diff * t;
    if (t >= 0.5f) r = b - diff * (1.0f - t);
    return r;
}

#define SEL_THR 1024
// One workgroup per (image, channel) plane.  Radix select, most significant byte first: four passes over the plane, each
// a 256-bin LDS histogram per rank of the keys that still match the rank's prefix; wave r then scans histogram r (lane l
// owns bins 4l .. 4l + 3) and picks the bin in which rank r falls.  Ranks with one prefix share a histogram (pass 0: all four).
__global__ void __launch_bounds__(SEL_THR) k_norm_stats_f32(const float *__restrict__ x, int HW, int lo_prev, float lo_g,
                                                            int hi_prev, float hi_g, float *__restrict__ stats) {
    __shared__ uint32_t hist[4][256];
    __shared__ uint32_t s_prefix[4], s_rank[4], s_min, s_max;
    const float *pl = x + (size_t)blockIdx.x * HW;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    if (tid == 0) {
        s_rank[0] = lo_prev; s_rank[1] = min(lo_prev + 1, HW - 1);
        s_rank[2] = hi_prev; s_rank[3] = min(hi_prev + 1, HW - 1);
        s_prefix[0] = s_prefix[1] = s_prefix[2] = s_prefix[3] = 0;
        s_min = 0xffffffffu; s_max = 0;
    }
    uint32_t kmin = 0xffffffffu, kmax = 0;
    for (int pass = 0; pass < 4; ++pass) {
        const int shift = 24 - 8 * pass;
        for (int i = tid; i < 4 * 256; i += SEL_THR) (&hist[0][0])[i] = 0;
        __syncthreads();
        uint32_t pre[4];
        bool own[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            pre[r] = s_prefix[r];
            own[r] = r == 0 || pre[r] != pre[r - 1];         // ranks ascend, so equal prefixes are neighbours
        }
        for (int i = tid; i < HW; i += SEL_THR) {
            const uint32_t k = f32_key(pl[i]);
            const uint32_t d = (k >> shift) & 255u;
            if (pass == 0) {
                // every value counts, and the sign and exponent bits of an image take a handful of values: 64 lanes adding
                // to one LDS word would serialise, so each distinct digit of the wave is added once, by its first lane
                kmin = min(kmin, k); kmax = max(kmax, k);
                unsigned long long todo = __ballot(1);
                while (todo) {
                    const int l = __ffsll((long long)todo) - 1;
                    const uint32_t dl = __shfl(d, l);
                    const unsigned long long m = __ballot(d == dl);
                    if (lane == l) atomicAdd(&hist[0][dl], (uint32_t)__popcll(m));
                    todo &= ~m;
                }
                continue;
            }
            const uint32_t hi_bits = k >> (shift + 8);
#pragma unroll
            for (int r = 0; r < 4; ++r)
                if (own[r] && hi_bits == pre[r]) atomicAdd(&hist[r][d], 1u);
        }
        if (pass == 0) { atomicMin(&s_min, kmin); atomicMax(&s_max, kmax); }
        __syncthreads();
        if (wave < 4) {
            int r = wave;                                    // the histogram of rank `wave` is its owner's
            while (!own[r]) --r;
            const uint32_t *h = hist[r] + 4 * lane;
            const uint32_t c0 = h[0], c1 = c0 + h[1], c2 = c1 + h[2], c3 = c2 + h[3];
            uint32_t incl = c3;
#pragma unroll
            for (int o = 1; o < 64; o <<= 1) {
                const uint32_t up = __shfl_up(incl, o);
                if (lane >= o) incl += up;
            }
            const uint32_t excl = incl - c3, k = s_rank[wave];
            const unsigned long long m = __ballot(incl > k);
            const int l = __ffsll((long long)m) - 1;         // first lane whose cumulative count passes the rank
            if (lane == l) {
                const int sub = excl + c0 > k ? 0 : (excl + c1 > k ? 1 : (excl + c2 > k ? 2 : 3));
                const uint32_t below = excl + (sub == 0 ? 0u : (sub == 1 ? c0 : (sub == 2 ? c1 : c2)));
                s_prefix[wave] = (pre[wave] << 8) | (uint32_t)(4 * lane + sub);
                s_rank[wave] = k - below;                    // rank among the keys that carry the longer prefix
            }
        }
        __syncthreads();
    }
    if (tid != 0) return;
    const float g0 = key_f32(s_prefix[0]), g1 = key_f32(s_prefix[1]), g2 = key_f32(s_prefix[2]), g3 = key_f32(s_prefix[3]);
    const float x01 = np_lerp_f32(g0, g1, lo_g), x99 = np_lerp_f32(g2, g3, hi_g);
    const float den = x99 - x01;
    float mode;
    if (s_max == s_min) mode = 0.f;                          // np.ptp == 0: channel left untouched
    else if (den > (float)1e-3) mode = 1.f;
    else mode = 2.f;
    float *st = stats + (size_t)blockIdx.x * 4;
    st[0] = x01; st[1] = den; st[2] = mode; st[3] = x99;
}

__global__ void k_norm_apply_f32(const float *__restrict__ x, const float *__restrict__ stats, int HW, float *__restrict__ out) {
    const int i = blockIdx.x * NTHR + threadIdx.x;
    if (i >= HW) return;
    const size_t pl = blockIdx.y;
    const float *st = stats + pl * 4;
    float v = x[pl * HW + i];
    const float mode = st[2];
    if (mode == 1.f) { v = v - st[0]; v = __fdiv_rn(v, st[1]); }
    else if (mode == 2.f) v = 0.f;
    out[pl * HW + i] = v;
}

extern "C" int cpx_normalize_stats_f32(const float *img, int n, int H, int W, int lo_prev, float lo_gamma, int hi_prev,
                                       float hi_gamma, float *stats, void *stream) {
    CPX_REQUIRE(img && stats && n > 0 && n <= (1 << 20) && H > 0 && W > 0 && (long long)H * W < (1ll << 30));
    CPX_REQUIRE(lo_prev >= 0 && hi_prev >= lo_prev && hi_prev < H * W);
    hipLaunchKernelGGL(k_norm_stats_f32, dim3(n * 3), dim3(SEL_THR), 0, (hipStream_t)stream, img, H * W, lo_prev, lo_gamma,
                       hi_prev, hi_gamma, stats);
    CPX_CHECK_LAUNCH();
    return CPX_OK;
}

extern "C" int cpx_normalize_apply_f32(const float *img, const float *stats, int n, int H, int W, float *out, void *stream) {
    CPX_REQUIRE(img && stats && out && n > 0 && n <= 21845 && H > 0 && W > 0 && (long long)H * W < (1ll << 30));
    hipLaunchKernelGGL(k_norm_apply_f32, dim3(cpx_cdiv((long long)H * W, NTHR), n * 3), dim3(NTHR), 0, (hipStream_t)stream,
                       img, stats, H * W, out);
    CPX_CHECK_LAUNCH();
    return CPX_OK;
}

// ---------------------------------------------------------------------------
// image quality (t6): Gaussian blur and hue / brightness / saturation jitter of transforms/image_quality.py
// ---------------------------------------------------------------------------
__device__ __forceinline__ float clamp01(float x) { return fminf(fmaxf(x, 0.0f), 1.0f); }

// _hbs_adjust of one uint8 pixel: torchvision's adjust_hue / adjust_brightness / adjust_saturation in float32, one rounding per
// operation (ATen's add_(other, alpha=) being one operation: a fused multiply-add).  par = {hue, brightness, saturation, 1 - saturation}; unit = arange(256, float32) / float32(255) from the host.
__device__ __forceinline__ void hbs_pixel(const uint8_t *px, const float *__restrict__ par, const float *unit, uint8_t *o) {
    float r = unit[px[0]], g = unit[px[1]], b = unit[px[2]];
    const float hue = par[0], bright = par[1], sat = par[2], one_minus_sat = par[3];
    if (hue != 0.0f) {
        const float maxc = fmaxf(fmaxf(r, g), b), minc = fminf(fminf(r, g), b);
        const bool eq = maxc == minc;
        const float cr = maxc - minc;
        const float s = __fdiv_rn(cr, eq ? 1.0f : maxc);
        const float d = eq ? 1.0f : cr;
        const float rc = __fdiv_rn(maxc - r, d), gc = __fdiv_rn(maxc - g, d), bc = __fdiv_rn(maxc - b, d);
        const float hr = (maxc == r) ? bc - gc : 0.0f;
        const float hg = (maxc == g && maxc != r) ? (rc + 2.0f) - bc : 0.0f;
        const float hb = (maxc != g && maxc != r) ? (gc + 4.0f) - rc : 0.0f;
        float h = fmodf(((hr + hg) + hb) * (float)(1.0 / 6.0) + 1.0f, 1.0f);
        h = fmodf(h + hue, 1.0f);                                       // remainder(h + hue, 1) with the divisor's sign
        if (h < 0.0f) h = h + 1.0f;
        const float h6 = h * 6.0f, fl = floorf(h6), f = h6 - fl;
        const int i = ((int)fl) % 6;
        const float v = maxc, sxf = s * f, oms = 1.0f - s;
        const float q = clamp01((1.0f - sxf) * v), t = clamp01((sxf + oms) * v), p = clamp01(oms * v);
        r = i == 0 ? v : (i == 1 ? q : (i == 2 ? p : (i == 3 ? p : (i == 4 ? t : v))));
        g = i == 0 ? t : (i == 1 ? v : (i == 2 ? v : (i == 3 ? q : (i == 4 ? p : p))));
        b = i == 0 ? p : (i == 1 ? p : (i == 2 ? t : (i == 3 ? v : (i == 4 ? v : q))));
    }
    r = clamp01(r * bright); g = clamp01(g * bright); b = clamp01(b * bright);
    if (sat != 1.0f) {
        // r.mul(0.2989).add_(g, alpha=0.587).add_(b, alpha=0.114) and x.mul(sat).add_(gray, alpha=1 - sat): ATen's add with
        // alpha is a fused multiply-add
        const float gray = __fmaf_rn(b, 0.114f, __fmaf_rn(g, 0.587f, r * 0.2989f));
        r = clamp01(__fmaf_rn(gray, one_minus_sat, r * sat));
        g = clamp01(__fmaf_rn(gray, one_minus_sat, g * sat));
        b = clamp01(__fmaf_rn(gray, one_minus_sat, b * sat));
    }
    o[0] = (uint8_t)(int)fminf(fmaxf(r * 255.0f, 0.0f), 255.0f);        // clip(x * 255, 0, 255).astype(uint8): truncation
    o[1] = (uint8_t)(int)fminf(fmaxf(g * 255.0f, 0.0f), 255.0f);
    o[2] = (uint8_t)(int)fminf(fmaxf(b * 255.0f, 0.0f), 255.0f);
}

__global__ void __launch_bounds__(NTHR) k_hbs(const uint8_t *__restrict__ img, const float *__restrict__ hbs,
                                              const int32_t *__restrict__ apply, const float *__restrict__ unit, int HW,
                                              uint8_t *__restrict__ out) {
    __shared__ float s_unit[256];
    s_unit[threadIdx.x] = unit[threadIdx.x];
    __syncthreads();
    const int p = blockIdx.x * NTHR + threadIdx.x;
    if (p >= HW) return;
    const size_t t = blockIdx.y;
    const uint8_t *px = img + (t * HW + p) * 3;
    uint8_t *o = out + (t * HW + p) * 3;
    uint8_t r[3] = {px[0], px[1], px[2]};
    if (apply[t]) hbs_pixel(r, hbs + t * 4, s_unit, r);
    o[0] = r[0]; o[1] = r[1]; o[2] = r[2];
}

extern "C" int cpx_hbs_u8(const uint8_t *img, int n, int H, int W, const float *hbs, const int32_t *apply, const float *unit,
                          uint8_t *out, void *stream) {
    CPX_REQUIRE(img && hbs && apply && unit && out && img != out && n > 0 && n <= 65535 && H > 0 && W > 0);
    CPX_REQUIRE((long long)H * W < (1ll << 29));
    hipLaunchKernelGGL(k_hbs, dim3(cpx_cdiv((long long)H * W, NTHR), n), dim3(NTHR), 0, (hipStream_t)stream, img, hbs, apply, unit,
                       H * W, out);
    CPX_CHECK_LAUNCH();
    return CPX_OK;
}

// Gaussian blur of rectangles of pool images, after the colour stage: scipy.ndimage.gaussian_filter(plane, sigma) per channel
// (mode reflect about the IMAGE's borders, rows first, a truncated uint8 intermediate, double accumulation from the outermost
// pair of weights inwards).  One workgroup per BLUR_TILE x BLUR_TILE tile of a request's rectangle: the tile with a halo of the
// request's radius goes through the colour functor once per pixel into three uint8 planes in LDS, the vertical pass writes a
// second set of planes, the horizontal pass writes the scratch.  No global intermediate.
// 32 x 32, by measurement: at radius 8 a tile loads and colours (48 / 32)^2 = 2.25 x its pixels against 1.56 x at
// 64 x 64, but a step blurs a handful of footprints, and four times as many workgroups fill the device: 2.1 .. 2.9 x faster on
// the blurred crops of a step, 1.2 x with 32 windows at radius 8.  3 * 48 * 48 + 3 * 32 * 48 = 11520 bytes of LDS planes.
#define BLUR_TILE 32
#define BLUR_RMAX 8
#define BLUR_NW (2 * BLUR_RMAX + 1)

__device__ __forceinline__ int reflect_index(int p, int n) {
    const long long n2 = 2ll * n;
    long long m = p % n2;
    if (m < 0) m += n2;
    return (int)(m < n ? m : n2 - 1 - m);
}

template <int TILE>
__global__ void __launch_bounds__(NTHR) k_blur_pool_rects(
    const uint8_t *__restrict__ pool, const int64_t *__restrict__ px_off, const int32_t *__restrict__ hw, int nI, long long pool_px,
    const int32_t *__restrict__ image_of, const int32_t *__restrict__ rects, const int32_t *__restrict__ radius,
    const double *__restrict__ weights, const int64_t *__restrict__ scratch_off, int max_h, int max_w,
    const float *__restrict__ sigma, const float *__restrict__ bias, int simple_mode, const double *__restrict__ params,
    const double *__restrict__ density, const int32_t *__restrict__ mode, uint8_t *__restrict__ scratch, long long scratch_bytes,
    int32_t *__restrict__ status) {
    __shared__ double s_dens[256];
    __shared__ double s_w[BLUR_NW];
    constexpr int LD = TILE + 2 * BLUR_RMAX;
    __shared__ uint8_t s_in[3][LD][LD];
    __shared__ uint8_t s_mid[3][TILE][LD];
    const size_t t = blockIdx.y;
    const int tid = threadIdx.x;
    // everything below up to the first barrier is uniform over the workgroup
    const int y0 = rects[4 * t], x0 = rects[4 * t + 1], rh = rects[4 * t + 2], rw = rects[4 * t + 3], r = radius[t];
    const long long soff = scratch_off[t];
    const PoolSource src = pool_source(px_off, hw, nI, pool_px, image_of, t);
    const int sh = src.sh, sw = src.sw;
    int bad = src.bad;
    if (!bad && (y0 < 0 || x0 < 0 || rh <= 0 || rw <= 0 || rh > max_h || rw > max_w || (long long)y0 + rh > sh ||
                 (long long)x0 + rw > sw || r < 0 || r > BLUR_RMAX))
        bad = 4;
    if (!bad && (soff < 0 || soff > scratch_bytes || 3ll * rh * rw > scratch_bytes - soff)) bad = 8;
    if (bad) {                                                          // nothing is read or written for this request
        if (blockIdx.x == 0 && tid == 0) atomicOr(status, bad);
        return;
    }
    const int tiles_x = (rw + TILE - 1) / TILE, tiles_y = (rh + TILE - 1) / TILE;
    if ((int)blockIdx.x >= tiles_x * tiles_y) return;
    const int ty = blockIdx.x / tiles_x, tx = blockIdx.x - ty * tiles_x;
    const int oy = y0 + ty * TILE, ox = x0 + tx * TILE;      // the tile's first output pixel, in image coordinates
    const int th = min(TILE, y0 + rh - oy), tw = min(TILE, x0 + rw - ox);
    const int m = mode[t];
    s_dens[tid] = density[tid];
    if (tid < BLUR_NW) s_w[tid] = weights[t * BLUR_NW + tid];
    __syncthreads();
    const uint8_t *img = pool + 3 * src.off;
    const float *sg = sigma + t * 3, *bs = bias + t * 3;
    const double *par = params + t * HE_NPAR;
    // tile + halo through the colour functor, reflected about the image's borders
    const int lh = th + 2 * r, lw = tw + 2 * r;
    for (int i = tid; i < lh * lw; i += NTHR) {
        const int ly = i / lw, lx = i - ly * lw;
        const int gy = reflect_index(oy - r + ly, sh), gx = reflect_index(ox - r + lx, sw);
        uint8_t c[3];
        colour_pixel(img + ((long long)gy * sw + gx) * 3, m, sg, bs, simple_mode, par, s_dens, c);
        s_in[0][ly][lx] = c[0]; s_in[1][ly][lx] = c[1]; s_in[2][ly][lx] = c[2];
    }
    __syncthreads();
    // axis 0: output row ly of the tile is centred on loaded row ly + r
    for (int i = tid; i < 3 * th * lw; i += NTHR) {
        const int c = i / (th * lw), rem = i - c * (th * lw), ly = rem / lw, lx = rem - ly * lw;
        double acc = (double)s_in[c][ly + r][lx] * s_w[r];
        for (int k = r; k >= 1; --k) acc += ((double)s_in[c][ly + r - k][lx] + (double)s_in[c][ly + r + k][lx]) * s_w[r - k];
        s_mid[c][ly][lx] = (uint8_t)(int)acc;
    }
    __syncthreads();
    // axis 1, to the request's rectangle in the scratch
    uint8_t *dst = scratch + soff;
    for (int i = tid; i < th * tw * 3; i += NTHR) {
        const int c = i % 3, p = i / 3, ly = p / tw, lx = p - ly * tw;
        double acc = (double)s_mid[c][ly][lx + r] * s_w[r];
        for (int k = r; k >= 1; --k) acc += ((double)s_mid[c][ly][lx + r - k] + (double)s_mid[c][ly][lx + r + k]) * s_w[r - k];
        dst[((long long)(oy - y0 + ly) * rw + (ox - x0 + lx)) * 3 + c] = (uint8_t)(int)acc;
    }
}

#ifdef CPX_DEBUG
static int g_blur_tile = BLUR_TILE;
extern "C" void cpx_blur_set_tile(int tile) { g_blur_tile = tile == 64 ? 64 : BLUR_TILE; }
#endif

extern "C" int cpx_blur_pool_rects_u8(const uint8_t *pool_u8, const int64_t *px_off, const int32_t *hw, int nI, long long pool_px,
                                      const int32_t *image_of, const int32_t *rects, const int32_t *radius, const double *weights,
                                      const int64_t *scratch_off, int k, int max_h, int max_w, const float *sigma,
                                      const float *bias, int simple_mode, const double *stain_params, const double *density,
                                      const int32_t *mode, uint8_t *scratch, long long scratch_bytes, int32_t *status,
                                      void *stream) {
    CPX_REQUIRE(pool_u8 && px_off && hw && image_of && rects && radius && weights && scratch_off && scratch && status);
    CPX_REQUIRE(sigma && bias && stain_params && density && mode);
    CPX_REQUIRE(nI > 0 && pool_px > 0 && k > 0 && k <= 65535 && max_h > 0 && max_w > 0 && scratch_bytes > 0);
    int tile = BLUR_TILE;
#ifdef CPX_DEBUG
    tile = g_blur_tile;
#endif
    const long long tiles = (long long)cpx_cdiv(max_h, tile) * cpx_cdiv(max_w, tile);
    CPX_REQUIRE(tiles < (1ll << 31));
    hipStream_t s = (hipStream_t)stream;
    CPX_HIP(hipMemsetAsync(status, 0, sizeof(int32_t), s));
#ifdef CPX_DEBUG
    if (tile == 64)
        hipLaunchKernelGGL(k_blur_pool_rects<64>, dim3((unsigned)tiles, k), dim3(NTHR), 0, s, pool_u8, px_off, hw, nI, pool_px,
                           image_of, rects, radius, weights, scratch_off, max_h, max_w, sigma, bias, simple_mode ? 1 : 0, stain_params,
                           density, mode, scratch, scratch_bytes, status);
    else
#endif
    hipLaunchKernelGGL(k_blur_pool_rects<BLUR_TILE>, dim3((unsigned)tiles, k), dim3(NTHR), 0, s, pool_u8, px_off, hw, nI, pool_px,
                       image_of, rects, radius, weights, scratch_off, max_h, max_w, sigma, bias, simple_mode ? 1 : 0, stain_params,
                       density, mode, scratch, scratch_bytes, status);
    CPX_CHECK_LAUNCH();
    return CPX_OK;
}

// the taps of cpx_warp_affine_pool_quality_u8: the shared colour tap, or the bytes of the crop's blurred rectangle in the scratch in
// its place, then hbs_pixel where the crop's flag is set.  A tap inside the image that the rectangle does not cover is 0, sets
// status bit 4 and reads nothing.
struct QualityTaps {
    ColourTaps colour;
    const float *hbs, *unit;
    const int32_t *hbs_apply;
    const uint8_t *scratch;
    long long scratch_bytes;
    const int64_t *ov_off;
    const int32_t *ov_rect;
    int32_t *status;
    __device__ __forceinline__ bool scratch_tap(size_t t, int sh, int sw, int y, int x, long long so, uint8_t *r) const {
        r[0] = r[1] = r[2] = 0;
        if (!tap_inside(sh, sw, y, x)) return false;
        const int *rc = ov_rect + 4 * t;
        const int ry = y - rc[0], rx = x - rc[1];
        if ((unsigned)ry >= (unsigned)rc[2] || (unsigned)rx >= (unsigned)rc[3]) { atomicOr(status, 16); return false; }
        const uint8_t *px = scratch + so + ((long long)ry * rc[3] + rx) * 3;
        r[0] = px[0]; r[1] = px[1]; r[2] = px[2];
        return true;
    }
    __device__ __forceinline__ void tap(size_t t, const uint8_t *img, int sh, int sw, int y, int x, long long so, int do_hbs,
                                        float *v) const {
        uint8_t r[3];
        const bool in = so >= 0 ? scratch_tap(t, sh, sw, y, x, so, r) : colour.bytes(colour.m, t, img, sh, sw, y, x, r);
        if (in && do_hbs) hbs_pixel(r, hbs + t * 4, unit, r);
        v[0] = (float)r[0]; v[1] = (float)r[1]; v[2] = (float)r[2];
    }
    __device__ __forceinline__ void operator()(size_t t, const uint8_t *img, int sh, int sw, int y0, int x0, float *a, float *b,
                                               float *d, float *e) const {
        const int do_hbs = hbs_apply[t];
        long long so = ov_off[t];
        if (so >= 0) {                                                  // a range outside the scratch is never read
            const int *rc = ov_rect + 4 * t;
            if (rc[2] <= 0 || rc[3] <= 0 || so > scratch_bytes || 3ll * rc[2] * rc[3] > scratch_bytes - so) {
                atomicOr(status, 8);
                a[0] = a[1] = a[2] = b[0] = b[1] = b[2] = d[0] = d[1] = d[2] = e[0] = e[1] = e[2] = 0.f;
                return;
            }
        }
        tap(t, img, sh, sw, y0, x0, so, do_hbs, a);
        tap(t, img, sh, sw, y0, x0 + 1, so, do_hbs, b);
        tap(t, img, sh, sw, y0 + 1, x0, so, do_hbs, d);
        tap(t, img, sh, sw, y0 + 1, x0 + 1, so, do_hbs, e);
    }
};

__global__ void __launch_bounds__(NTHR) k_warp_affine_pool_quality(
    const uint8_t *__restrict__ pool, const int16_t *__restrict__ pool_lab, const int64_t *__restrict__ px_off,
    const int32_t *__restrict__ hw, int nI, long long pool_px, const int32_t *__restrict__ image_of, const double *__restrict__ inv,
    const float *__restrict__ sigma, const float *__restrict__ bias, int simple_mode, const double *__restrict__ params,
    const double *__restrict__ density, const int32_t *__restrict__ mode, const float *__restrict__ hbs,
    const int32_t *__restrict__ hbs_apply, const float *__restrict__ unit, const uint8_t *__restrict__ scratch,
    long long scratch_bytes, const int64_t *__restrict__ ov_off, const int32_t *__restrict__ ov_rect, int dh, int dw, int label_fill,
    float *__restrict__ out, int16_t *__restrict__ lab_out, int32_t *__restrict__ status) {
    __shared__ double s_dens[256];
    __shared__ float s_unit[256];
    s_dens[threadIdx.x] = density[threadIdx.x];
    s_unit[threadIdx.x] = unit[threadIdx.x];
    __syncthreads();
    warp_pool_pixel(pool, pool_lab, px_off, hw, nI, pool_px, image_of, inv, dh, dw, label_fill, out, lab_out, status,
                    QualityTaps{ColourTaps{mode[blockIdx.y], sigma, bias, simple_mode, params, s_dens}, hbs, s_unit, hbs_apply, scratch,
                                scratch_bytes, ov_off, ov_rect, status});
}

extern "C" int cpx_warp_affine_pool_quality_u8(const uint8_t *pool_u8, const int16_t *pool_lab, const int64_t *px_off,
                                               const int32_t *hw, int nI, long long pool_px, const int32_t *image_of,
                                               const double *inv, int n, const float *sigma, const float *bias, int simple_mode,
                                               const double *stain_params, const double *density, const int32_t *mode,
                                               const float *hbs, const int32_t *hbs_apply, const float *unit, const uint8_t *scratch,
                                               long long scratch_bytes, const int64_t *override_off, const int32_t *override_rect,
                                               int dh, int dw, int label_fill, float *out, int16_t *labels_out, int32_t *status,
                                               void *stream) {
    hipStream_t s = (hipStream_t)stream;
    CPX_REQUIRE(sigma && bias && stain_params && density && mode && hbs && hbs_apply && unit && override_off && override_rect);
    CPX_REQUIRE(scratch_bytes >= 0 && (scratch != nullptr || scratch_bytes == 0));
    if (int rc = pool_warp_require(pool_u8, pool_lab, px_off, hw, nI, pool_px, image_of, inv, n, dh, dw, label_fill, out, labels_out,
                                   status, s))
        return rc;
    hipLaunchKernelGGL(k_warp_affine_pool_quality, dim3(cpx_cdiv((long long)dh * dw, NTHR), n), dim3(NTHR), 0, s, pool_u8, pool_lab,
                       px_off, hw, nI, pool_px, image_of, inv, sigma, bias, simple_mode ? 1 : 0, stain_params, density, mode, hbs,
                       hbs_apply, unit, scratch, scratch_bytes, override_off, override_rect, dh, dw, label_fill, out, labels_out,
                       status);
    CPX_CHECK_LAUNCH();
    return CPX_OK;
}
