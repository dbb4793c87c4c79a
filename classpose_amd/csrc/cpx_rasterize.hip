// r1: polygon rings -> instance-id maps on the device, the inverse of the polygoniser (cpx_polygons.hip).
//
// The reference paints annotations on the host, ring by ring, with skimage.draw.polygon (paper_experiments/scripts/
// organise-datasets.py:626-652: instance id = 1-based feature index, every ring of a feature painted, later features over
// earlier ones).  Here every ring is painted by its own wave or workgroups, and `inst[p] = max(inst[p], value)` by an integer
// atomic max replaces the painter's order: ids rise in feature order, so the later feature wins whatever the scheduling.
//
// THE RULE (include/classpose_hip.h; tests/rasterize_reference.py states it on the CPU):
//   pixel (r, c) has its centre at x = c, y = r; a ring paints it when the centre lies ON the ring (an edge or a vertex) or has an
//   odd crossing number (even-odd rule, an edge (x0, y0) -> (x1, y1) counts when min(y0, y1) <= y < max(y0, y1) and the centre is
//   strictly left of it).  One predicate decides both, in float64, contraction off, in this operand order:
//       d = (x1 - x0) * (py - y0) - (y1 - y0) * (px - x0)
//   on the edge:  d == 0 and min(x0, x1) <= px <= max(x0, x1) and min(y0, y1) <= py <= max(y0, y1)
//   crossing:     (y0 <= py < y1 and d > 0) or (y1 <= py < y0 and d < 0)
//   A closing vertex equal to the first is dropped; fewer than three vertices after that paint nothing.
//
//   k_rast_small  one wave per ring: bounding box by a wave reduction (double, clamped to the image BEFORE the conversion to
//                 int).  A ring of at most RS_SMALL_VERTS vertices and RS_SMALL_AREA box pixels is painted here: vertices staged
//                 in LDS, lanes stride the pixels of the box, every pixel tests every edge.  Any other ring gets a descriptor in
//                 the workspace (the slot comes from an integer counter: the ORDER of the list depends on scheduling, the maps
//                 do not).
//   k_rast_large  a workgroup per (listed ring, band of RL_BAND rows).  Per row and per chunk of RL_CHUNK edges, in order: the
//                 edges whose closed y range holds the row are compacted into LDS by ballot and prefix, in edge order; then each
//                 pixel of the row is tested against that short list only.  Parity and the on-ring flag are carried per pixel
//                 (one byte in LDS) from chunk to chunk, so the result does not depend on the chunking.
//
// Integer atomics only, no spin loops; every loop is bounded by a count fixed when its kernel starts; every store is bounds-checked;
// pixel indexing is 64-bit.
#include "cpx_common.h"

#pragma clang fp contract(off)

#define RS_THR 256                        // threads per workgroup, both kernels
#define RS_WAVES (RS_THR / 64)
#define RS_SMALL_VERTS 256                // small path: at most this many vertices (after the closing vertex is dropped) ...
#define RS_SMALL_AREA 4096                // ... and at most this many pixels in the clipped bounding box
#define RL_CHUNK 512                      // large path: edges compacted per pass
#define RL_SUB (RL_CHUNK / RS_THR)
#define RL_BAND 8                         // large path: rows per work item
#define RL_GRID_X 64                      // large path: workgroups striding the bands of one ring
#define RL_GRID_Y 32                      // large path: workgroups striding the listed rings
#define RS_MAX_DIM 32768                  // H, W limit: the per-pixel state of one row is RS_MAX_DIM bytes of LDS
#define RS_MAX_VERTS (1 << 30)

struct RsRing {                           // a ring the small kernel left to the large one
    int ring, n;                          // n: vertices after the closing vertex is dropped
    int c0, c1, r0, r1;                   // clipped bounding box, inclusive
    int pad0, pad1;
};

struct RsArgs {
    const double *xy;
    const long long *ring_off;
    const int *ring_value, *ring_image;
    long long n_rings;
    int n_images, H, W;
    int *inst;
    unsigned *n_large;                    // workspace: counter, then the list
    RsRing *large;
};

// parity (bit 0) and on-ring flag (bit 1) of centre (px, py) against one edge
__device__ __forceinline__ unsigned rs_edge(double x0, double y0, double x1, double y1, double px, double py) {
    const double d = (x1 - x0) * (py - y0) - (y1 - y0) * (px - x0);
    unsigned s = 0;
    if ((y0 <= py && py < y1 && d > 0.0) || (y1 <= py && py < y0 && d < 0.0)) s = 1u;
    if (d == 0.0 && fmin(x0, x1) <= px && px <= fmax(x0, x1) && fmin(y0, y1) <= py && py <= fmax(y0, y1)) s |= 2u;
    return s;
}

__device__ __forceinline__ double rs_wave_min(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmin(v, __shfl_xor(v, o));
    return v;
}
__device__ __forceinline__ double rs_wave_max(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmax(v, __shfl_xor(v, o));
    return v;
}

__device__ __forceinline__ void rs_paint(const RsArgs &a, int img, int r, int c, int value) {
    if (r < 0 || r >= a.H || c < 0 || c >= a.W || img < 0 || img >= a.n_images) return;
    atomicMax(&a.inst[((size_t)img * a.H + (size_t)r) * a.W + (size_t)c], value);
}

__global__ void __launch_bounds__(RS_THR) k_rast_small(RsArgs a) {
    __shared__ double s_x[RS_WAVES][RS_SMALL_VERTS + 1], s_y[RS_WAVES][RS_SMALL_VERTS + 1];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long long ring = (long long)blockIdx.x * RS_WAVES + wave;
    if (ring >= a.n_rings) return;                                   // wave-uniform: no barrier below
    const int value = a.ring_value[ring];
    const int img = a.ring_image ? a.ring_image[ring] : 0;
    const long long o0 = a.ring_off[ring], cnt = a.ring_off[ring + 1] - o0;
    if (value <= 0 || img < 0 || img >= a.n_images || o0 < 0 || cnt < 3 || cnt > RS_MAX_VERTS) return;
    const double *v = a.xy + 2 * o0;
    int n = (int)cnt;
    if (v[0] == v[2 * (n - 1)] && v[1] == v[2 * (n - 1) + 1]) --n;  // the closing vertex
    if (n < 3) return;
    double lox = INFINITY, hix = -INFINITY, loy = INFINITY, hiy = -INFINITY;
    for (int i = lane; i < n; i += 64) {
        const double x = v[2 * i], y = v[2 * i + 1];
        lox = fmin(lox, x); hix = fmax(hix, x); loy = fmin(loy, y); hiy = fmax(hiy, y);
    }
    lox = rs_wave_min(lox); loy = rs_wave_min(loy); hix = rs_wave_max(hix); hiy = rs_wave_max(hiy);
    // clamped in double first: the conversions below see values in [-1, 32768] whatever the vertices are
    const int c0 = (int)ceil(fmin(fmax(lox, 0.0), (double)a.W)), c1 = (int)floor(fmin(fmax(hix, -1.0), (double)(a.W - 1)));
    const int r0 = (int)ceil(fmin(fmax(loy, 0.0), (double)a.H)), r1 = (int)floor(fmin(fmax(hiy, -1.0), (double)(a.H - 1)));
    if (c0 > c1 || r0 > r1) return;                                  // no pixel centre inside the box
    const int bw = c1 - c0 + 1, bh = r1 - r0 + 1;
    const long long area = (long long)bw * bh;
    if (n > RS_SMALL_VERTS || area > RS_SMALL_AREA) {
        if (lane == 0) {
            const unsigned slot = atomicAdd(a.n_large, 1u);
            if ((long long)slot < a.n_rings) {
                RsRing d;
                d.ring = (int)ring; d.n = n; d.c0 = c0; d.c1 = c1; d.r0 = r0; d.r1 = r1; d.pad0 = d.pad1 = 0;
                a.large[slot] = d;
            }
        }
        return;
    }
    double *sx = s_x[wave], *sy = s_y[wave];
    for (int i = lane; i < n; i += 64) { sx[i] = v[2 * i]; sy[i] = v[2 * i + 1]; }
    if (lane == 0) { sx[n] = v[0]; sy[n] = v[1]; }
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    for (int p = lane; p < (int)area; p += 64) {
        const int r = r0 + p / bw, c = c0 + p % bw;
        const double px = (double)c, py = (double)r;
        unsigned st = 0;
        for (int e = 0; e < n; ++e) {
            const unsigned s = rs_edge(sx[e], sy[e], sx[e + 1], sy[e + 1], px, py);
            st = (st ^ (s & 1u)) | (s & 2u);
        }
        if (st) rs_paint(a, img, r, c, value);
    }
}

__global__ void __launch_bounds__(RS_THR) k_rast_large(RsArgs a) {
    __shared__ double s_x0[RL_CHUNK], s_y0[RL_CHUNK], s_x1[RL_CHUNK], s_y1[RL_CHUNK];
    __shared__ unsigned char s_state[RS_MAX_DIM];
    __shared__ int s_wcnt[RL_SUB][RS_WAVES];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const long long listed = min((long long)*a.n_large, a.n_rings);
    for (long long li = blockIdx.y; li < listed; li += gridDim.y) {
        const RsRing d = a.large[li];
        const int value = a.ring_value[d.ring];
        const int img = a.ring_image ? a.ring_image[d.ring] : 0;
        const double *v = a.xy + 2 * a.ring_off[d.ring];
        const int n = d.n, bw = d.c1 - d.c0 + 1;
        if (bw < 1 || bw > RS_MAX_DIM || n < 3) continue;            // uniform over the workgroup
        const int n_bands = (d.r1 - d.r0 + RL_BAND) / RL_BAND;
        for (int band = blockIdx.x; band < n_bands; band += gridDim.x) {
            const int rb = d.r0 + band * RL_BAND, re = min(rb + RL_BAND - 1, d.r1);
            for (int r = rb; r <= re; ++r) {
                const double py = (double)r;
                for (int j = tid; j < bw; j += RS_THR) s_state[j] = 0;   // a pixel's byte is only ever touched by its owner
                for (int e0 = 0; e0 < n; e0 += RL_CHUNK) {
                    double ex0[RL_SUB], ey0[RL_SUB], ex1[RL_SUB], ey1[RL_SUB];
                    int pre[RL_SUB];
                    bool take[RL_SUB];
#pragma unroll
                    for (int s = 0; s < RL_SUB; ++s) {
                        const int e = e0 + s * RS_THR + tid;
                        take[s] = false;
                        if (e < n) {
                            const int e1 = e + 1 == n ? 0 : e + 1;
                            ex0[s] = v[2 * e]; ey0[s] = v[2 * e + 1]; ex1[s] = v[2 * e1]; ey1[s] = v[2 * e1 + 1];
                            take[s] = fmin(ey0[s], ey1[s]) <= py && py <= fmax(ey0[s], ey1[s]);
                        }
                        const unsigned long long m = __ballot(take[s]);
                        pre[s] = __popcll(m & ((1ULL << lane) - 1ULL));
                        if (lane == 0) s_wcnt[s][wave] = __popcll(m);
                    }
                    __syncthreads();
                    int total = 0;
#pragma unroll
                    for (int s = 0; s < RL_SUB; ++s) {
#pragma unroll
                        for (int w = 0; w < RS_WAVES; ++w) {
                            if (w == wave && take[s]) {
                                const int q = total + pre[s];            // < RL_CHUNK: one slot per edge of the chunk at most
                                s_x0[q] = ex0[s]; s_y0[q] = ey0[s]; s_x1[q] = ex1[s]; s_y1[q] = ey1[s];
                            }
                            total += s_wcnt[s][w];
                        }
                    }
                    __syncthreads();
                    if (total) {
                        for (int j = tid; j < bw; j += RS_THR) {
                            const double px = (double)(d.c0 + j);
                            unsigned st = s_state[j];
                            for (int q = 0; q < total; ++q) {
                                const unsigned s = rs_edge(s_x0[q], s_y0[q], s_x1[q], s_y1[q], px, py);
                                st = (st ^ (s & 1u)) | (s & 2u);
                            }
                            s_state[j] = (unsigned char)st;
                        }
                    }
                    __syncthreads();                                     // the list and the counts are rewritten by the next chunk
                }
                for (int j = tid; j < bw; j += RS_THR)
                    if (s_state[j]) rs_paint(a, img, r, d.c0 + j, value);
            }
        }
    }
}

__global__ void __launch_bounds__(RS_THR) k_ids_to_classes(const int *inst, long long n_px, const unsigned char *class_of, int n_ids,
                                                          unsigned char *cls) {
    const long long step = (long long)gridDim.x * RS_THR;
    for (long long p = (long long)blockIdx.x * RS_THR + threadIdx.x; p < n_px; p += step) {
        const int id = inst[p];
        cls[p] = (id >= 0 && id <= n_ids) ? class_of[id] : (unsigned char)0;
    }
}

static bool rs_args_ok(long long n_rings, int n_images, int H, int W) {
    return n_rings >= 0 && n_rings <= 0x7fffffffLL - RS_WAVES && n_images >= 1 && H >= 1 && W >= 1 && H <= RS_MAX_DIM && W <= RS_MAX_DIM;
}

#define RS_LIST_OFF 256                   // the counter has the first 256 bytes of the workspace to itself

extern "C" size_t cpx_rasterize_workspace_bytes(long long n_rings, long long n_vertices, int n_images, int H, int W) {
    if (!rs_args_ok(n_rings, n_images, H, W) || n_vertices < 0) return 0;
    return RS_LIST_OFF + cpx_align_up((size_t)n_rings * sizeof(RsRing), 256);
}

extern "C" int cpx_rasterize_polygons(const double *xy, const long long *ring_off, const int *ring_value, const int *ring_image,
                                      long long n_rings, int n_images, int H, int W, int *inst, void *workspace,
                                      size_t workspace_bytes, void *stream) {
    CPX_REQUIRE(rs_args_ok(n_rings, n_images, H, W));
    CPX_REQUIRE(inst != nullptr);
    if (n_rings == 0) return CPX_OK;
    CPX_REQUIRE(xy && ring_off && ring_value && workspace);
    CPX_REQUIRE(((uintptr_t)workspace & 15) == 0);
    CPX_REQUIRE(workspace_bytes >= RS_LIST_OFF + (size_t)n_rings * sizeof(RsRing));
    hipStream_t s = (hipStream_t)stream;
    CPX_HIP(hipMemsetAsync(workspace, 0, RS_LIST_OFF, s));
    RsArgs a;
    a.xy = xy; a.ring_off = ring_off; a.ring_value = ring_value; a.ring_image = ring_image;
    a.n_rings = n_rings; a.n_images = n_images; a.H = H; a.W = W; a.inst = inst;
    a.n_large = reinterpret_cast<unsigned *>(workspace);
    a.large = reinterpret_cast<RsRing *>((char *)workspace + RS_LIST_OFF);
    hipLaunchKernelGGL(k_rast_small, dim3(cpx_cdiv(n_rings, RS_WAVES)), dim3(RS_THR), 0, s, a);
    hipLaunchKernelGGL(k_rast_large, dim3(RL_GRID_X, (unsigned)(n_rings < RL_GRID_Y ? n_rings : RL_GRID_Y)), dim3(RS_THR), 0, s, a);
    CPX_CHECK_LAUNCH();
    return CPX_OK;
}

extern "C" int cpx_ids_to_classes(const int *inst, long long n_px, const unsigned char *class_of, int n_ids, unsigned char *cls,
                                  void *stream) {
    CPX_REQUIRE(n_px >= 0 && n_ids >= 0);
    if (n_px == 0) return CPX_OK;
    CPX_REQUIRE(inst && class_of && cls);
    const long long blocks = (n_px + RS_THR - 1) / RS_THR;
    hipLaunchKernelGGL(k_ids_to_classes, dim3((unsigned)(blocks < 65536 ? blocks : 65536)), dim3(RS_THR), 0, (hipStream_t)stream,
                       inst, n_px, class_of, n_ids, cls);
    CPX_CHECK_LAUNCH();
    return CPX_OK;
}
