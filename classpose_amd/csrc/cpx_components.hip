// r2: connected-component labelling of int32 value maps on the device: class maps -> instance maps without a host pass.
//
// The reference labels on the host: `ndimage.label` per class (paper_experiments/run_cellpose_semantic.py:89-100) and
// `skimage.measure.label` inside get_instance_counts(label_instances=True) (train_utils.py:407-436).  The rule (include/
// classpose_hip.h, r2): 0 is background, two neighbouring pixels of the same non-zero value are connected (4 or 8 neighbours), a
// component's label is its 1-based rank by the raster index of its first pixel, per image.
//
// Every pixel has a parent, an in-image raster index that is never larger than its own; a pixel that is its own parent is a
// root.  Parents only ever decrease (integer atomic minima), and a union always hangs the larger root under the smaller one, so
// the root of a finished component is its smallest index: its raster-first pixel, whatever the order of the unions.
//
//   k_cc_tile     a workgroup labels one 64 x 64 tile in LDS.  A thread owns 16 consecutive pixels of one row: it first gives
//                 every pixel the start of its run (no atomics), then joins runs across its strip's left edge and to the row
//                 above by union-find in LDS; a join to the pixel above is skipped where the pixels to the left of both already
//                 make it.  Every pixel is then flattened to its tile root, written as an in-image index to `labels` (kept to
//                 the end: the pixel's tile root) and to the global parents.
//   k_cc_seams    one thread per pixel of a tile's first row or first column: unions across the seam on the global parents,
//                 agent-scope atomic loads and minima (workgroups on other XCDs write the same words concurrently).
//   k_cc_roots    every tile root finds its final root and stores it as its parent (so the last pass needs no loop); the
//                 roots that are their own -- the components -- are counted per block of 4096 pixels.
//   k_cc_offsets  one workgroup per image: exclusive scan of the block counts, the image's total -> n_components.
//   k_cc_rank     per block: the roots' ranks in raster order (ballot scan), stored in place of the root's parent as -(rank + 1).
//   k_cc_relabel  labels[p] = rank of the root of the tile root of p.
//
// Launch boundaries are the only device-wide synchronisation: no workgroup ever waits for another.  Integer atomics only; the
// outputs are functions of the map alone.
#include "cpx_common.h"

#define CC_TILE 64                                // tile side
#define CC_THR 256
#define CC_STRIP 16                               // consecutive pixels of one tile row per thread: CC_TILE * CC_TILE / CC_THR
#define CC_TILE_PX 4096                           // CC_TILE * CC_TILE
#define CC_BLOCK 4096                             // pixels per workgroup of the counting and ranking passes: CC_THR * 16
#define CC_MAX_PX 268435456                       // 2^28 pixels per image
// pixel l of the tile sits at l + l / 16 in LDS: a thread's strip starts at 17 * tid, so the lanes of a wave spread over the banks
#define CC_IDX(l) ((l) + ((l) >> 4))

static_assert(CC_TILE * CC_TILE == CC_TILE_PX && CC_THR * CC_STRIP == CC_TILE_PX && CC_TILE % CC_STRIP == 0, "tile geometry");
static_assert(CC_BLOCK % CC_THR == 0 && CC_THR == 256, "block geometry (cpx_block_scan256)");

struct CcArgs {
    const int32_t *map;
    int32_t *labels, *parent, *sums, *n_components;
    int n, H, W, HW, tilesX, tilesY, nblk, conn8;
};

// ---- union-find in LDS (workgroup scope) ----------------------------------------------------------------------------------------
__device__ __forceinline__ int cc_find_lds(const int *par, int x) {
    // terminates: the loop goes on only to a parent STRICTLY below x (a parent is never above its pixel), and x >= 0
    for (;;) {
        const int p = __hip_atomic_load(&par[CC_IDX(x)], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        if (p >= x || p < 0) return x;
        x = p;
    }
}
__device__ __forceinline__ void cc_union_lds(int *par, int a, int b) {
    // terminates: a turn that does not return replaces a by `old`, strictly below the root a it displaced, and find never
    // goes up: a + b strictly decreases from turn to turn and both stay >= 0.
    // correct: when a is no longer a root the minimum may have replaced its link to `old` by one to b; joining old and b next
    // restores what was lost.
    for (;;) {
        a = cc_find_lds(par, a); b = cc_find_lds(par, b);
        if (a == b) return;
        if (a < b) { const int t = a; a = b; b = t; }
        const int old = __hip_atomic_fetch_min(&par[CC_IDX(a)], b, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        if (old >= a || old < 0) return;                     // a was a root: joined
        a = old;
    }
}

// ---- the same on the global parents of one image (agent scope) ------------------------------------------------------------------
__device__ __forceinline__ int cc_find(const int32_t *par, int x) {
    // terminates: as cc_find_lds -- x strictly decreases and stays >= 0
    for (;;) {
        const int p = __hip_atomic_load(&par[x], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (p >= x || p < 0) return x;
        x = p;
    }
}
__device__ __forceinline__ void cc_union(int32_t *par, int a, int b) {
    // terminates and is correct as cc_union_lds: a + b strictly decreases, both >= 0
    for (;;) {
        a = cc_find(par, a); b = cc_find(par, b);
        if (a == b) return;
        if (a < b) { const int t = a; a = b; b = t; }
        const int old = __hip_atomic_fetch_min(&par[a], b, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (old >= a || old < 0) return;
        a = old;
    }
}

__global__ void __launch_bounds__(CC_THR) k_cc_tile(CcArgs a) {
    __shared__ int s_val[CC_TILE_PX + CC_TILE_PX / 16];
    __shared__ int s_par[CC_TILE_PX + CC_TILE_PX / 16];
    const int tid = threadIdx.x, img = blockIdx.y;
    const int y0 = ((int)blockIdx.x / a.tilesX) * CC_TILE, x0 = ((int)blockIdx.x % a.tilesX) * CC_TILE;
    const size_t base = (size_t)img * a.HW;
    const int32_t *m = a.map + base;
    for (int l = tid; l < CC_TILE_PX; l += CC_THR) {
        const int y = y0 + l / CC_TILE, x = x0 + l % CC_TILE;
        s_val[CC_IDX(l)] = (y < a.H && x < a.W) ? m[y * a.W + x] : 0;       // outside the image: background
    }
    __syncthreads();
    const int ly = tid / (CC_TILE / CC_STRIP), sx = (tid % (CC_TILE / CC_STRIP)) * CC_STRIP, l0 = ly * CC_TILE + sx;
    int prev = 0, run = l0;
#pragma unroll
    for (int k = 0; k < CC_STRIP; ++k) {                                    // runs of equal value inside the strip
        const int l = l0 + k, v = s_val[CC_IDX(l)];
        if (v != prev) run = l;
        s_par[CC_IDX(l)] = v ? run : -1;
        prev = v;
    }
    __syncthreads();
    for (int k = 0; k < CC_STRIP; ++k) {
        const int l = l0 + k, lx = sx + k, v = s_val[CC_IDX(l)];
        if (!v) continue;
        const bool west = lx > 0 && s_val[CC_IDX(l - 1)] == v;
        if (k == 0 && west) cc_union_lds(s_par, l, l - 1);                  // the run goes on in the strip to the left
        if (ly == 0) continue;
        const int up = l - CC_TILE;
        if (s_val[CC_IDX(up)] == v) {
            // west of both the same value too: (l - 1, up - 1) are joined by their own turn and each row by its runs
            if (!(west && s_val[CC_IDX(up - 1)] == v)) cc_union_lds(s_par, l, up);
        } else if (a.conn8) {                                               // with `up` in the component both corners hang on it
            if (lx > 0 && s_val[CC_IDX(up - 1)] == v) cc_union_lds(s_par, l, up - 1);
            if (lx < CC_TILE - 1 && s_val[CC_IDX(up + 1)] == v) cc_union_lds(s_par, l, up + 1);
        }
    }
    __syncthreads();
    for (int l = tid; l < CC_TILE_PX; l += CC_THR) {
        const int y = y0 + l / CC_TILE, x = x0 + l % CC_TILE;
        if (y >= a.H || x >= a.W) continue;
        int g = -1;
        if (s_val[CC_IDX(l)]) {
            const int r = cc_find_lds(s_par, l);                            // the tile's raster order is the image's
            g = (y0 + r / CC_TILE) * a.W + x0 + r % CC_TILE;
        }
        a.labels[base + y * a.W + x] = g;
        a.parent[base + y * a.W + x] = g;
    }
}

// items of one image: (tilesY - 1) * W pixels on the first row of a tile row, then (tilesX - 1) * H on the first column of a tile column
__global__ void __launch_bounds__(CC_THR) k_cc_seams(CcArgs a) {
    const int i = blockIdx.x * CC_THR + threadIdx.x, img = blockIdx.y;
    const int n_row = (a.tilesY - 1) * a.W, n_col = (a.tilesX - 1) * a.H, W = a.W;
    if (i >= n_row + n_col) return;
    const size_t base = (size_t)img * a.HW;
    const int32_t *m = a.map + base;
    int32_t *par = a.parent + base;
    if (i < n_row) {
        const int y = (i / W + 1) * CC_TILE, x = i % W, p = y * W + x, q = p - W;
        const int v = m[p];
        if (!v) return;
        if (m[q] == v) {
            // inside a tile column the pixels to the west, when of the same value, make the join (as in k_cc_tile)
            if (!(x % CC_TILE != 0 && m[p - 1] == v && m[q - 1] == v)) cc_union(par, p, q);
        } else if (a.conn8) {
            if (x > 0 && m[q - 1] == v) cc_union(par, p, q - 1);
            if (x < W - 1 && m[q + 1] == v) cc_union(par, p, q + 1);
        }
    } else {
        const int j = i - n_row;
        const int x = (j / a.H + 1) * CC_TILE, y = j % a.H, p = y * W + x;
        const int v = m[p], w = m[p - 1];
        if (v && w == v) cc_union(par, p, p - 1);
        if (a.conn8 && y > 0) {
            const int up = m[p - W], upw = m[p - W - 1];
            // each corner pair matters only when the pixel between them (above p, or above p - 1) is not of their value
            if (v && upw == v && up != v) cc_union(par, p, p - W - 1);
            if (w && up == w && upw != w) cc_union(par, p - 1, p - W);
        }
    }
}

__global__ void __launch_bounds__(CC_THR) k_cc_roots(CcArgs a) {
    __shared__ int s_cnt;
    const int tid = threadIdx.x, img = blockIdx.y;
    const size_t base = (size_t)img * a.HW;
    int32_t *par = a.parent + base;
    const int32_t *lab = a.labels + base;
    if (tid == 0) s_cnt = 0;
    __syncthreads();
    int cnt = 0;
    for (int j = 0; j < CC_BLOCK / CC_THR; ++j) {
        const int p = blockIdx.x * CC_BLOCK + j * CC_THR + tid;
        if (p >= a.HW || lab[p] != p) continue;                             // tile roots only: nothing else was ever joined
        const int r = cc_find(par, p);
        if (r == p) ++cnt;
        // r is an ancestor of p whenever it is read: a concurrent find through p ends at the same root either way
        else __hip_atomic_store(&par[p], r, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    if (cnt) atomicAdd(&s_cnt, cnt);
    __syncthreads();
    if (tid == 0) a.sums[(size_t)img * a.nblk + blockIdx.x] = s_cnt;
}

__global__ void __launch_bounds__(CC_THR) k_cc_offsets(CcArgs a) {           // one workgroup per image: the scan stays inside it
    __shared__ int s_w[CC_THR / 64];
    const int tid = threadIdx.x, img = blockIdx.x;
    int32_t *sums = a.sums + (size_t)img * a.nblk;
    int carry = 0;
    for (int c0 = 0; c0 < a.nblk; c0 += CC_THR) {
        const int i = c0 + tid, v = i < a.nblk ? sums[i] : 0;
        int tot;
        const int incl = cpx_block_scan256(v, s_w, &tot);
        if (i < a.nblk) sums[i] = carry + incl - v;
        carry += tot;
    }
    if (tid == 0) a.n_components[img] = carry;
}

__global__ void __launch_bounds__(CC_THR) k_cc_rank(CcArgs a) {
    __shared__ int s_w[CC_THR / 64];
    const int tid = threadIdx.x, img = blockIdx.y;
    int32_t *par = a.parent + (size_t)img * a.HW;
    int running = a.sums[(size_t)img * a.nblk + blockIdx.x];
    for (int j = 0; j < CC_BLOCK / CC_THR; ++j) {
        const int p = blockIdx.x * CC_BLOCK + j * CC_THR + tid;
        const int flag = (p < a.HW && par[p] == p) ? 1 : 0;                  // its own parent: a component's first pixel
        int tot;
        const int incl = cpx_block_scan256(flag, s_w, &tot);
        if (flag) par[p] = -(running + incl);                               // 1-based rank, negated: no parent is negative
        running += tot;
    }
}

__global__ void __launch_bounds__(CC_THR) k_cc_relabel(CcArgs a) {
    const int p = blockIdx.x * CC_THR + threadIdx.x, img = blockIdx.y;
    if (p >= a.HW) return;
    const size_t base = (size_t)img * a.HW;
    const int32_t *par = a.parent + base;
    const int t = a.labels[base + p];                                       // the tile root, or -1 on background
    int v = 0;
    if (t >= 0) {
        v = par[t];                                                         // its root (k_cc_roots), or its own rank
        if (v >= 0) v = par[v];
    }
    a.labels[base + p] = -v;
}

struct CcLayout { size_t parent, sums, total; };

static bool cc_args_ok(int n, int H, int W) {
    return n >= 1 && n <= 65535 && H >= 1 && W >= 1 && (long long)H * W <= CC_MAX_PX;
}

static CcLayout cc_layout(int n, int H, int W) {
    CcLayout L; CpxArena a;
    const size_t HW = (size_t)H * W;
    L.parent = a.take((size_t)n * HW * 4);
    L.sums = a.take((size_t)n * cpx_cdiv((long long)HW, CC_BLOCK) * 4);
    L.total = a.o;
    return L;
}

extern "C" size_t cpx_label_components_workspace_bytes(int n, int H, int W) {
    if (!cc_args_ok(n, H, W)) return 0;
    return cc_layout(n, H, W).total;
}

extern "C" int cpx_label_components(const int32_t *map, int n, int H, int W, int connectivity, int32_t *labels,
                                    int32_t *n_components, void *workspace, size_t workspace_bytes, void *stream) {
    CPX_REQUIRE(connectivity == 4 || connectivity == 8);
    if (n == 0) return CPX_OK;
    CPX_REQUIRE(cc_args_ok(n, H, W));
    const CcLayout L = cc_layout(n, H, W);
    CPX_REQUIRE(workspace_bytes >= L.total);
    CPX_REQUIRE(map && labels && n_components && workspace);
    CPX_REQUIRE((const void *)labels != (const void *)map);
    hipStream_t s = (hipStream_t)stream;
    CcArgs a;
    a.map = map; a.labels = labels; a.n_components = n_components;
    a.parent = reinterpret_cast<int32_t *>((char *)workspace + L.parent);
    a.sums = reinterpret_cast<int32_t *>((char *)workspace + L.sums);
    a.n = n; a.H = H; a.W = W; a.HW = H * W;
    a.tilesX = cpx_cdiv(W, CC_TILE); a.tilesY = cpx_cdiv(H, CC_TILE);
    a.nblk = cpx_cdiv(a.HW, CC_BLOCK); a.conn8 = connectivity == 8;
    const dim3 blk(CC_THR);
    const long long seam_items = (long long)(a.tilesY - 1) * W + (long long)(a.tilesX - 1) * H;      // < 2 * H * W / CC_TILE
    hipLaunchKernelGGL(k_cc_tile, dim3(a.tilesX * a.tilesY, n), blk, 0, s, a);
    if (seam_items > 0) hipLaunchKernelGGL(k_cc_seams, dim3(cpx_cdiv(seam_items, CC_THR), n), blk, 0, s, a);
    hipLaunchKernelGGL(k_cc_roots, dim3(a.nblk, n), blk, 0, s, a);
    hipLaunchKernelGGL(k_cc_offsets, dim3(n), blk, 0, s, a);
    hipLaunchKernelGGL(k_cc_rank, dim3(a.nblk, n), blk, 0, s, a);
    hipLaunchKernelGGL(k_cc_relabel, dim3(cpx_cdiv(a.HW, CC_THR), n), blk, 0, s, a);
    CPX_CHECK_LAUNCH();
    return CPX_OK;
}
