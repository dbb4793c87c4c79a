// r3: touching cells of one class -> separate instances on the device: exact squared distance map, its peaks as seeds, every
// pixel to the nearest seed of its own instance, connected components of the result.
//
// cpx_label_components (r2) makes one instance of every connected region of one class, so touching cells merge.  The rule that
// splits them is stated in include/classpose_hip.h (r3) in integers alone; tests/split_reference.py restates it on the CPU and
// the device must equal it on every pixel.
//
//   k_sp_columns  a thread owns one column: a sweep down and a sweep up give g[p], the vertical distance to the nearest pixel of
//                 another value in p's column (SP_NONE where the column holds one value).
//   k_sp_rows     a thread owns one pixel: inside its horizontal run of equal value D2 = min((x - x')^2 + g(x', y)^2), capped by
//                 the squared distance to the first pixel past either run end.  The scan walks outwards and stops once the
//                 squared offset reaches the current best.
//   k_sp_peaks    a thread owns one pixel: a seed when D2 >= min_radius^2 and no pixel of the same instance in the Chebyshev
//                 window beats it (larger D2, or equal D2 and earlier in raster order).  Seeds are flagged in the g plane and
//                 counted per instance id (integer atomic adds).
//   k_sp_blocksum, k_sp_offsets, k_sp_scan
//                 exclusive scan of the per-id counts of every image in three launches (4096 ids per workgroup, one workgroup per
//                 image for the block sums); the image's total -> n_seeds, more than the capacity -> status 1.
//   k_sp_fill     every seed takes a slot of its instance's segment (integer atomic cursor: the order inside a segment is whatever
//                 the scheduler made it) ...
//   k_sp_order    ... and every slot's seed is moved to its rank inside the segment, so a segment ends in raster order whatever
//                 the fill did: the list is a function of the map alone.
//   k_sp_assign   a thread owns one pixel: it scans its own instance's segment for the seed with the smallest squared distance
//                 (the first of equals: the raster-earlier one) and writes 1 + the seed's slot, or capacity + id for an instance
//                 without a seed, into the g plane.
//   cpx_label_components over that plane gives the labels and the counts.
//
// Launch boundaries are the only device-wide synchronisation: no workgroup ever waits for another.  Integer arithmetic and integer
// atomics only; every loop runs over a strictly increasing or decreasing index with a fixed end.
#include "cpx_common.h"

#define SP_THR 256
#define SP_BLOCK 4096                             // table entries per workgroup of the scan passes: SP_THR * 16
#define SP_MAX_PX 268435456                       // 2^28 pixels per image, as cpx_label_components
#define SP_MAX_DIAG2 1073741824                   // H * H + W * W <= 2^30: every sum of two squared distances stays an int32
#define SP_MAX_WINDOW 64                          // min_distance limit: the peak window holds at most 129 x 129 pixels
#define SP_MAX_RADIUS 32768                       // min_radius limit: its square is an int32
#define SP_NONE 0x7fffffff                        // g of a column that holds one value

static_assert(SP_BLOCK % SP_THR == 0 && SP_THR == 256, "block geometry (cpx_block_scan256)");

struct SpArgs {
    const int32_t *map;
    int32_t *d2, *g, *cnt, *off, *sums, *tmp, *seeds, *n_seeds, *status;
    int n, H, W, HW, ntab, nblk, md, r2, cap;
};

__global__ void __launch_bounds__(SP_THR) k_sp_columns(SpArgs a) {
    const int x = blockIdx.x * SP_THR + threadIdx.x, img = blockIdx.y, W = a.W;
    if (x >= W) return;
    const size_t base = (size_t)img * a.HW + x;
    const int32_t *__restrict__ m = a.map + base;
    int32_t *__restrict__ g = a.g + base;
    int prev = m[0], d = SP_NONE;
    g[0] = d;
#pragma unroll 8
    for (int y = 1; y < a.H; ++y) {                                         // distance to the nearest other value above
        const int v = m[y * W];
        d = v != prev ? 1 : (d == SP_NONE ? SP_NONE : d + 1);
        g[y * W] = d;
        prev = v;
    }
    d = SP_NONE;                                                            // prev = m[(H - 1) * W]
#pragma unroll 8
    for (int y = a.H - 2; y >= 0; --y) {                                    // ... and below
        const int v = m[y * W];
        d = v != prev ? 1 : (d == SP_NONE ? SP_NONE : d + 1);
        const int up = g[y * W];
        g[y * W] = d < up ? d : up;
        prev = v;
    }
}

__global__ void __launch_bounds__(SP_THR) k_sp_rows(SpArgs a) {
    const int p = blockIdx.x * SP_THR + threadIdx.x, img = blockIdx.y, W = a.W;
    if (p >= a.HW) return;
    const size_t base = (size_t)img * a.HW;
    const int y = p / W, x = p - y * W;
    const int32_t *row = a.map + base + y * W, *grow = a.g + base + y * W;
    const int v = row[x];
    int best = 0;
    if (v) {
        best = a.H * a.H + W * W;                                           // what a pixel without any site keeps
        const int gc = grow[x];
        if (gc != SP_NONE) best = gc * gc;
        bool left = true, right = true;
        // d strictly increases and a side closes at the image border at the latest; d * d < best <= 2^30
        for (int d = 1; (left || right) && d * d < best; ++d) {
            const int dd = d * d;
            if (left) {
                const int xl = x - d;
                if (xl < 0) left = false;
                else if (row[xl] != v) { best = dd; left = false; }         // dd < best: the loop's condition
                else { const int gg = grow[xl]; if (gg != SP_NONE && dd + gg * gg < best) best = dd + gg * gg; }
            }
            if (right) {
                const int xr = x + d;
                if (xr >= W) right = false;
                else if (row[xr] != v) { if (dd < best) best = dd; right = false; }
                else { const int gg = grow[xr]; if (gg != SP_NONE && dd + gg * gg < best) best = dd + gg * gg; }
            }
        }
    }
    a.d2[base + p] = best;
}

__global__ void __launch_bounds__(SP_THR) k_sp_peaks(SpArgs a) {
    const int p = blockIdx.x * SP_THR + threadIdx.x, img = blockIdx.y, W = a.W;
    if (p >= a.HW) return;
    const size_t base = (size_t)img * a.HW;
    const int32_t *m = a.map + base, *d2 = a.d2 + base;
    const int v = m[p];
    int seed = 0;
    if (v < 0 || v > a.HW) atomicOr(&a.status[img], 2);                     // no slot in the id table: the image is void
    else if (v) {
        const int c = d2[p];
        if (c >= a.r2) {
            const int y = p / W, x = p - y * W;
            const int y0 = y - a.md < 0 ? 0 : y - a.md, y1 = y + a.md > a.H - 1 ? a.H - 1 : y + a.md;
            const int x0 = x - a.md < 0 ? 0 : x - a.md, x1 = x + a.md > W - 1 ? W - 1 : x + a.md;
            seed = 1;
            for (int yy = y0; yy <= y1 && seed; ++yy)
                for (int xx = x0; xx <= x1; ++xx) {
                    const int q = yy * W + xx;
                    if (m[q] != v) continue;
                    const int e = d2[q];
                    if (e > c || (e == c && q < p)) { seed = 0; break; }
                }
            if (seed) atomicAdd(&a.cnt[(size_t)img * a.ntab + v], 1);
        }
    }
    a.g[base + p] = seed;
}

__global__ void __launch_bounds__(SP_THR) k_sp_blocksum(SpArgs a) {
    __shared__ int s_w[SP_THR / 64];
    const int tid = threadIdx.x, img = blockIdx.y;
    const int32_t *cnt = a.cnt + (size_t)img * a.ntab;
    int sum = 0;
    for (int j = 0; j < SP_BLOCK / SP_THR; ++j) {
        const int i = blockIdx.x * SP_BLOCK + j * SP_THR + tid;
        if (i < a.ntab) sum += cnt[i];
    }
    int tot;
    cpx_block_scan256(sum, s_w, &tot);
    if (tid == 0) a.sums[(size_t)img * a.nblk + blockIdx.x] = tot;
}

__global__ void __launch_bounds__(SP_THR) k_sp_offsets(SpArgs a) {           // one workgroup per image: the scan stays inside it
    __shared__ int s_w[SP_THR / 64];
    const int tid = threadIdx.x, img = blockIdx.x;
    int32_t *sums = a.sums + (size_t)img * a.nblk;
    int carry = 0;
    for (int c0 = 0; c0 < a.nblk; c0 += SP_THR) {
        const int i = c0 + tid, v = i < a.nblk ? sums[i] : 0;
        int tot;
        const int incl = cpx_block_scan256(v, s_w, &tot);
        if (i < a.nblk) sums[i] = carry + incl - v;
        carry += tot;
    }
    if (tid == 0) {
        a.n_seeds[img] = carry;                                             // the true total, also when it does not fit
        if (carry > a.cap) a.status[img] |= 1;                              // the only writer of this word in this launch
    }
}

__global__ void __launch_bounds__(SP_THR) k_sp_scan(SpArgs a) {
    __shared__ int s_w[SP_THR / 64];
    const int tid = threadIdx.x, img = blockIdx.y;
    const int32_t *cnt = a.cnt + (size_t)img * a.ntab;
    int32_t *off = a.off + (size_t)img * (a.ntab + 1);
    int running = a.sums[(size_t)img * a.nblk + blockIdx.x];
    for (int j = 0; j < SP_BLOCK / SP_THR; ++j) {
        const int i = blockIdx.x * SP_BLOCK + j * SP_THR + tid;
        const int v = i < a.ntab ? cnt[i] : 0;
        int tot;
        const int incl = cpx_block_scan256(v, s_w, &tot);
        if (i < a.ntab) off[i] = running + incl - v;
        if (i == a.ntab - 1) off[a.ntab] = running + incl;                  // the end of the last segment
        running += tot;
    }
}

__global__ void __launch_bounds__(SP_THR) k_sp_fill(SpArgs a) {
    const int p = blockIdx.x * SP_THR + threadIdx.x, img = blockIdx.y;
    if (p >= a.HW || a.status[img]) return;
    const size_t base = (size_t)img * a.HW;
    if (!a.g[base + p]) return;
    const int v = a.map[base + p];                                          // 1 <= v <= HW: status is 0
    // the count is the cursor: it ends at 0, and a slot is below the image's total, which is at most the capacity
    const int slot = a.off[(size_t)img * (a.ntab + 1) + v] + atomicSub(&a.cnt[(size_t)img * a.ntab + v], 1) - 1;
    a.tmp[(size_t)img * a.cap + slot] = p;
}

__global__ void __launch_bounds__(SP_THR) k_sp_order(SpArgs a) {
    const int j = blockIdx.x * SP_THR + threadIdx.x, img = blockIdx.y;
    if (a.status[img] || j >= a.n_seeds[img]) return;                        // n_seeds <= cap: status is 0
    const int32_t *tmp = a.tmp + (size_t)img * a.cap, *off = a.off + (size_t)img * (a.ntab + 1);
    const int p = tmp[j], v = a.map[(size_t)img * a.HW + p];
    const int lo = off[v], hi = off[v + 1];
    int rank = 0;
    for (int i = lo; i < hi; ++i) rank += tmp[i] < p ? 1 : 0;
    a.seeds[(size_t)img * a.cap + lo + rank] = p;
}

__global__ void __launch_bounds__(SP_THR) k_sp_assign(SpArgs a) {
    const int p = blockIdx.x * SP_THR + threadIdx.x, img = blockIdx.y, W = a.W;
    if (p >= a.HW) return;
    const size_t base = (size_t)img * a.HW;
    const int v = a.map[base + p];
    int out = 0;
    if (v && !a.status[img]) {
        const int32_t *off = a.off + (size_t)img * (a.ntab + 1), *seeds = a.seeds + (size_t)img * a.cap;
        const int lo = off[v], hi = off[v + 1];
        if (hi == lo) out = a.cap + v;                                      // above every 1 + slot, one value per id
        else {
            const int y = p / W, x = p - y * W;
            int bd = SP_NONE, bj = lo;
            for (int j = lo; j < hi; ++j) {
                const int q = seeds[j], qy = q / W, dy = y - qy, dx = x - (q - qy * W);
                const int dist = dy * dy + dx * dx;
                if (dist < bd) { bd = dist; bj = j; }                       // strictly: equals stay with the raster-earlier seed
            }
            out = 1 + bj;
        }
    }
    a.g[base + p] = out;
}

struct SpLayout { size_t d2, g, cnt, off, sums, tmp, cc, cc_bytes, total; };

static bool sp_shape_ok(int n, int H, int W) {
    return n >= 1 && n <= 65535 && H >= 1 && W >= 1 && (long long)H * W <= SP_MAX_PX
           && (long long)H * H + (long long)W * W <= SP_MAX_DIAG2;
}

static SpLayout sp_layout(int n, int H, int W, int cap) {
    SpLayout L; CpxArena a;
    const size_t HW = (size_t)H * W, ntab = HW + 1;
    L.d2 = a.take((size_t)n * HW * 4);
    L.g = a.take((size_t)n * HW * 4);
    L.cnt = a.take((size_t)n * ntab * 4);
    L.off = a.take((size_t)n * (ntab + 1) * 4);
    L.sums = a.take((size_t)n * cpx_cdiv((long long)ntab, SP_BLOCK) * 4);
    L.tmp = a.take((size_t)n * cap * 4);
    L.cc_bytes = cpx_label_components_workspace_bytes(n, H, W);
    L.cc = a.take(L.cc_bytes);
    L.total = a.o;
    return L;
}

static void sp_geometry(SpArgs &a, const int32_t *map, int n, int H, int W) {
    a.map = map; a.n = n; a.H = H; a.W = W; a.HW = H * W;
    a.ntab = a.HW + 1; a.nblk = cpx_cdiv(a.ntab, SP_BLOCK);
}

static void sp_launch_distance(const SpArgs &a, hipStream_t s) {
    hipLaunchKernelGGL(k_sp_columns, dim3(cpx_cdiv(a.W, SP_THR), a.n), dim3(SP_THR), 0, s, a);
    hipLaunchKernelGGL(k_sp_rows, dim3(cpx_cdiv(a.HW, SP_THR), a.n), dim3(SP_THR), 0, s, a);
}

extern "C" int cpx_distance_sq(const int32_t *map, int n, int H, int W, int32_t *d2, void *workspace, size_t workspace_bytes,
                               void *stream) {
    if (n == 0) return CPX_OK;
    CPX_REQUIRE(sp_shape_ok(n, H, W));
    CPX_REQUIRE(workspace_bytes >= (size_t)n * H * W * 4);
    CPX_REQUIRE(map && d2 && workspace);
    CPX_REQUIRE((const void *)d2 != (const void *)map);
    SpArgs a = {};
    sp_geometry(a, map, n, H, W);
    a.d2 = d2; a.g = reinterpret_cast<int32_t *>(workspace);
    sp_launch_distance(a, (hipStream_t)stream);
    CPX_CHECK_LAUNCH();
    return CPX_OK;
}

extern "C" size_t cpx_split_workspace_bytes(int n, int H, int W, int seed_cap) {
    if (!sp_shape_ok(n, H, W) || seed_cap < 1 || seed_cap > (long long)H * W) return 0;
    return sp_layout(n, H, W, seed_cap).total;
}

extern "C" int cpx_split_touching(const int32_t *inst, int n, int H, int W, int min_distance, int min_radius, int connectivity,
                                  int seed_cap, int32_t *labels, int32_t *n_instances, int32_t *seeds, int32_t *n_seeds,
                                  int32_t *status, void *workspace, size_t workspace_bytes, void *stream) {
    CPX_REQUIRE(connectivity == 4 || connectivity == 8);
    CPX_REQUIRE(min_distance >= 1 && min_distance <= SP_MAX_WINDOW);
    CPX_REQUIRE(min_radius >= 1 && min_radius <= SP_MAX_RADIUS);
    if (n == 0) return CPX_OK;
    CPX_REQUIRE(sp_shape_ok(n, H, W));
    CPX_REQUIRE(seed_cap >= 1 && seed_cap <= (long long)H * W);
    const SpLayout L = sp_layout(n, H, W, seed_cap);
    CPX_REQUIRE(workspace_bytes >= L.total);
    CPX_REQUIRE(inst && labels && n_instances && seeds && n_seeds && status && workspace);
    CPX_REQUIRE((const void *)labels != (const void *)inst);
    hipStream_t s = (hipStream_t)stream;
    char *ws = (char *)workspace;
    SpArgs a = {};
    sp_geometry(a, inst, n, H, W);
    a.d2 = reinterpret_cast<int32_t *>(ws + L.d2); a.g = reinterpret_cast<int32_t *>(ws + L.g);
    a.cnt = reinterpret_cast<int32_t *>(ws + L.cnt); a.off = reinterpret_cast<int32_t *>(ws + L.off);
    a.sums = reinterpret_cast<int32_t *>(ws + L.sums); a.tmp = reinterpret_cast<int32_t *>(ws + L.tmp);
    a.seeds = seeds; a.n_seeds = n_seeds; a.status = status;
    a.md = min_distance; a.r2 = min_radius * min_radius; a.cap = seed_cap;
    const dim3 blk(SP_THR), px(cpx_cdiv(a.HW, SP_THR), n), tab(a.nblk, n);
    CPX_HIP(hipMemsetAsync(status, 0, (size_t)n * 4, s));
    CPX_HIP(hipMemsetAsync(a.cnt, 0, (size_t)n * a.ntab * 4, s));
    sp_launch_distance(a, s);
    hipLaunchKernelGGL(k_sp_peaks, px, blk, 0, s, a);
    hipLaunchKernelGGL(k_sp_blocksum, tab, blk, 0, s, a);
    hipLaunchKernelGGL(k_sp_offsets, dim3(n), blk, 0, s, a);
    hipLaunchKernelGGL(k_sp_scan, tab, blk, 0, s, a);
    hipLaunchKernelGGL(k_sp_fill, px, blk, 0, s, a);
    hipLaunchKernelGGL(k_sp_order, dim3(cpx_cdiv(seed_cap, SP_THR), n), blk, 0, s, a);
    hipLaunchKernelGGL(k_sp_assign, px, blk, 0, s, a);
    CPX_CHECK_LAUNCH();
    return cpx_label_components(a.g, n, H, W, connectivity, labels, n_instances, ws + L.cc, L.cc_bytes, stream);
}
