// t3: dataset statistics of (instance, class) training maps on the device: what class weights, oversampling and the
// rescale by cell diameter need, in ONE pass over the maps.
//
// The reference makes that pass on the host, per image: n_classes `np.unique(instances[classes == j])` calls
// (train_utils.py:407-436), one `np.bincount` of the classes (train_utils.py:387-404) and one `fastremap.unique(masks,
// return_counts=True)` inside cellpose.utils.diameters (train_utils.py:256-268).  Here every image has two open-addressing
// tables in the caller's workspace, both of a power of two >= 2 * H * W slots (an image has at most H * W distinct keys of
// either kind, so neither can fill up -- the sizing of cpx_pq_stats):
//     id table      key id + 1                       -> area (pixels of the id over the whole image, whatever the class)
//     (id, class)   key (class + 1) << 32 | id       -> presence only
//
//   k_ls_pixels   a workgroup stages 4096 pixels in LDS; a thread walks 16 consecutive ones and issues one insert + one
//                 integer add per RUN of equal (id, class).  Pixels per class, background pixels, the smallest id and the
//                 status bits are gathered per workgroup in LDS first: one global atomic each per workgroup.
//   k_ls_slots    per slot: (id, class) entries -> inst_per_class; id entries other than the smallest id -> a dense area
//                 list per image (the position comes from an integer counter, so the ORDER of the list depends on
//                 scheduling; its CONTENT, and everything derived from it, does not).
//   k_ls_select   one workgroup per image: radix select (four 8-bit digits, 256-bin LDS histograms, as k_norm_stats_f32)
//                 of the two middle order statistics of the list.  Exact integers: no floating point on the device.
//
// Integer atomics only; launch boundaries are the only device-wide synchronisation.
//
// Reference quirks kept (each is pinned by tests/golden/reference_label_stats.npz):
//   * get_class_counts drops EVERY negative class, not only -100 (`labels[labels >= 0]`, train_utils.py:401);
//   * get_instance_counts counts the background id 0 as an id when it carries class j, and an id that carries two
//     classes in both (`np.unique(instances[classes == j]).size`, train_utils.py:435);
//   * cellpose.utils.diameters drops the count of the SMALLEST id present (`counts[1:]` after a sorted unique): the
//     background when the image has one, else its smallest real cell.
#include "cpx_common.h"

#define LS_THR 256
#define LS_RUN 16                        // consecutive pixels per thread
#define LS_TILE (LS_THR * LS_RUN)        // pixels per workgroup
#define LS_SLOTS 8                       // table slots per thread in k_ls_slots
#define LS_MAXC 64

typedef unsigned long long u64;

struct LsLayout {                        // byte offsets into the workspace
    size_t id_key, ic_key;               // [nI][cap] u64
    size_t id_area;                      // [nI][cap] u32
    size_t count;                        // [nI] u32: length of the area list
    size_t zero_bytes;                   // [0, zero_bytes) is cleared to 0
    size_t min_id;                       // [nI] u32, cleared to 0xff
    size_t areas;                        // [nI][HW] u32, not cleared
    size_t total;
};

static size_t ls_cap(int H, int W) {
    size_t cap = 16;
    while (cap < 2 * (size_t)H * W) cap <<= 1;
    return cap;
}

static LsLayout ls_layout(int nI, int H, int W) {
    LsLayout L; CpxArena a;
    const size_t n = (size_t)nI * ls_cap(H, W);
    L.id_key = a.take(n * 8); L.ic_key = a.take(n * 8); L.id_area = a.take(n * 4); L.count = a.take((size_t)nI * 4);
    L.zero_bytes = a.o;
    L.min_id = a.take((size_t)nI * 4);
    L.areas = a.take((size_t)nI * H * W * 4);
    L.total = a.o;
    return L;
}

// the hash and the insert of cpx_metrics.hip (pq_hash / pq_insert)
__device__ __forceinline__ unsigned ls_hash(u64 k) {
    k ^= k >> 33; k *= 0xff51afd7ed558ccdULL; k ^= k >> 33; k *= 0xc4ceb9fe1a85ec53ULL; k ^= k >> 33;
    return (unsigned)k;
}
// slot of `key` (non-zero) in keys[cap] (cap a power of two), inserted if absent; -1 = table full (cannot happen here)
__device__ __forceinline__ int ls_insert(u64 *keys, int cap, u64 key) {
    unsigned h = ls_hash(key) & (unsigned)(cap - 1);
    for (int probe = 0; probe < cap; ++probe) {
        u64 k = __atomic_load_n(&keys[h], __ATOMIC_RELAXED);
        if (k == 0) k = atomicCAS(&keys[h], 0ULL, key);
        if (k == 0 || k == key) return (int)h;
        h = (h + 1) & (unsigned)(cap - 1);
    }
    return -1;
}

struct LsArgs {
    const int32_t *inst;
    const int16_t *cls;
    int nI, HW, ncls, cap;
    char *ws;
    LsLayout L;
    u64 *class_px;
    int32_t *inst_per_class, *n_masks, *mid_area, *status;
};
#define LS_ARR(type, off, img) (reinterpret_cast<type *>(a.ws + (off)) + (size_t)(img) * a.cap)

__global__ void __launch_bounds__(LS_THR) k_ls_pixels(LsArgs a) {
    // pixel e of the tile sits at e + e / 16: a thread's strip starts at 17 * tid, so the 64 lanes of a wave read 64 banks
    __shared__ int s_id[LS_TILE + LS_THR];
    __shared__ short s_cl[LS_TILE + LS_THR];
    __shared__ unsigned s_px[LS_MAXC], s_bg, s_min, s_status;
    const int img = blockIdx.y, tid = threadIdx.x;
    const int tile0 = blockIdx.x * LS_TILE;
    const int nt = min(LS_TILE, a.HW - tile0);
    const int32_t *ip = a.inst + (size_t)img * a.HW + tile0;
    const int16_t *cp = a.cls + (size_t)img * a.HW + tile0;
    for (int e = tid; e < nt; e += LS_THR) {
        s_id[e + (e >> 4)] = ip[e];
        s_cl[e + (e >> 4)] = cp[e];
    }
    if (tid < LS_MAXC) s_px[tid] = 0;
    if (tid == 0) { s_bg = 0; s_min = 0xffffffffu; s_status = 0; }
    __syncthreads();
    u64 *idk = LS_ARR(u64, a.L.id_key, img), *ick = LS_ARR(u64, a.L.ic_key, img);
    unsigned *area = LS_ARR(unsigned, a.L.id_area, img);
    const int cnt = min(LS_RUN, nt - tid * LS_RUN);          // <= 0 past the end of the image
    const int *sid = s_id + 17 * tid;
    const short *scl = s_cl + 17 * tid;
    unsigned st = 0, mn = 0xffffffffu;
    int k = 0;
    while (k < cnt) {
        const int t = sid[k], c = scl[k];
        int n = 1;
        while (k + n < cnt && sid[k + n] == t && scl[k + n] == c) ++n;
        k += n;
        if (t < 0) { st |= 1u; continue; }                   // the image's results are void: the caller raises
        if (c >= a.ncls) { st |= 2u; continue; }
        mn = min(mn, (unsigned)t);
        if (t == 0) atomicAdd(&s_bg, (unsigned)n);           // the background is every workgroup's hot key: summed in LDS
        else {
            const int s = ls_insert(idk, a.cap, (u64)(unsigned)t + 1);
            if (s >= 0) atomicAdd(&area[s], (unsigned)n);
        }
        if (c >= 0) {                                        // a negative class takes no part in either class output
            atomicAdd(&s_px[c], (unsigned)n);
            ls_insert(ick, a.cap, ((u64)(unsigned)(c + 1) << 32) | (unsigned)t);
        }
    }
    if (mn != 0xffffffffu) atomicMin(&s_min, mn);
    if (st) atomicOr(&s_status, st);
    __syncthreads();
    if (tid < a.ncls && s_px[tid]) atomicAdd(&a.class_px[(size_t)img * a.ncls + tid], (u64)s_px[tid]);
    if (tid == LS_MAXC && s_bg) {
        const int s = ls_insert(idk, a.cap, 1ULL);
        if (s >= 0) atomicAdd(&area[s], s_bg);
    }
    if (tid == LS_MAXC + 1 && s_min != 0xffffffffu) atomicMin(reinterpret_cast<unsigned *>(a.ws + a.L.min_id) + img, s_min);
    if (tid == LS_MAXC + 2 && s_status) atomicOr(&a.status[img], (int)s_status);
}

__global__ void __launch_bounds__(LS_THR) k_ls_slots(LsArgs a) {
    __shared__ unsigned s_ipc[LS_MAXC], s_n, s_base;
    const int img = blockIdx.y, tid = threadIdx.x;
    const int q0 = blockIdx.x * (LS_THR * LS_SLOTS) + tid;
    if (tid < LS_MAXC) s_ipc[tid] = 0;
    if (tid == 0) s_n = 0;
    __syncthreads();
    const u64 *idk = LS_ARR(u64, a.L.id_key, img), *ick = LS_ARR(u64, a.L.ic_key, img);
    const unsigned *area = LS_ARR(unsigned, a.L.id_area, img);
    // cellpose.utils.diameters: `counts[1:]` of a sorted unique drops the smallest id present, background or not
    const u64 drop = (u64)reinterpret_cast<const unsigned *>(a.ws + a.L.min_id)[img] + 1;
    unsigned mine = 0;
#pragma unroll
    for (int j = 0; j < LS_SLOTS; ++j) {
        const int q = q0 + j * LS_THR;
        if (q >= a.cap) break;
        const u64 kc = ick[q];
        if (kc) atomicAdd(&s_ipc[(int)(kc >> 32) - 1], 1u);
        const u64 ki = idk[q];
        if (ki && ki != drop) ++mine;
    }
    unsigned off = 0;
    if (mine) off = atomicAdd(&s_n, mine);
    __syncthreads();
    if (tid == 0 && s_n) s_base = atomicAdd(reinterpret_cast<unsigned *>(a.ws + a.L.count) + img, s_n);
    if (tid < a.ncls && s_ipc[tid]) atomicAdd(&a.inst_per_class[(size_t)img * a.ncls + tid], (int)s_ipc[tid]);
    __syncthreads();
    if (!mine) return;
    unsigned *list = reinterpret_cast<unsigned *>(a.ws + a.L.areas) + (size_t)img * a.HW + s_base + off;
#pragma unroll
    for (int j = 0; j < LS_SLOTS; ++j) {
        const int q = q0 + j * LS_THR;
        if (q >= a.cap) break;
        const u64 ki = idk[q];
        if (ki && ki != drop) *list++ = area[q];
    }
}

// One workgroup per image.  m = the length of the area list; with the areas sorted ascending and ranked from 0 the two values
// np.median averages are those at ranks (m - 1) / 2 and m / 2.  Radix select, most significant byte first; wave r scans the
// histogram of rank r (lane l owns bins 4l .. 4l + 3); while the two ranks share a prefix they share histogram 0.
__global__ void __launch_bounds__(LS_THR) k_ls_select(LsArgs a) {
    __shared__ unsigned hist[2][256];
    __shared__ unsigned s_prefix[2], s_rank[2];
    const int img = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int m = (int)reinterpret_cast<const unsigned *>(a.ws + a.L.count)[img];
    if (m == 0) {
        if (tid == 0) { a.n_masks[img] = 0; a.mid_area[2 * img] = 0; a.mid_area[2 * img + 1] = 0; }
        return;
    }
    const unsigned *list = reinterpret_cast<const unsigned *>(a.ws + a.L.areas) + (size_t)img * a.HW;
    if (tid == 0) { s_rank[0] = (m - 1) / 2; s_rank[1] = m / 2; s_prefix[0] = s_prefix[1] = 0; }
    for (int pass = 0; pass < 4; ++pass) {
        const int shift = 24 - 8 * pass;
        for (int i = tid; i < 2 * 256; i += LS_THR) (&hist[0][0])[i] = 0;
        __syncthreads();
        const unsigned pre0 = s_prefix[0], pre1 = s_prefix[1];
        const bool own1 = pre1 != pre0;
        for (int i = tid; i < m; i += LS_THR) {
            const unsigned v = list[i];
            const unsigned d = (v >> shift) & 255u;
            const unsigned hi_bits = pass == 0 ? 0u : v >> (shift + 8);
            if (hi_bits == pre0) atomicAdd(&hist[0][d], 1u);
            if (own1 && hi_bits == pre1) atomicAdd(&hist[1][d], 1u);
        }
        __syncthreads();
        if (wave < 2) {
            const unsigned *h = hist[(wave == 1 && own1) ? 1 : 0] + 4 * lane;
            const unsigned c0 = h[0], c1 = c0 + h[1], c2 = c1 + h[2], c3 = c2 + h[3];
            unsigned incl = c3;
#pragma unroll
            for (int o = 1; o < 64; o <<= 1) {
                const unsigned up = __shfl_up(incl, o);
                if (lane >= o) incl += up;
            }
            const unsigned excl = incl - c3, k = s_rank[wave];
            const unsigned long long mask = __ballot(incl > k);
            const int l = __ffsll((long long)mask) - 1;      // first lane whose cumulative count passes the rank
            if (lane == l) {
                const int sub = excl + c0 > k ? 0 : (excl + c1 > k ? 1 : (excl + c2 > k ? 2 : 3));
                const unsigned below = excl + (sub == 0 ? 0u : (sub == 1 ? c0 : (sub == 2 ? c1 : c2)));
                s_prefix[wave] = ((wave == 1 ? pre1 : pre0) << 8) | (unsigned)(4 * lane + sub);
                s_rank[wave] = k - below;                    // rank among the areas that carry the longer prefix
            }
        }
        __syncthreads();
    }
    if (tid == 0) {
        a.n_masks[img] = m;
        a.mid_area[2 * img] = (int32_t)s_prefix[0];
        a.mid_area[2 * img + 1] = (int32_t)s_prefix[1];
    }
}

static bool ls_args_ok(int nI, int H, int W, int ncls) {
    return nI > 0 && nI <= 65535 && H > 0 && W > 0 && (long long)H * W <= (1LL << 28) && ncls >= 1 && ncls <= LS_MAXC;
}

extern "C" size_t cpx_label_stats_workspace_bytes(int nI, int H, int W, int ncls) {
    if (!ls_args_ok(nI, H, W, ncls)) return 0;
    return ls_layout(nI, H, W).total;
}

extern "C" int cpx_label_stats(const int32_t *inst, const int16_t *cls, int nI, int H, int W, int ncls, int64_t *class_px,
                               int32_t *inst_per_class, int32_t *n_masks, int32_t *mid_area, int32_t *status,
                               void *workspace, size_t workspace_bytes, void *stream) {
    CPX_REQUIRE(ls_args_ok(nI, H, W, ncls));
    CPX_REQUIRE(inst && cls && class_px && inst_per_class && n_masks && mid_area && status && workspace);
    const LsLayout L = ls_layout(nI, H, W);
    CPX_REQUIRE(workspace_bytes >= L.total);
    hipStream_t s = (hipStream_t)stream;
    CPX_HIP(hipMemsetAsync(workspace, 0, L.zero_bytes, s));
    CPX_HIP(hipMemsetAsync((char *)workspace + L.min_id, 0xff, (size_t)nI * 4, s));
    CPX_HIP(hipMemsetAsync(class_px, 0, (size_t)nI * ncls * 8, s));
    CPX_HIP(hipMemsetAsync(inst_per_class, 0, (size_t)nI * ncls * 4, s));
    CPX_HIP(hipMemsetAsync(status, 0, (size_t)nI * 4, s));
    LsArgs a;
    a.inst = inst; a.cls = cls; a.nI = nI; a.HW = H * W; a.ncls = ncls; a.cap = (int)ls_cap(H, W);
    a.ws = (char *)workspace; a.L = L;
    a.class_px = reinterpret_cast<u64 *>(class_px); a.inst_per_class = inst_per_class; a.n_masks = n_masks;
    a.mid_area = mid_area; a.status = status;
    const dim3 blk(LS_THR);
    hipLaunchKernelGGL(k_ls_pixels, dim3(cpx_cdiv(a.HW, LS_TILE), nI), blk, 0, s, a);
    hipLaunchKernelGGL(k_ls_slots, dim3(cpx_cdiv(a.cap, LS_THR * LS_SLOTS), nI), blk, 0, s, a);
    hipLaunchKernelGGL(k_ls_select, dim3(nI), blk, 0, s, a);
    CPX_CHECK_LAUNCH();
    return CPX_OK;
}
