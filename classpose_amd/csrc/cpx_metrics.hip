// a16b: panoptic-quality statistics of (true, predicted) instance + class maps on the device.
//
// The reference (classpose.metrics: pq.py:95-290, stats_utils.py:8-178, utils.py:162-252) loops over classes, true
// instances and overlapping predicted instances with full-image `pred == pred_id` passes: O(instances x pixels) per
// image.  Every statistic it derives follows from integer co-occurrence tables of one image pair:
//     area_true[c][t], area_pred[c][p], inter[c][t][p]            (pixels; c = class, t / p = instance ids)
// plus, for the unlabelled-cell filter, the same tables without the class.  Here they are open-addressing hash tables in
// the caller's workspace, filled by two pixel passes (one add per RUN of equal (t, p, class, class) keys inside a
// thread's 16-pixel strip, integer atomics only) and consumed by per-slot passes.  Launch boundaries are the only
// device-wide synchronisation (no tickets, no spinning).
//
//   pass A  k_pq_agnostic   inst_t[id] / inst_p[id] (area, LABELLED), pair_a[(t, p)] (inter)         filter or border
//           k_pq_border     BORDER-touching ids -> REMOVED                                            no_border_instances
//           k_pq_filter     per pair_a slot: unlabelled t with IoU > 0.5 -> REMOVED on both sides     multiclass
//   pass B  k_pq_classes    effective ids (REMOVED -> 0): cls_t[(c, t)] / cls_p[(c, p)] (area, first raster pixel),
//                           pair_c[(slot_t, slot_p)] (inter); "the one-class map has a zero pixel" per side
//           k_pq_match      per pair_c slot: iou = inter / (a_t + a_p - inter), ONE float64 division of exactly
//                           converted integers (numpy's true_divide); iou > match_iou -> tp, MATCHED on both entries,
//                           iou added to a 128-bit fixed-point accumulator (four 32-bit limbs in 64-bit integer atomics:
//                           integer addition commutes, so the sum does not depend on arrival order and is EXACT)
//           k_pq_count      per cls_t / cls_p slot: unmatched entries -> fn / fp; optional instance list
//           k_pq_finish     the accumulator rounded ONCE to float64 (round-to-nearest-even) -> iou_sum
//
// A table that fills up marks its image in status[] and the image's results are void: the caller repeats the call with
// a larger table_cap (2 * H * W slots always suffice: an image has at most H * W distinct keys of any kind).
#include "cpx_common.h"

#define PQ_THR 256
#define PQ_RUN 16                    // pixels per thread in the pixel passes
#define PQ_LABELLED 1u
#define PQ_REMOVED 2u
#define PQ_MATCHED 4u
#define PQ_FIX_SHIFT 96              // the accumulator counts units of 2^-96

typedef unsigned long long u64;

struct PqLayout {                    // byte offsets into the workspace; every array is [nI][cap] unless noted
    size_t inst_key[2], inst_area[2], inst_flag[2];        // [side]: 0 = true, 1 = predicted (class-agnostic)
    size_t paira_key, paira_inter;
    size_t cls_key[2], cls_area[2], cls_flag[2], cls_first[2];
    size_t pairc_key, pairc_inter;
    size_t acc;                      // [nI][nr][4] u64 limbs
    size_t haszero;                  // [nI][2] int
    size_t drop;                     // [nI][2] int: 1 + cls slot of the instance at pixel 0 (0 = none)
    size_t total;
    size_t zero_bytes;               // [0, zero_bytes) is cleared to 0, [first_begin, first_end) to 0xff
    size_t first_begin, first_end;
};

static PqLayout pq_layout(int nI, int nr, size_t cap) {
    PqLayout L; CpxArena a;
    const size_t n = (size_t)nI * cap;
    for (int s = 0; s < 2; ++s) { L.inst_key[s] = a.take(n * 8); L.inst_area[s] = a.take(n * 4); L.inst_flag[s] = a.take(n * 4); }
    L.paira_key = a.take(n * 8); L.paira_inter = a.take(n * 4);
    for (int s = 0; s < 2; ++s) { L.cls_key[s] = a.take(n * 8); L.cls_area[s] = a.take(n * 4); L.cls_flag[s] = a.take(n * 4); }
    L.pairc_key = a.take(n * 8); L.pairc_inter = a.take(n * 4);
    L.acc = a.take((size_t)nI * nr * 4 * 8);
    L.haszero = a.take((size_t)nI * 2 * 4);
    L.drop = a.take((size_t)nI * 2 * 4);
    L.zero_bytes = a.o;
    L.first_begin = a.o;
    for (int s = 0; s < 2; ++s) L.cls_first[s] = a.take(n * 4);
    L.first_end = a.o;
    L.total = a.o;
    return L;
}

__device__ __forceinline__ unsigned pq_hash(u64 k) {
    k ^= k >> 33; k *= 0xff51afd7ed558ccdULL; k ^= k >> 33; k *= 0xc4ceb9fe1a85ec53ULL; k ^= k >> 33;
    return (unsigned)k;
}
// slot of `key` (non-zero) in keys[cap] (cap a power of two), inserted if absent; -1 = table full
__device__ __forceinline__ int pq_insert(u64 *keys, int cap, u64 key) {
    unsigned h = pq_hash(key) & (unsigned)(cap - 1);
    for (int probe = 0; probe < cap; ++probe) {
        u64 k = __atomic_load_n(&keys[h], __ATOMIC_RELAXED);
        if (k == 0) k = atomicCAS(&keys[h], 0ULL, key);
        if (k == 0 || k == key) return (int)h;
        h = (h + 1) & (unsigned)(cap - 1);
    }
    return -1;
}
// slot of `key`, -1 if absent (the table was completed by an earlier launch)
__device__ __forceinline__ int pq_find(const u64 *keys, int cap, u64 key) {
    unsigned h = pq_hash(key) & (unsigned)(cap - 1);
    for (int probe = 0; probe < cap; ++probe) {
        const u64 k = keys[h];
        if (k == key) return (int)h;
        if (k == 0) return -1;
        h = (h + 1) & (unsigned)(cap - 1);
    }
    return -1;
}

struct PqArgs {
    const void *ids[2];              // [side] instance ids, IdT [nI][HW]
    const uint8_t *cls[2];           // [side] class maps (both NULL: binary mode, every pixel is class 1)
    int nI, H, W, HW, nr, cap;
    int use_removed;                 // pass A ran: pass B looks the REMOVED flags up
    double match_iou;
    char *ws;
    PqLayout L;
    int32_t *status;
};
#define PQ_ARR(type, off, img) (reinterpret_cast<type *>(a.ws + (off)) + (size_t)(img) * a.cap)

// PQ_RUN consecutive pixels of one image into registers; VEC: HW % 16 == 0 and 16-byte aligned maps
template <class IdT, bool VEC>
__device__ __forceinline__ void pq_load(const PqArgs &a, int img, int base, int (&id)[2][PQ_RUN], int (&cl)[2][PQ_RUN]) {
#pragma unroll
    for (int s = 0; s < 2; ++s) {
        const IdT *ip = reinterpret_cast<const IdT *>(a.ids[s]) + (size_t)img * a.HW + base;
        const uint8_t *cp = a.cls[s] ? a.cls[s] + (size_t)img * a.HW + base : nullptr;
        if (VEC) {
            constexpr int NV = (int)(PQ_RUN * sizeof(IdT) / 16);
            union { uint4 v[NV]; IdT e[PQ_RUN]; } u;
#pragma unroll
            for (int k = 0; k < NV; ++k) u.v[k] = reinterpret_cast<const uint4 *>(ip)[k];
#pragma unroll
            for (int k = 0; k < PQ_RUN; ++k) id[s][k] = (int)u.e[k];
            if (cp) {
                union { uint4 v; uint8_t e[PQ_RUN]; } c;
                c.v = *reinterpret_cast<const uint4 *>(cp);
#pragma unroll
                for (int k = 0; k < PQ_RUN; ++k) cl[s][k] = c.e[k];
            }
        } else {
#pragma unroll
            for (int k = 0; k < PQ_RUN; ++k) {
                const bool in = base + k < a.HW;
                id[s][k] = in ? (int)ip[k] : 0;
                if (cp) cl[s][k] = in ? cp[k] : 0;
            }
        }
        if (!cp) {
#pragma unroll
            for (int k = 0; k < PQ_RUN; ++k) cl[s][k] = 1;
        }
    }
}

// ---- pass A: class-agnostic tables ---------------------------------------------------------------------------------
template <class IdT, bool VEC>
__global__ void __launch_bounds__(PQ_THR) k_pq_agnostic(PqArgs a) {
    const int img = blockIdx.y;
    const int base = (blockIdx.x * PQ_THR + threadIdx.x) * PQ_RUN;
    if (base >= a.HW) return;
    int id[2][PQ_RUN], cl[2][PQ_RUN];
    pq_load<IdT, VEC>(a, img, base, id, cl);
    u64 *kt = PQ_ARR(u64, a.L.inst_key[0], img), *kp = PQ_ARR(u64, a.L.inst_key[1], img), *kq = PQ_ARR(u64, a.L.paira_key, img);
    bool full = false;
    int k = 0;
    while (k < PQ_RUN) {
        const int t = id[0][k], p = id[1][k];
        const int lab = (t != 0 && cl[0][k] > 0) ? 1 : 0;
        int n = 1;
        while (k + n < PQ_RUN && id[0][k + n] == t && id[1][k + n] == p && ((t != 0 && cl[0][k + n] > 0) ? 1 : 0) == lab) ++n;
        k += n;
        if (t == 0 && p == 0) continue;
        int st = -1, sp = -1;
        if (t != 0) {
            st = pq_insert(kt, a.cap, (u64)(unsigned)t);
            if (st < 0) full = true;
            else {
                atomicAdd(&PQ_ARR(unsigned, a.L.inst_area[0], img)[st], (unsigned)n);
                if (lab) atomicOr(&PQ_ARR(unsigned, a.L.inst_flag[0], img)[st], PQ_LABELLED);
            }
        }
        if (p != 0) {
            sp = pq_insert(kp, a.cap, (u64)(unsigned)p);
            if (sp < 0) full = true;
            else atomicAdd(&PQ_ARR(unsigned, a.L.inst_area[1], img)[sp], (unsigned)n);
        }
        if (st >= 0 && sp >= 0) {
            const int sq = pq_insert(kq, a.cap, ((u64)(unsigned)(st + 1) << 32) | (unsigned)(sp + 1));
            if (sq < 0) full = true;
            else atomicAdd(&PQ_ARR(unsigned, a.L.paira_inter, img)[sq], (unsigned)n);
        }
    }
    if (full) a.status[img] = 1;
}

// pq.py:65-92 after the filter: an id with a pixel on the first / last row / column is removed (each map on its own)
template <class IdT>
__global__ void __launch_bounds__(PQ_THR) k_pq_border(PqArgs a) {
    const int img = blockIdx.y;
    const int i = blockIdx.x * PQ_THR + threadIdx.x;
    const int H = a.H, W = a.W;
    if (i >= 2 * (H + W)) return;
    int y, x;
    if (i < W) { y = 0; x = i; }
    else if (i < 2 * W) { y = H - 1; x = i - W; }
    else if (i < 2 * W + H) { y = i - 2 * W; x = 0; }
    else { y = i - 2 * W - H; x = W - 1; }
    for (int s = 0; s < 2; ++s) {
        const int v = (int)(reinterpret_cast<const IdT *>(a.ids[s]) + (size_t)img * a.HW)[y * W + x];
        if (v == 0) continue;
        const int slot = pq_find(PQ_ARR(u64, a.L.inst_key[s], img), a.cap, (u64)(unsigned)v);
        if (slot >= 0) atomicOr(&PQ_ARR(unsigned, a.L.inst_flag[s], img)[slot], PQ_REMOVED);
    }
}

// utils.py:162-252: a true instance without a single class > 0 pixel takes every predicted instance whose
// class-agnostic IoU with it is > 0.5 out of the comparison, and leaves with it
__global__ void __launch_bounds__(PQ_THR) k_pq_filter(PqArgs a) {
    const int img = blockIdx.y;
    const int q = blockIdx.x * PQ_THR + threadIdx.x;
    if (q >= a.cap) return;
    const u64 key = PQ_ARR(u64, a.L.paira_key, img)[q];
    if (key == 0) return;
    const int st = (int)(key >> 32) - 1, sp = (int)(key & 0xffffffffu) - 1;
    if (PQ_ARR(unsigned, a.L.inst_flag[0], img)[st] & PQ_LABELLED) return;
    const long long in = PQ_ARR(unsigned, a.L.paira_inter, img)[q];
    const long long un = (long long)PQ_ARR(unsigned, a.L.inst_area[0], img)[st] + PQ_ARR(unsigned, a.L.inst_area[1], img)[sp] - in;
    if ((double)in / (double)un > 0.5) {
        atomicOr(&PQ_ARR(unsigned, a.L.inst_flag[0], img)[st], PQ_REMOVED);
        atomicOr(&PQ_ARR(unsigned, a.L.inst_flag[1], img)[sp], PQ_REMOVED);
    }
}

// ---- pass B: per-class tables of the filtered maps (stats_utils.py:8-61: inst * (cls == c) per class) ---------------
template <class IdT, bool VEC>
__global__ void __launch_bounds__(PQ_THR) k_pq_classes(PqArgs a) {
    const int img = blockIdx.y;
    const int base = (blockIdx.x * PQ_THR + threadIdx.x) * PQ_RUN;
    if (base >= a.HW) return;
    int id[2][PQ_RUN], cl[2][PQ_RUN];
    pq_load<IdT, VEC>(a, img, base, id, cl);
    // the class of pixel 0 per side: the only class whose one-class map can be free of zero pixels
    int c0[2];
#pragma unroll
    for (int s = 0; s < 2; ++s) c0[s] = a.cls[s] ? (int)a.cls[s][(size_t)img * a.HW] : 1;
    bool full = false;
    bool zero[2] = {false, false};
    int k = 0;
    while (k < PQ_RUN) {
        int t = id[0][k], p = id[1][k];
        int ct = t ? cl[0][k] : 0, cp = p ? cl[1][k] : 0;
        int n = 1;
        while (k + n < PQ_RUN && id[0][k + n] == t && id[1][k + n] == p && (t ? cl[0][k + n] : 0) == ct && (p ? cl[1][k + n] : 0) == cp) ++n;
        const int start = base + k;
        const bool valid = start < a.HW;                 // the padded tail of the last strip is not part of the image
        k += n;
        if (!valid) continue;
        if (a.use_removed) {
            if (t) {
                const int s = pq_find(PQ_ARR(u64, a.L.inst_key[0], img), a.cap, (u64)(unsigned)t);
                if (s < 0 || (PQ_ARR(unsigned, a.L.inst_flag[0], img)[s] & PQ_REMOVED)) { t = 0; ct = 0; }
            }
            if (p) {
                const int s = pq_find(PQ_ARR(u64, a.L.inst_key[1], img), a.cap, (u64)(unsigned)p);
                if (s < 0 || (PQ_ARR(unsigned, a.L.inst_flag[1], img)[s] & PQ_REMOVED)) { p = 0; cp = 0; }
            }
        }
        if (!(t && ct == c0[0])) zero[0] = true;
        if (!(p && cp == c0[1])) zero[1] = true;
        int st = -1, sp = -1;
        if (t && ct >= 1 && ct <= a.nr) {
            st = pq_insert(PQ_ARR(u64, a.L.cls_key[0], img), a.cap, ((u64)(unsigned)ct << 32) | (unsigned)t);
            if (st < 0) full = true;
            else {
                atomicAdd(&PQ_ARR(unsigned, a.L.cls_area[0], img)[st], (unsigned)n);
                atomicMin(&PQ_ARR(unsigned, a.L.cls_first[0], img)[st], (unsigned)start);
                if (start == 0) reinterpret_cast<int *>(a.ws + a.L.drop)[img * 2 + 0] = st + 1;
            }
        }
        if (p && cp >= 1 && cp <= a.nr) {
            sp = pq_insert(PQ_ARR(u64, a.L.cls_key[1], img), a.cap, ((u64)(unsigned)cp << 32) | (unsigned)p);
            if (sp < 0) full = true;
            else {
                atomicAdd(&PQ_ARR(unsigned, a.L.cls_area[1], img)[sp], (unsigned)n);
                atomicMin(&PQ_ARR(unsigned, a.L.cls_first[1], img)[sp], (unsigned)start);
                if (start == 0) reinterpret_cast<int *>(a.ws + a.L.drop)[img * 2 + 1] = sp + 1;
            }
        }
        if (st >= 0 && sp >= 0 && ct == cp) {
            const int sq = pq_insert(PQ_ARR(u64, a.L.pairc_key, img), a.cap, ((u64)(unsigned)(st + 1) << 32) | (unsigned)(sp + 1));
            if (sq < 0) full = true;
            else atomicAdd(&PQ_ARR(unsigned, a.L.pairc_inter, img)[sq], (unsigned)n);
        }
    }
    if (full) a.status[img] = 1;
    int *hz = reinterpret_cast<int *>(a.ws + a.L.haszero) + img * 2;
    if (zero[0]) hz[0] = 1;                              // racing stores of the same value
    if (zero[1]) hz[1] = 1;
}

struct PqPairOut { cpx_pq_pair *pairs; int max_pairs; cpx_pq_inst *insts; int max_insts; int32_t *list_counts; };

// stats_utils.py:100-141.  `true_id_list[1:]` drops the FIRST id of np.unique: the background when the one-class map has a
// zero pixel, else its first-appearing instance (pixel 0's), whose row then stays zero: no pair, no fn.
__global__ void __launch_bounds__(PQ_THR) k_pq_match(PqArgs a, int32_t *tp, PqPairOut o) {
    const int img = blockIdx.y;
    const int q = blockIdx.x * PQ_THR + threadIdx.x;
    if (q >= a.cap) return;
    const u64 key = PQ_ARR(u64, a.L.pairc_key, img)[q];
    if (key == 0) return;
    const int st = (int)(key >> 32) - 1, sp = (int)(key & 0xffffffffu) - 1;
    const int *hz = reinterpret_cast<const int *>(a.ws + a.L.haszero) + img * 2;
    const int *drop = reinterpret_cast<const int *>(a.ws + a.L.drop) + img * 2;
    if (!hz[0] && drop[0] == st + 1) return;
    const int c = (int)(PQ_ARR(u64, a.L.cls_key[0], img)[st] >> 32);
    const long long in = PQ_ARR(unsigned, a.L.pairc_inter, img)[q];
    const long long at = PQ_ARR(unsigned, a.L.cls_area[0], img)[st], ap = PQ_ARR(unsigned, a.L.cls_area[1], img)[sp];
    if (o.pairs) {
        const int w = atomicAdd(&o.list_counts[0], 1);
        if (w < o.max_pairs) {
            cpx_pq_pair r;
            r.image = img; r.cls = c;
            r.first_true = (int32_t)PQ_ARR(unsigned, a.L.cls_first[0], img)[st];
            r.first_pred = (int32_t)PQ_ARR(unsigned, a.L.cls_first[1], img)[sp];
            r.inter = (int32_t)in; r.area_true = (int32_t)at; r.area_pred = (int32_t)ap; r.reserved = 0;
            o.pairs[w] = r;
        }
    }
    const double iou = (double)in / (double)(at + ap - in);
    if (!(iou > a.match_iou)) return;
    atomicAdd(&tp[(size_t)img * a.nr + c - 1], 1);
    atomicOr(&PQ_ARR(unsigned, a.L.cls_flag[0], img)[st], PQ_MATCHED);
    atomicOr(&PQ_ARR(unsigned, a.L.cls_flag[1], img)[sp], PQ_MATCHED);
    // iou = m * 2^(e - 53) with a 53-bit integer m, 2^-32 < iou <= 1: exact in units of 2^-96
    int e;
    const double fr = frexp(iou, &e);
    const u64 m = (u64)ldexp(fr, 53);
    const int sh = e - 53 + PQ_FIX_SHIFT;                 // >= 96 - 32 - 53 > 0
    const unsigned __int128 big = (unsigned __int128)m << sh;
    u64 *acc = reinterpret_cast<u64 *>(a.ws + a.L.acc) + ((size_t)img * a.nr + c - 1) * 4;
#pragma unroll
    for (int l = 0; l < 4; ++l) {
        const u64 limb = (u64)(big >> (32 * l)) & 0xffffffffULL;
        if (limb) atomicAdd(&acc[l], limb);
    }
}

// stats_utils.py:160-168: entries of the id lists (minus the dropped first one) that sit in no pair
__global__ void __launch_bounds__(PQ_THR) k_pq_count(PqArgs a, int32_t *fp, int32_t *fn, PqPairOut o) {
    const int img = blockIdx.y;
    const int q = blockIdx.x * PQ_THR + threadIdx.x;
    if (q >= a.cap) return;
    const int *hz = reinterpret_cast<const int *>(a.ws + a.L.haszero) + img * 2;
    const int *drop = reinterpret_cast<const int *>(a.ws + a.L.drop) + img * 2;
    for (int s = 0; s < 2; ++s) {
        const u64 key = PQ_ARR(u64, a.L.cls_key[s], img)[q];
        if (key == 0) continue;
        const int c = (int)(key >> 32);
        if (o.insts) {
            const int w = atomicAdd(&o.list_counts[1], 1);
            if (w < o.max_insts) {
                cpx_pq_inst r;
                r.image = img; r.side = s; r.cls = c;
                r.first = (int32_t)PQ_ARR(unsigned, a.L.cls_first[s], img)[q];
                r.area = (int32_t)PQ_ARR(unsigned, a.L.cls_area[s], img)[q];
                r.reserved = 0;
                o.insts[w] = r;
            }
        }
        if (!hz[s] && drop[s] == q + 1) continue;
        if (!(PQ_ARR(unsigned, a.L.cls_flag[s], img)[q] & PQ_MATCHED)) atomicAdd(&(s ? fp : fn)[(size_t)img * a.nr + c - 1], 1);
    }
}

// the fixed-point sum -> float64, rounded once to nearest-even; nobg[img][side] = the class whose one-class map has no zero pixel
__global__ void __launch_bounds__(PQ_THR) k_pq_finish(PqArgs a, double *iou_sum, int32_t *nobg) {
    const int i = blockIdx.x * PQ_THR + threadIdx.x;
    if (nobg && i < a.nI * 2) {
        const int img = i >> 1, s = i & 1;
        const int hz = reinterpret_cast<const int *>(a.ws + a.L.haszero)[i];
        const int c0 = a.cls[s] ? (int)a.cls[s][(size_t)img * a.HW] : 1;
        nobg[i] = (!hz && c0 >= 1 && c0 <= a.nr) ? c0 : 0;
    }
    if (i >= a.nI * a.nr) return;
    const u64 *acc = reinterpret_cast<const u64 *>(a.ws + a.L.acc) + (size_t)i * 4;
    unsigned limb[6];
    u64 carry = 0;
    for (int l = 0; l < 6; ++l) {
        const u64 v = (l < 4 ? acc[l] : 0ULL);
        const u64 lo = (v & 0xffffffffULL) + (carry & 0xffffffffULL);
        limb[l] = (unsigned)lo;
        carry = (v >> 32) + (carry >> 32) + (lo >> 32);
    }
    int h = 5;
    while (h >= 0 && limb[h] == 0) --h;
    if (h < 0) { iou_sum[i] = 0.0; return; }
    // a 96-bit window below the top limb + a sticky bit for everything under it
    unsigned __int128 v = 0;
    for (int l = 0; l < 3; ++l) v = (v << 32) | (h - l >= 0 ? limb[h - l] : 0u);
    bool sticky = false;
    for (int l = h - 3; l >= 0; --l) sticky |= limb[l] != 0;
    const int msb = 95 - __clz(limb[h]);                  // bit index of the leading one inside the window, 64 .. 95
    const int sh = msb - 52;
    u64 mant = (u64)(v >> sh);
    const unsigned __int128 rem = v & (((unsigned __int128)1 << sh) - 1), half = (unsigned __int128)1 << (sh - 1);
    if (rem > half || (rem == half && (sticky || (mant & 1)))) ++mant;
    iou_sum[i] = ldexp((double)mant, sh + 32 * (h - 2) - PQ_FIX_SHIFT);
}

static bool pq_pow2(int v) { return v > 0 && (v & (v - 1)) == 0; }

extern "C" size_t cpx_pq_workspace_bytes(int nI, int H, int W, int nr_classes, int table_cap) {
    if (nI <= 0 || H <= 0 || W <= 0 || nr_classes <= 0 || !pq_pow2(table_cap)) return 0;
    return pq_layout(nI, nr_classes, (size_t)table_cap).total;
}

template <class IdT>
static int pq_run(PqArgs a, int filter, int border, int32_t *tp, int32_t *fp, int32_t *fn, double *iou_sum, int32_t *nobg,
                  PqPairOut o, hipStream_t s) {
    bool vec = a.HW % PQ_RUN == 0 && (size_t)a.HW * sizeof(IdT) % 16 == 0;
    for (int k = 0; k < 2; ++k) {
        vec = vec && ((uintptr_t)a.ids[k] % 16 == 0) && ((uintptr_t)a.cls[k] % 16 == 0);
    }
    const dim3 blk(PQ_THR), gpix(cpx_cdiv(a.HW, PQ_THR * PQ_RUN), a.nI), gslot(cpx_cdiv(a.cap, PQ_THR), a.nI);
    if (a.use_removed) {
        if (vec) hipLaunchKernelGGL((k_pq_agnostic<IdT, true>), gpix, blk, 0, s, a);
        else hipLaunchKernelGGL((k_pq_agnostic<IdT, false>), gpix, blk, 0, s, a);
        if (border) hipLaunchKernelGGL((k_pq_border<IdT>), dim3(cpx_cdiv(2 * (a.H + a.W), PQ_THR), a.nI), blk, 0, s, a);
        if (filter) hipLaunchKernelGGL(k_pq_filter, gslot, blk, 0, s, a);
        CPX_CHECK_LAUNCH();
    }
    if (vec) hipLaunchKernelGGL((k_pq_classes<IdT, true>), gpix, blk, 0, s, a);
    else hipLaunchKernelGGL((k_pq_classes<IdT, false>), gpix, blk, 0, s, a);
    hipLaunchKernelGGL(k_pq_match, gslot, blk, 0, s, a, tp, o);
    hipLaunchKernelGGL(k_pq_count, gslot, blk, 0, s, a, fp, fn, o);
    const int nfin = a.nI * a.nr > a.nI * 2 ? a.nI * a.nr : a.nI * 2;
    hipLaunchKernelGGL(k_pq_finish, dim3(cpx_cdiv(nfin, PQ_THR)), blk, 0, s, a, iou_sum, nobg);
    CPX_CHECK_LAUNCH();
    return CPX_OK;
}

extern "C" int cpx_pq_stats(const void *true_ids, const void *pred_ids, int id_bytes, const uint8_t *true_cls,
                            const uint8_t *pred_cls, int nI, int H, int W, int nr_classes, double match_iou,
                            int filter_unlabelled, int no_border_instances, int table_cap, int32_t *tp, int32_t *fp,
                            int32_t *fn, double *iou_sum, int32_t *status, int32_t *nobg, cpx_pq_pair *pairs,
                            int max_pairs, cpx_pq_inst *insts, int max_insts, int32_t *list_counts, void *workspace,
                            size_t workspace_bytes, void *stream) {
    CPX_REQUIRE(true_ids && pred_ids && (id_bytes == 2 || id_bytes == 4));
    CPX_REQUIRE(nI > 0 && nI <= 65535 && H > 0 && W > 0 && (long long)H * W < (1LL << 31) - PQ_THR * PQ_RUN);
    CPX_REQUIRE((true_cls == nullptr) == (pred_cls == nullptr));
    CPX_REQUIRE(nr_classes >= 1 && nr_classes <= 255 && (true_cls || nr_classes == 1) && (true_cls || !filter_unlabelled));
    CPX_REQUIRE(match_iou >= 0.0 && pq_pow2(table_cap) && table_cap >= 16);
    CPX_REQUIRE(tp && fp && fn && iou_sum && status && workspace);
    CPX_REQUIRE((pairs == nullptr) == (insts == nullptr) && (!pairs || (list_counts && max_pairs > 0 && max_insts > 0)));
    const PqLayout L = pq_layout(nI, nr_classes, (size_t)table_cap);
    CPX_REQUIRE(workspace_bytes >= L.total);
    hipStream_t s = (hipStream_t)stream;
    CPX_HIP(hipMemsetAsync(workspace, 0, L.zero_bytes, s));
    CPX_HIP(hipMemsetAsync((char *)workspace + L.first_begin, 0xff, L.first_end - L.first_begin, s));
    const size_t nst = (size_t)nI * nr_classes;
    CPX_HIP(hipMemsetAsync(tp, 0, nst * 4, s));
    CPX_HIP(hipMemsetAsync(fp, 0, nst * 4, s));
    CPX_HIP(hipMemsetAsync(fn, 0, nst * 4, s));
    CPX_HIP(hipMemsetAsync(status, 0, (size_t)nI * 4, s));
    if (list_counts) CPX_HIP(hipMemsetAsync(list_counts, 0, 8, s));
    PqArgs a;
    a.ids[0] = true_ids; a.ids[1] = pred_ids; a.cls[0] = true_cls; a.cls[1] = pred_cls;
    a.nI = nI; a.H = H; a.W = W; a.HW = H * W; a.nr = nr_classes; a.cap = table_cap;
    a.use_removed = (filter_unlabelled || no_border_instances) ? 1 : 0;
    a.match_iou = match_iou; a.ws = (char *)workspace; a.L = L; a.status = status;
    const PqPairOut o{pairs, max_pairs, insts, max_insts, list_counts};
    if (id_bytes == 2) return pq_run<uint16_t>(a, filter_unlabelled, no_border_instances, tp, fp, fn, iou_sum, nobg, o, s);
    return pq_run<int32_t>(a, filter_unlabelled, no_border_instances, tp, fp, fn, iou_sum, nobg, o, s);
}
