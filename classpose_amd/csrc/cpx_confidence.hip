// Per-cell class confidence on gfx950 (include/classpose_hip.h: cpx_instance_confidence): per instance of the final id
// map, the class vote table, the summed softmax of the class logits and the summed sigmoid of cellprob.
//
// A stand-alone pass AFTER the fused post-processing chain (cpx_postproc.hip), which it does not touch: it re-reads the
// id map, the logits and cellprob once, nT * H * W * (4 * ncls + 6) bytes.
//
// Exactness: every per-pixel probability is computed in float64 and quantised to 2^-24 (llrint, round half to even)
// BEFORE it is summed, so all sums are integer sums -- 64-bit integer adds in LDS, 64-bit integer atomics in global memory.
// The result does not depend on the order in which pixels arrive; there are no floating-point atomics.  Built with
// -ffp-contract=off: the softmax is the written sequence of IEEE operations (max, subtract, exp, add in class order, divide).
//
// Shape: one pass, a lane owns a pixel and consecutive lanes own consecutive pixels of a row, so each of the ncls logit
// planes is read coalesced.  A workgroup collects its pixels' contributions per (label, class) in an LDS open-addressing
// table (the lh_slot pattern of cpx_postproc.hip, keyed by label * 33 + class; pseudo-class 32 = the detection sum) and
// flushes one global atomic per occupied slot and quantity.  A contribution that finds no slot in 8 probes goes straight
// to global integer atomics, as in k_class_count.
#include "cpx_common.h"
#include "cpx_internal.h"

#define CF_THREADS 256
#define CF_MAXCLS 32                    // == PP_MAXCLS, the vote table's class limit (cpx_postproc.hip)
#define CF_DET CF_MAXCLS                // pseudo-class of the detection sum in a slot key
#define CF_KEYS (CF_MAXCLS + 1)
#define CF_SLOTS 512                    // 16 B per slot: 8 KB of LDS
#define CF_SLOT_BITS 9
#define CF_Q 16777216.0                 // 2^24

struct CfLds {
    int key[CF_SLOTS];                  // (label - 1) * CF_KEYS + class + 1; 0 = free
    int cnt[CF_SLOTS];                  // votes
    unsigned long long sum[CF_SLOTS];   // quantised probability sum
};

struct CfOut {
    int32_t *votes;                     // this tile's [max_rec][ncls]
    unsigned long long *prob_q;         // this tile's [max_rec][ncls]
    unsigned long long *cellprob_q;     // this tile's [max_rec]
    int ncls;
};

__device__ __forceinline__ int cf_slot(int *key, int k) {
    const unsigned h = ((unsigned)k * 2654435761u) >> (32 - CF_SLOT_BITS);
#pragma unroll 1
    for (int p = 0; p < 8; ++p) {
        const int s = (int)((h + p) & (CF_SLOTS - 1));
        const int old = atomicCAS(&key[s], 0, k);
        if (old == 0 || old == k) return s;
    }
    return -1;
}

// where slot key k's quantities live in global memory; row < min(rec_counts, max_rec) and c < ncls (or CF_DET) by construction
__device__ __forceinline__ void cf_global_add(const CfOut &o, int row, int c, int votes, unsigned long long q) {
    if (c == CF_DET) {
        if (q) atomicAdd(&o.cellprob_q[row], q);
    } else {
        const size_t i = (size_t)row * o.ncls + c;
        if (votes) atomicAdd(&o.votes[i], votes);
        if (q) atomicAdd(&o.prob_q[i], q);
    }
}

__device__ __forceinline__ void cf_add(CfLds &L, const CfOut &o, int row, int c, int votes, unsigned long long q) {
    const int s = cf_slot(L.key, row * CF_KEYS + c + 1);
    if (s >= 0) {
        // workgroup scope: LDS adds (ds_add_u32 / ds_add_u64) that the compiler cannot merge with the global atomics of the other branch
        if (votes) __hip_atomic_fetch_add(&L.cnt[s], votes, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        if (q) __hip_atomic_fetch_add(&L.sum[s], q, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    } else {
        cf_global_add(o, row, c, votes, q);
    }
}

// FOOT 0: a workgroup = 256 consecutive pixels of the raster (one row piece where W >= 256); FOOT 1: a 16 x 16 block, 16
// lanes per row.  Grid: (workgroups per tile, nT).
template <int FOOT>
__global__ void __launch_bounds__(CF_THREADS) k_confidence(const uint16_t *__restrict__ masks, const float *__restrict__ logits,
                                                           const float *__restrict__ cellprob, const int32_t *__restrict__ rec_counts,
                                                           int ncls, int H, int W, int max_rec, int32_t *__restrict__ votes,
                                                           unsigned long long *__restrict__ prob_q,
                                                           unsigned long long *__restrict__ cellprob_q) {
    __shared__ CfLds L;
    for (int i = threadIdx.x; i < CF_SLOTS; i += CF_THREADS) { L.key[i] = 0; L.cnt[i] = 0; L.sum[i] = 0; }
    __syncthreads();
    const size_t t = blockIdx.y;
    const int HW = H * W;
    int nrec = rec_counts[t];
    nrec = nrec < 0 ? 0 : (nrec > max_rec ? max_rec : nrec);
    CfOut o;
    o.ncls = ncls;
    o.votes = votes ? votes + t * (size_t)max_rec * ncls : nullptr;
    o.prob_q = prob_q ? prob_q + t * (size_t)max_rec * ncls : nullptr;
    o.cellprob_q = cellprob_q ? cellprob_q + t * (size_t)max_rec : nullptr;

    int idx = -1;
    if (FOOT == 0) {
        const long long i = (long long)blockIdx.x * CF_THREADS + threadIdx.x;
        if (i < HW) idx = (int)i;
    } else {
        const int nbx = (W + 15) >> 4;
        const int y = (int)(blockIdx.x / nbx) * 16 + (int)(threadIdx.x >> 4), x = (int)(blockIdx.x % nbx) * 16 + (int)(threadIdx.x & 15);
        if (y < H && x < W) idx = y * W + x;
    }
    int lab = 0;
    if (idx >= 0) lab = masks[t * HW + idx];
    if (lab >= 1 && lab <= nrec) {                       // 0, ids past rec_counts and ids past max_rec are background
        const int row = lab - 1;
        if (cellprob) {
            const float z = cellprob[t * HW + idx];
            unsigned long long q = 0;
            if (fabsf(z) <= 3.402823466e38f) {           // finite (false for a NaN)
                const double p = 1.0 / (1.0 + exp(-(double)z));
                q = (unsigned long long)llrint(p * CF_Q);
            }
            if (q) cf_add(L, o, row, CF_DET, 0, q);
        }
        if (logits) {
            const float *lg = logits + t * (size_t)ncls * HW + idx;
            // registers, not memory: every index below is a compile-time constant behind a uniform guard
            double e[CF_MAXCLS];
            float best = lg[0], mx = best;
            int bi = 0;
            bool finite = fabsf(best) <= 3.402823466e38f;
            e[0] = (double)best;
#pragma unroll
            for (int c = 1; c < CF_MAXCLS; ++c) {
                if (c < ncls) {
                    const float v = lg[(size_t)c * HW];
                    // np.argmax: the first maximum wins, a NaN beats every number and the first NaN wins (k_class_count)
                    const bool take = !(v <= best) & (best == best);
                    best = take ? v : best; bi = take ? c : bi;
                    finite &= fabsf(v) <= 3.402823466e38f;
                    mx = v > mx ? v : mx;
                    e[c] = (double)v;
                }
            }
            if (!finite) {
                cf_add(L, o, row, bi, 1, 0);             // it votes; it adds 0 to every probability sum
            } else {
                const double m = (double)mx;
                double s = 0.0;
#pragma unroll
                for (int c = 0; c < CF_MAXCLS; ++c) {
                    if (c < ncls) { e[c] = exp(e[c] - m); s = s + e[c]; }
                }
#pragma unroll
                for (int c = 0; c < CF_MAXCLS; ++c) {
                    if (c < ncls) {
                        const unsigned long long q = (unsigned long long)llrint((e[c] / s) * CF_Q);
                        const int v = c == bi ? 1 : 0;
                        if (v | (q != 0)) cf_add(L, o, row, c, v, q);
                    }
                }
            }
        }
    }
    __syncthreads();
    for (int i = threadIdx.x; i < CF_SLOTS; i += CF_THREADS) {
        const int k = L.key[i];
        if (k) cf_global_add(o, (k - 1) / CF_KEYS, (k - 1) % CF_KEYS, L.cnt[i], L.sum[i]);
    }
}

// rows < min(rec_counts[t], max_rec) of the enabled parts to 0, from the device-resident counts; every other row untouched
__global__ void __launch_bounds__(CF_THREADS) k_confidence_clear(const int32_t *__restrict__ rec_counts, int ncls, int max_rec,
                                                                 int32_t *__restrict__ votes, unsigned long long *__restrict__ prob_q,
                                                                 unsigned long long *__restrict__ cellprob_q) {
    const size_t t = blockIdx.y;
    int nrec = rec_counts[t];
    nrec = nrec < 0 ? 0 : (nrec > max_rec ? max_rec : nrec);
    const long long i = (long long)blockIdx.x * CF_THREADS + threadIdx.x;
    if (votes && i < (long long)nrec * ncls) {
        votes[t * (size_t)max_rec * ncls + i] = 0;
        prob_q[t * (size_t)max_rec * ncls + i] = 0;
    }
    if (cellprob_q && i < nrec) cellprob_q[t * (size_t)max_rec + i] = 0;
}

// the workgroup's pixel footprint: 0 = 256 consecutive pixels (production), 1 = a 16 x 16 block (tools/bench_cell_confidence.py)
CPX_SWITCH(g_conf_foot, 0);
#ifdef CPX_DEBUG
extern "C" void cpx_confidence_set_footprint(int foot) { g_conf_foot = foot; }
#endif

extern "C" size_t cpx_instance_confidence_workspace_bytes(int nT, int ncls, int H, int W, int max_rec) {
    (void)nT; (void)ncls; (void)H; (void)W; (void)max_rec;
    return 0;                           // the tables are the outputs themselves; the argument pair is kept for the ABI's sake
}

extern "C" int cpx_instance_confidence(const uint16_t *masks_u16, const float *logits, const float *cellprob,
                                       const int32_t *rec_counts, int nT, int ncls, int H, int W, int max_rec,
                                       int32_t *votes, uint64_t *prob_q, uint64_t *cellprob_q,
                                       void *workspace, size_t workspace_bytes, void *stream) {
    (void)workspace;
    CPX_REQUIRE(nT > 0 && nT <= 65535 && H >= 1 && W >= 1 && H <= 16384 && W <= 16384 && max_rec > 0);
    CPX_REQUIRE(ncls >= 0 && ncls <= CF_MAXCLS);
    CPX_REQUIRE(masks_u16 && rec_counts);
    CPX_REQUIRE(workspace_bytes >= cpx_instance_confidence_workspace_bytes(nT, ncls, H, W, max_rec));
    const bool cls_part = logits != nullptr && ncls > 1;
    CPX_REQUIRE(cls_part || cellprob);
    CPX_REQUIRE(!cls_part || (votes && prob_q));
    CPX_REQUIRE(!cellprob || cellprob_q);
    hipStream_t s = (hipStream_t)stream;
    const int ncp = cls_part ? ncls : 0;
    int32_t *v = cls_part ? votes : nullptr;
    unsigned long long *pq = cls_part ? (unsigned long long *)prob_q : nullptr;
    unsigned long long *cq = cellprob ? (unsigned long long *)cellprob_q : nullptr;
    const int nclear = cpx_cdiv((long long)max_rec * (ncp > 1 ? ncp : 1), CF_THREADS);
    hipLaunchKernelGGL(k_confidence_clear, dim3(nclear, nT), dim3(CF_THREADS), 0, s, rec_counts, ncp, max_rec, v, pq, cq);
    const float *lg = cls_part ? logits : nullptr;
    if (g_conf_foot == 1)
        hipLaunchKernelGGL(k_confidence<1>, dim3(cpx_cdiv(W, 16) * cpx_cdiv(H, 16), nT), dim3(CF_THREADS), 0, s, masks_u16, lg,
                           cellprob, rec_counts, ncp, H, W, max_rec, v, pq, cq);
    else
        hipLaunchKernelGGL(k_confidence<0>, dim3(cpx_cdiv((long long)H * W, CF_THREADS), nT), dim3(CF_THREADS), 0, s, masks_u16, lg,
                           cellprob, rec_counts, ncp, H, W, max_rec, v, pq, cq);
    CPX_CHECK_LAUNCH();
    return CPX_OK;
}
