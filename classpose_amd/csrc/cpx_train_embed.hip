// The backward of the patch embedding and the position table (gfx950): the last stage of full fine-tuning.
//   forward   x[row][c] = round(sum_k p[row][k] W[c][k] + b[c] + pos[row % 1024][c])      p [rows][192], W [1024][192], pos [1024][1024]
//   backward  from dx [rows][1024] float32, the gradient of block 0's input (cpx_blocks_backward_in), rounding passed straight through:
//     dpos[t][c] = sum over crops n of dx[n * 1024 + t][c]       float64 chain in crop order, rounded once
//     db[c]      = sum over rows of dx[row][c]                   float64: per column the per-token float64 sums of dpos, unrounded, added in
//                                                                token order within groups of EB_POS_T tokens, the groups' partials in order
//     dW[c][k]   = sum over rows of dx[row][c] p[row][k]
//         grad_dtype CPX_DT_F32   exact-float32 MFMA (cpx_gemm_f32) behind transposing copies, p widened exactly, in slabs of two crops added
//                                 in slab order -- the float32 route of the blocks' linear_bwd
//         grad_dtype CPX_DT_BF16  k_embed_dw16 below: r(dx)^T p on v_mfma_f32_32x32x16_bf16, dx rounded to bf16 once (nearest even) on its way
//                                 to LDS, float32 accumulation
// One flat float32 record W | b | pos (cpx_embed_grad_layout) is overwritten.  No atomics, no workgroup waits for another, every sum in an
// order fixed by n_subtiles alone: two runs are bitwise equal.
//
// k_embed_dw16: the shape cpx_gemm_tn_bf16 does not take (K = 192; a contraction of rows = 32 768 at 32 crops against 1024 x 192 outputs).
//   split     the rows are split across workgroups: grid (8 tiles of 128 channels, S splits), S = 8 min(n_subtiles, 4) -- 128 rows per split up
//             to 4 crops, 32 n_subtiles rows from there (256 workgroups on 256 CUs) --, each split writing its float32 partial tile to
//             part [S][1024][192]; k_embed_dw_finish adds the partials in split order.
//   tile      128 (c) x 192 (k) per workgroup, 32 rows per stage; 4 waves of 64 (c) x 96 (k) = 2 x 3 MFMA tiles
//   LDS       per stage three [32 m][256 B] tiles in the chunk order of cpx_gemm_tn.hip (tn_off there): r(dx) columns c0 .. c0 + 127, p columns
//             0 .. 127, p columns 128 .. 191 (chunks 0 .. 7 of its rows; the XOR spreads them over the 256-byte row, so the pitch stays);
//             two stages: 48 KB.  Both operands are read transposed by ds_read_b64_tr_b16, as there: lane l holds row / column l & 31 and
//             contraction slots 8 (l >> 5) .. + 7 from two reads of 4 rows each.
//   schedule  the next stage's dx (4 float4) and p (3 chunks) per thread are loaded to registers before the current stage's 12 MFMAs per
//             wave, rounded and stored after them; one barrier per stage.  All tiles are full: no bounds branch, EXEC all ones at every
//             transposed read.
#include "cpx_internal.h"
#include <algorithm>

typedef __attribute__((ext_vector_type(8))) __bf16 eb_bf16x8;
typedef __attribute__((ext_vector_type(4))) short eb_s16x4;
typedef __attribute__((ext_vector_type(8))) short eb_s16x8;
typedef __attribute__((ext_vector_type(4))) unsigned eb_u32x4;

#define EB_C 1024
#define EB_K 192
#define EB_BN 128
#define EB_BM 32
#define EB_TILE (EB_BM * 256)            // bytes of one LDS tile
#define EB_POS_T 4                       // tokens per workgroup of k_embed_pos
#define EB_SLAB 2                        // crops per slab of the float32 route

static int embed_splits(int nS) { return 8 * std::min(nS, 4); }

__device__ __forceinline__ int eb_off(int row, int ch) { return 256 * row + 16 * (ch ^ (((row & 3) << 2) | ((row >> 2) & 3))); }
__device__ __forceinline__ eb_s16x4 eb_read(const unsigned char *p) {
    return __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) eb_s16x4 *)p);
}
__device__ __forceinline__ unsigned eb_pack(float lo, float hi) { return (unsigned)f32_to_bf16(lo) | ((unsigned)f32_to_bf16(hi) << 16); }

// grid (EB_C / EB_BN, S); rows_split a multiple of EB_BM
__global__ void __launch_bounds__(256) k_embed_dw16(const float *__restrict__ dx, const unsigned short *__restrict__ p, int rows_split,
                                                    float *__restrict__ part) {
    __shared__ __attribute__((aligned(16))) unsigned char lds[2][3][EB_TILE];      // [stage][r(dx) | p 0..127 | p 128..191]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int n0 = blockIdx.x * EB_BN;
    const size_t m0 = (size_t)blockIdx.y * rows_split;
    const int wn = (wave >> 1) * 64, wk = (wave & 1) * 96;

    // staging: dx chunk id = tid + 256 j (j < 2) -> row id >> 4, chunk id & 15 (8 floats); p chunk id = tid + 256 j (j < 3) -> row id / 24,
    // chunk id % 24 (8 bf16)
    float4 ra[2][2];
    eb_u32x4 rb[3];
    auto load = [&](int t) {
        const size_t m = m0 + (size_t)t * EB_BM;
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const int id = tid + 256 * j, row = id >> 4, ch = id & 15;
            const float *src = dx + (m + row) * EB_C + n0 + 8 * ch;
            ra[j][0] = *reinterpret_cast<const float4 *>(src);
            ra[j][1] = *reinterpret_cast<const float4 *>(src + 4);
        }
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            const int id = tid + 256 * j, row = id / 24, ch = id - 24 * row;
            rb[j] = *reinterpret_cast<const eb_u32x4 *>(p + (m + row) * EB_K + 8 * ch);
        }
    };
    auto store = [&](int buf) {
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const int id = tid + 256 * j;
            const eb_u32x4 v = {eb_pack(ra[j][0].x, ra[j][0].y), eb_pack(ra[j][0].z, ra[j][0].w), eb_pack(ra[j][1].x, ra[j][1].y),
                                eb_pack(ra[j][1].z, ra[j][1].w)};
            *reinterpret_cast<eb_u32x4 *>(&lds[buf][0][eb_off(id >> 4, id & 15)]) = v;
        }
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            const int id = tid + 256 * j, row = id / 24, ch = id - 24 * row;
            *reinterpret_cast<eb_u32x4 *>(&lds[buf][1 + (ch >> 4)][eb_off(row, ch & 15)]) = rb[j];
        }
    };
    // the transposed read of lane l for the 32 columns from element column cb of a tile, contraction rows 16 ks + 8 (l >> 5) [+ 4]
    // (cpx_gemm_tn.hip: lane 4 q + p of its 16-lane group g supplies row q, columns 4 p .. 4 p + 3 of the block at column cb + 16 (g & 1))
    const int g = lane >> 4, q = (lane >> 2) & 3, pp = lane & 3;
    const int rq = 8 * (g >> 1) + q, cg = 2 * (g & 1) + (pp >> 1), ob = 8 * (pp & 1);
    auto operand = [&](const unsigned char *tile, int cb, int ks) {
        const int c = (cb >> 3) + cg, r = 16 * ks + rq;
        const eb_s16x4 lo = eb_read(tile + eb_off(r, c) + ob), hi = eb_read(tile + eb_off(r + 4, c) + ob);
        const eb_s16x8 v = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
        return __builtin_bit_cast(eb_bf16x8, v);
    };

    f32x16 acc[2][3];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j)
#pragma unroll
            for (int v = 0; v < 16; ++v) acc[i][j][v] = 0.f;

    const int T = rows_split / EB_BM;
    load(0);
    store(0);
    __syncthreads();
    for (int t = 0; t < T; ++t) {
        const int buf = t & 1;
        if (t + 1 < T) load(t + 1);                                   // (uniform in the workgroup)
#pragma unroll
        for (int ks = 0; ks < EB_BM / 16; ++ks) {
            eb_bf16x8 a[2], b[3];
#pragma unroll
            for (int i = 0; i < 2; ++i) a[i] = operand(lds[buf][0], wn + 32 * i, ks);
#pragma unroll
            for (int j = 0; j < 3; ++j) {
                const int cb = wk + 32 * j;                           // 0 .. 160: the third tile holds columns 128 ..
                b[j] = operand(lds[buf][1 + (cb >> 7)], cb & 127, ks);
            }
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int j = 0; j < 3; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[i], b[j], acc[i][j], 0, 0, 0);
        }
        if (t + 1 < T) store(buf ^ 1);
        __syncthreads();
    }
    // accumulator register v of lane l: row (v & 3) + 8 (v >> 2) + 4 (l >> 5), column l & 31 of the 32 x 32 tile
    const int r = lane & 31, h2 = lane >> 5;
    float *o0 = part + (size_t)blockIdx.y * EB_C * EB_K;
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            float *o = o0 + (size_t)(n0 + wn + 32 * i + 4 * h2) * EB_K + wk + 32 * j + r;
#pragma unroll
            for (int v = 0; v < 16; ++v) o[(size_t)((v & 3) + 8 * (v >> 2)) * EB_K] = acc[i][j][v];
        }
}
// dW = ((part[0] + part[1]) + part[2]) + ...: the splits in order, float32.  One thread per four elements.
__global__ void __launch_bounds__(256) k_embed_dw_finish(const float *__restrict__ part, int S, float *__restrict__ dW) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x, n4 = (size_t)EB_C * EB_K / 4;
    if (i >= n4) return;
    float4 s = *reinterpret_cast<const float4 *>(part + 4 * i);
    for (int k = 1; k < S; ++k) {
        const float4 v = *reinterpret_cast<const float4 *>(part + ((size_t)k * n4 + i) * 4);
        s.x += v.x; s.y += v.y; s.z += v.z; s.w += v.w;
    }
    *reinterpret_cast<float4 *>(dW + 4 * i) = s;
}

// dpos and the partials of db in one pass over dx.  grid (1024 / EB_POS_T): thread = four columns, EB_POS_T tokens in order, per token one
// float64 chain over the crops in order -> dpos (rounded once); the unrounded token sums added in token order -> partb [group][1024].
__global__ void __launch_bounds__(256) k_embed_pos(const float *__restrict__ dx, int nS, float *__restrict__ dpos, double *__restrict__ partb) {
    const int c = 4 * threadIdx.x;
    double b[4] = {0, 0, 0, 0};
    for (int tt = 0; tt < EB_POS_T; ++tt) {
        const int t = blockIdx.x * EB_POS_T + tt;
        double s[4] = {0, 0, 0, 0};
        for (int n = 0; n < nS; ++n) {
            const float4 v = *reinterpret_cast<const float4 *>(dx + ((size_t)n * 1024 + t) * EB_C + c);
            s[0] += (double)v.x; s[1] += (double)v.y; s[2] += (double)v.z; s[3] += (double)v.w;
        }
        *reinterpret_cast<float4 *>(dpos + (size_t)t * EB_C + c) = make_float4((float)s[0], (float)s[1], (float)s[2], (float)s[3]);
#pragma unroll
        for (int i = 0; i < 4; ++i) b[i] += s[i];
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) partb[(size_t)blockIdx.x * EB_C + c + i] = b[i];
}
__global__ void __launch_bounds__(256) k_embed_db_finish(const double *__restrict__ partb, float *__restrict__ db) {
    const int c = blockIdx.x * 256 + threadIdx.x;
    double s = 0;
    for (int k = 0; k < 1024 / EB_POS_T; ++k) s += partb[(size_t)k * EB_C + c];
    db[c] = (float)s;
}
// the float32 route forms dW in a [1024][256] buffer (cpx_gemm_f32 takes widths that are multiples of 128): its first 192 columns -> dW
__global__ void __launch_bounds__(256) k_embed_dw_crop(const float *__restrict__ wide, float *__restrict__ dW) {
    const int i = blockIdx.x * 256 + threadIdx.x;                      // < 1024 * 48 float4
    const int r = i / (EB_K / 4), c4 = i - r * (EB_K / 4);
    *reinterpret_cast<float4 *>(dW + (size_t)r * EB_K + 4 * c4) = *reinterpret_cast<const float4 *>(wide + (size_t)r * 256 + 4 * c4);
}

extern "C" long long cpx_embed_grad_layout(long long *off) {
    if (off) { off[0] = 0; off[1] = (long long)EB_C * EB_K; off[2] = (long long)EB_C * EB_K + EB_C; }
    return (long long)EB_C * EB_K + EB_C + 1024ll * EB_C;
}

// workspace: the float64 partials of db; then bf16 mode: the float32 partial tiles of the splits (24 MiB from 4 crops up); float32 mode: the
// transposed slab operands [1024][Ms] and [256][Ms] (rows 192 .. zero) and the [1024][256] result (11 MiB)
struct EmbedBwdLayout { size_t partb, part, t1, t2, wide, total; };
static EmbedBwdLayout embed_bwd_layout(int nS, int grad_dtype) {
    EmbedBwdLayout L; CpxArena a; const bool g16 = grad_dtype == CPX_DT_BF16; const size_t Ms = (size_t)EB_SLAB * 1024;
    L.partb = a.take((size_t)(1024 / EB_POS_T) * EB_C * sizeof(double));
    L.part = a.take(g16 ? (size_t)embed_splits(nS) * EB_C * EB_K * 4 : 0);
    L.t1 = a.take(g16 ? 0 : (size_t)EB_C * Ms * 4); L.t2 = a.take(g16 ? 0 : 256 * Ms * 4); L.wide = a.take(g16 ? 0 : (size_t)EB_C * 256 * 4);
    L.total = a.o;
    return L;
}
static bool embed_args_ok(int nS, int dtype, int grad_dtype) { return cpx_crops_ok(nS) && dtype_ok(dtype) && cpx_grad_dtype_ok(dtype, grad_dtype); }
extern "C" size_t cpx_embed_backward_workspace_bytes(int nS, int dtype, int grad_dtype) {
    return embed_args_ok(nS, dtype, grad_dtype) ? embed_bwd_layout(nS, grad_dtype).total : 0;
}

extern "C" int cpx_embed_backward(int dtype, const void *patches, const float *dx_in, int nS, int grad_dtype, float *grads, void *workspace,
                                  size_t workspace_bytes, void *stream) {
    CPX_REQUIRE(patches && dx_in && grads && workspace && embed_args_ok(nS, dtype, grad_dtype));
    const EmbedBwdLayout L = embed_bwd_layout(nS, grad_dtype);
    CPX_REQUIRE(workspace_bytes >= L.total && ((uintptr_t)workspace & 255) == 0);
    CPX_REQUIRE((((uintptr_t)patches | (uintptr_t)dx_in | (uintptr_t)grads) & 15) == 0);
    hipStream_t s = (hipStream_t)stream;
    char *ws = (char *)workspace;
    long long go[3];
    cpx_embed_grad_layout(go);
    float *dW = grads + go[0], *db = grads + go[1], *dpos = grads + go[2];
    double *partb = (double *)(ws + L.partb);
    hipLaunchKernelGGL(k_embed_pos, dim3(1024 / EB_POS_T), dim3(256), 0, s, dx_in, nS, dpos, partb);
    CPX_CHECK_LAUNCH();
    hipLaunchKernelGGL(k_embed_db_finish, dim3(EB_C / 256), dim3(256), 0, s, (const double *)partb, db);
    CPX_CHECK_LAUNCH();
    if (grad_dtype == CPX_DT_BF16) {
        const int S = embed_splits(nS), rows_split = (int)((size_t)nS * 1024 / S);      // 128, or 32 nS: a multiple of EB_BM
        float *part = (float *)(ws + L.part);
        hipLaunchKernelGGL(k_embed_dw16, dim3(EB_C / EB_BN, S), dim3(256), 0, s, dx_in, (const unsigned short *)patches, rows_split, part);
        CPX_CHECK_LAUNCH();
        hipLaunchKernelGGL(k_embed_dw_finish, grid1((size_t)EB_C * EB_K / 4), dim3(256), 0, s, (const float *)part, S, dW);
        CPX_CHECK_LAUNCH();
        return CPX_OK;
    }
    float *t1 = (float *)(ws + L.t1), *t2 = (float *)(ws + L.t2), *wide = (float *)(ws + L.wide);
    const size_t es = es_of(dtype);
    for (int c0 = 0; c0 < nS; c0 += EB_SLAB) {
        const int Ms = std::min(EB_SLAB, nS - c0) * 1024;
        const size_t r0 = (size_t)c0 * 1024;
        CPX_RUN(cpx_transpose_f32_run(CPX_DT_F32, dx_in + r0 * EB_C, Ms, EB_C, t1, s));
        CPX_RUN(cpx_transpose_f32_run(dtype, (const char *)patches + r0 * EB_K * es, Ms, EB_K, t2, s));
        CPX_HIP(hipMemsetAsync(t2 + (size_t)EB_K * Ms, 0, (size_t)(256 - EB_K) * Ms * 4, s));
        CPX_RUN(cpx_gemm_f32(t1, t2, EB_C, 256, Ms, c0 ? CPX_EPI_RESID_BF16 : CPX_EPI_F32, nullptr, c0 ? wide : nullptr, wide, 256, stream));
    }
    hipLaunchKernelGGL(k_embed_dw_crop, grid1((size_t)EB_C * EB_K / 4), dim3(256), 0, s, (const float *)wide, dW);
    CPX_CHECK_LAUNCH();
    return CPX_OK;
}
