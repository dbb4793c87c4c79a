// The attention backward of a bf16 network on the bf16 matrix instruction (gfx950): cpx_attention_backward_bf16, the opt-in third precision
// switch of the blocks' backward (cpx_blocks_backward_mp, attn_grad_dtype CPX_DT_BF16).  The function differentiated and the decomposition are
// cpx_attention_backward's (cpx_train_blocks.hip: one wave per image row of 32 queries for dq, one wave per 32 keys for dk and dv, the
// table gradients from the row-group sums; no atomics, no workgroup waits for another, every sum in a fixed order).  What changes is the
// arithmetic of the nine 1024 x 1024 x 64 products per (crop, head): v_mfma_f32_32x32x16_bf16 with float32 accumulation.
//
// Contract.  q, k, v, Rh, Rw as stored (bf16, exact); r(.) = round to nearest even to bf16, each value once:
//   S'    = q . (k + Rh[qy - ky + 31] + Rw[qx - kx + 31])    three bf16 products, each accumulated in float32, added in float32, nothing rounded
//   P     = softmax_j(scale S')                              float32, exponent (S' - m) * scale, times 1 / l before any rounding
//   dP    = r(dO) v^T                                        r(dO) is the only form in which dO enters anything
//   delta = sum_j P dP                                       float32, from the unrounded P and dP
//   dS'   = scale P (dP - delta)                             float32
//   dv    = r(P)^T r(dO),   dk = r(dS')^T q
//   dq    = r(dS') k + sum_ky r(G_h) Rh[..] + sum_kx r(G_w) Rw[..]      (the bias terms: exact products, float32 sums in key order)
//   G_h, G_w = the row-group sums of the unrounded float32 dS';  dRh, dRw = cpx_attn_rel_grad_run on them (the float32 mode's code)
//
// Operands.  D = A B of the instruction: lane (r, h) = (lane & 31, lane >> 5) holds A[row r][k = 8 h + j] and B[k = 8 h + j][col r],
// j = 0 .. 7, and D[row A16_SLOT(v, h)][col r] in register v.
//   k_attn_bwd16_dq   S'^T = K Q^T and dP^T = V r(dO)^T: the key in the registers, the query on the lane.  A: rows of the K / V tile in LDS
//                     (one 16-byte read per k-step); B: the wave's Q and r(dO) rows, in registers for the whole kernel.  dS'^T is then
//                     the B operand of dq^T = K^T dS'^T as it lies: registers 8 s .. 8 s + 7 rounded pairwise are k-step s, whose
//                     element j is key 16 s + 8 (j >> 2) + 4 h + (j & 3); the A operand K^T is read in that key order by two transposed
//                     reads (ds_read_b64_tr_b16) of four keys each from the same K image.
//   k_attn_bwd16_dkv  S' = Q K^T and dP = r(dO) V^T: the query in the registers, the key on the lane.  A: rows of the Q / r(dO) tiles;
//                     B: the wave's K and V rows in registers.  P and dS' are the B operands of dv^T = r(dO)^T P and dk^T = Q^T dS',
//                     Q^T and r(dO)^T by transposed reads of the same two images.  dO is rounded as its tile is staged; the float32
//                     values go no further than the staging registers.
// LDS image of a [32 rows][64 bf16] tile (4 KB): 16-byte chunk ch (0 .. 7) of row m at
//   128 m + 16 (ch ^ ((((m >> 1) & 1) << 2) | ((m >> 2) & 3)))
// counted by the bank rule (64 banks of 4 bytes = 16 slots of 16 bytes per 256-byte bank row; two tile rows share a bank row):
//   row read (ds_read_b128, lane r: row r, chunk 2 s + h; lane groups {0-3, 12-15, 20-27}, {4-11, 16-19, 28-31} and the same + 32): a
//     group holds 8 even and 8 odd rows; the even ones of the first group, 0 2 12 14 20 22 24 26, get the XOR values 0 4 3 7 1 5 2 6 and
//     those of the second, 4 6 8 10 16 18 28 30, get 1 5 2 6 0 4 3 7: eight different chunks in each half of the bank row -> 16 slots once;
//   transposed read (per 32-lane half rows m0 .. m0 + 3, m0 a multiple of 4, chunks c0 .. c0 + 3, c0 0 or 4): m0, m0 + 2 lie in one
//     half of the bank row and differ in bit 2 of the XOR, so they take the two different aligned groups of four chunks; likewise
//     m0 + 1, m0 + 3 in the other half: 16 slots once;
//   store (ds_write_b128, 8 consecutive lanes = one row's 8 chunks, permuted): 32 banks once.
//   0 conflict cycles computed for every access of the tiles (not measured with a counter).  The float32 side arrays (the bias rows
//   with stride 36, the per-wave scratch with stride 97) are the float32 kernels' and keep their access patterns.
// Every lane runs every LDS instruction (the only branches are uniform in the workgroup), so EXEC is all ones at the transposed reads.
//
// Footprint (the compiler's resource-usage remarks, gfx950): k_attn_bwd16_dq 216 VGPRs, 0 AGPRs, no scratch, no spill, 66 048 bytes of
// LDS; k_attn_bwd16_dkv 222 VGPRs, 0 AGPRs, no scratch, no spill, 27 392 bytes of LDS.  Both: occupancy 2 waves per SIMD = 2 workgroups
// per CU (registers; for dq the LDS allows 2 as well).  The blocks' backward launches a slab of two crops, 256 workgroups, which is one
// workgroup per CU and one wave per SIMD: the kernels run latency-bound there.
#include "cpx_internal.h"

typedef __attribute__((ext_vector_type(8))) __bf16 a16_bf16x8;
typedef __attribute__((ext_vector_type(4))) short a16_s16x4;
typedef __attribute__((ext_vector_type(8))) short a16_s16x8;
typedef __attribute__((ext_vector_type(4))) unsigned a16_u32x4;

#define A16_TILE 4096                   // bytes of a [32][64] bf16 tile image
#define A16_GLD 97                      // per-query scratch row of the dq kernel: [0, 64) q . table rows, [64, 96) the G_h sums
#define A16_SLOT(v, h2) (((v) & 3) + 8 * ((v) >> 2) + 4 * (h2))
#define MFMA_BF16(a, b, c) __builtin_amdgcn_mfma_f32_32x32x16_bf16((a), (b), (c), 0, 0, 0)

__device__ __forceinline__ int a16_off(int row, int ch) { return 128 * row + 16 * (ch ^ ((((row >> 1) & 1) << 2) | ((row >> 2) & 3))); }
__device__ __forceinline__ a16_s16x4 a16_tr(const unsigned char *p) {
    return __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) a16_s16x4 *)p);
}
// k-step s (channels 16 s + 8 h2 ..) of row r of a tile image: the A operand of a product that sums over the channels
__device__ __forceinline__ a16_bf16x8 a16_row(const unsigned char *tile, int r, int h2, int s) {
    return *reinterpret_cast<const a16_bf16x8 *>(tile + a16_off(r, 2 * s + h2));
}
// the A operand tile^T[channel cb + (lane & 31)][row] of a product that sums over the tile's 32 rows against an accumulator tile: k-step
// s, element j = row 16 s + 8 (j >> 2) + 4 h2 + (j & 3).  Lane 4 q + p of a 16-lane group supplies row q, elements 4 p .. 4 p + 3 of the
// group's block of 4 rows x 16 channels
__device__ __forceinline__ a16_bf16x8 a16_col(const unsigned char *tile, int lane, int cb, int s) {
    const int g = lane >> 4, q = (lane >> 2) & 3, p = lane & 3;
    const int row = 16 * s + 4 * (g >> 1) + q, ch = (cb >> 3) + 2 * (g & 1) + (p >> 1), ob = 8 * (p & 1);
    const a16_s16x4 lo = a16_tr(tile + a16_off(row, ch) + ob), hi = a16_tr(tile + a16_off(row + 8, ch) + ob);
    const a16_s16x8 v = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
    return __builtin_bit_cast(a16_bf16x8, v);
}
// eight float32 values rounded to nearest even: registers 8 s .. 8 s + 7 of an accumulator are k-step s of the next product
__device__ __forceinline__ a16_bf16x8 a16_pack(const float *x) {
    a16_bf16x8 o;
#pragma unroll
    for (int j = 0; j < 8; ++j) o[j] = (__bf16)x[j];
    return o;
}
__device__ __forceinline__ a16_bf16x8 a16_pack(float4 a, float4 b) {
    const float x[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
    return a16_pack(x);
}
__device__ __forceinline__ float a16_round(float x) { return bf16_to_f32(f32_to_bf16(x)); }
__device__ __forceinline__ float4 a16_widen4(const void *p, size_t idx) { return ld4<CPX_DT_BF16>(p, idx); }

// ---------------------------------------------------------------------------
// dq, the row statistics and the row-group sums of dS'
// ---------------------------------------------------------------------------
// grid (8 row groups, 16 heads, crops), 4 waves: wave w of row group g owns the image row qh = 4 g + w, lane (r, h2) the query qx = r.
// Accumulator register v belongs to key kx = A16_SLOT(v, h2) of the tile (S'^T, dP^T) or to channel A16_SLOT(v, h2) (dq^T).
// st_*, Bh, Bw, Gh, Gw are indexed by (crop * 16 + head) * 1024 + query, as in the float32 kernels.
__global__ void __launch_bounds__(256) k_attn_bwd16_dq(const unsigned short *__restrict__ qkv, const unsigned short *__restrict__ relh,
                                                       const unsigned short *__restrict__ relw, const float *__restrict__ dO,
                                                       float *__restrict__ dqkv, float *__restrict__ st_m, float *__restrict__ st_il,
                                                       float *__restrict__ st_delta, float *__restrict__ Bh, float *__restrict__ Bw,
                                                       float *__restrict__ Gh, float *__restrict__ Gw) {
    __shared__ __attribute__((aligned(16))) unsigned char sK[2][A16_TILE];
    __shared__ __attribute__((aligned(16))) unsigned char sV[2][A16_TILE];
    __shared__ float sG[4][32 * A16_GLD];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int r = lane & 31, h2 = lane >> 5;
    const int head = blockIdx.y, s = blockIdx.z, qh = blockIdx.x * 4 + wave;
    const size_t tok0 = (size_t)s * 1024;
    const size_t qi = ((size_t)s * 16 + head) * 1024 + qh * 32 + r;

    // the B operands Q^T and r(dO)^T: channels 16 ks + 8 h2 .. + 7 of the lane's query
    a16_bf16x8 qB[4], doB[4];
    {
        const size_t qo = (tok0 + qh * 32 + r) * 3072 + head * 64 + 8 * h2, oo = (tok0 + qh * 32 + r) * 1024 + head * 64 + 8 * h2;
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) {
            qB[ks] = *reinterpret_cast<const a16_bf16x8 *>(qkv + qo + 16 * ks);
            doB[ks] = a16_pack(*reinterpret_cast<const float4 *>(dO + oo + 16 * ks), *reinterpret_cast<const float4 *>(dO + oo + 16 * ks + 4));
        }
    }
    // G[q][j] = q . table[j] -> the wave's scratch
    float *G = sG[wave];
    auto compute_G = [&](const unsigned short *table) {
#pragma unroll
        for (int jb = 0; jb < 2; ++jb) {
            f32x16 acc;
#pragma unroll
            for (int v = 0; v < 16; ++v) acc[v] = 0.f;
            const size_t to = (size_t)(jb * 32 + r) * 64 + 8 * h2;
#pragma unroll
            for (int ks = 0; ks < 4; ++ks) acc = MFMA_BF16(*reinterpret_cast<const a16_bf16x8 *>(table + to + 16 * ks), qB[ks], acc);
#pragma unroll
            for (int v = 0; v < 16; ++v) G[r * A16_GLD + jb * 32 + A16_SLOT(v, h2)] = acc[v];
        }
        // G belongs to this wave alone, and its lane halves read each other's stores: a wave's LDS operations complete in order; the
        // wave barrier keeps the compiler from moving a load above these stores
        __builtin_amdgcn_wave_barrier();
    };
    compute_G(relw);
    f32x16 GW;
#pragma unroll
    for (int v = 0; v < 16; ++v) GW[v] = G[r * A16_GLD + (r - A16_SLOT(v, h2) + 31)];
#pragma unroll
    for (int g4 = 0; g4 < 4; ++g4)
        *reinterpret_cast<float4 *>(Bw + qi * 32 + 8 * g4 + 4 * h2) = make_float4(GW[4 * g4], GW[4 * g4 + 1], GW[4 * g4 + 2], GW[4 * g4 + 3]);
    __builtin_amdgcn_wave_barrier();                                   // the reads of q . Rw above, before q . Rh overwrites them
    compute_G(relh);
#pragma unroll
    for (int k = 0; k < 16; ++k) Bh[qi * 32 + h2 * 16 + k] = G[r * A16_GLD + (qh - (h2 * 16 + k) + 31)];

    // K / V tiles: 32 keys x 64 channels, thread -> (key tid >> 3, chunk tid & 7)
    const int skey = tid >> 3, sch = tid & 7;
    const size_t kbase = (tok0 + skey) * 3072 + 1024 + head * 64 + 8 * sch;
    const int sdst = a16_off(skey, sch);
    a16_u32x4 kr, vr;
    auto load_kv = [&](int kh) {
        const size_t o = kbase + (size_t)kh * 32 * 3072;
        kr = *reinterpret_cast<const a16_u32x4 *>(qkv + o);
        vr = *reinterpret_cast<const a16_u32x4 *>(qkv + o + 1024);
    };
    auto store_kv = [&](int buf) {
        *reinterpret_cast<a16_u32x4 *>(&sK[buf][sdst]) = kr;
        *reinterpret_cast<a16_u32x4 *>(&sV[buf][sdst]) = vr;
    };
    // S'^T = K . Q^T on top of the Rw bias (the Rh bias gh is one number per query and tile); dP^T = V . r(dO)^T
    auto scores = [&](int buf) {
        f32x16 S = GW;
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) S = MFMA_BF16(a16_row(sK[buf], r, h2, ks), qB[ks], S);
        return S;
    };
    auto dprobs = [&](int buf) {
        f32x16 dP;
#pragma unroll
        for (int v = 0; v < 16; ++v) dP[v] = 0.f;
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) dP = MFMA_BF16(a16_row(sV[buf], r, h2, ks), doB[ks], dP);
        return dP;
    };
    const float cexp = 0.125f * 1.44269504088896340736f;      // scale * log2(e)

    // pass 1: m = max_j S'[i][j], l = sum_j exp(scale (S'[i][j] - m)) and delta = sum_j P[i][j] dP[i][j]
    float m_run = -1e30f, l_run = 0.f, d_run = 0.f;
    load_kv(0);
    store_kv(0);
    __syncthreads();
    for (int kh = 0; kh < 32; ++kh) {
        const int buf = kh & 1;
        if (kh + 1 < 32) load_kv(kh + 1);
        const float gh = G[r * A16_GLD + (qh - kh + 31)];
        const f32x16 S = scores(buf);
        const f32x16 dP = dprobs(buf);
        float mx = S[0];
#pragma unroll
        for (int v = 1; v < 16; ++v) mx = fmaxf(mx, S[v]);
        mx = fmaxf(mx, __shfl_xor(mx, 32)) + gh;
        const float m_new = fmaxf(m_run, mx);
        const float alpha = __builtin_amdgcn_exp2f((m_run - m_new) * cexp);
        m_run = m_new;
        // (S' - m) first, then the one multiplication, as in the float32 kernel
        const float off = gh - m_new;
        float ps = 0.f, pd = 0.f;
#pragma unroll
        for (int v = 0; v < 16; ++v) { const float p = __builtin_amdgcn_exp2f((S[v] + off) * cexp); ps += p; pd = fmaf(p, dP[v], pd); }
        l_run = fmaf(l_run, alpha, ps);
        d_run = fmaf(d_run, alpha, pd);
        if (kh + 1 < 32) store_kv(buf ^ 1);
        __syncthreads();
    }
    const float inv_l = 1.0f / (l_run + __shfl_xor(l_run, 32));
    const float delta = (d_run + __shfl_xor(d_run, 32)) * inv_l;
    if (h2 == 0) { st_m[qi] = m_run; st_il[qi] = inv_l; st_delta[qi] = delta; }

    // pass 2
    f32x16 dQ[2];
    float gw[16];
#pragma unroll
    for (int v = 0; v < 16; ++v) { dQ[0][v] = 0.f; dQ[1][v] = 0.f; gw[v] = 0.f; }
    load_kv(0);
    store_kv(0);
    __syncthreads();
    for (int kh = 0; kh < 32; ++kh) {
        const int buf = kh & 1;
        if (kh + 1 < 32) load_kv(kh + 1);
        const float gh = G[r * A16_GLD + (qh - kh + 31)];
        const f32x16 S = scores(buf);
        const f32x16 dP = dprobs(buf);
        const float off = gh - m_run;
        float ds[16], gsum = 0.f;
#pragma unroll
        for (int v = 0; v < 16; ++v) {
            const float p = __builtin_amdgcn_exp2f((S[v] + off) * cexp) * inv_l;
            ds[v] = 0.125f * (p * (dP[v] - delta));
            gsum += ds[v];
            gw[v] += ds[v];
        }
        gsum += __shfl_xor(gsum, 32);
        G[r * A16_GLD + 64 + kh] = gsum;                         // (both lane halves store the same value; read after the loop)
        // dq^T[d][q] += K^T[d][key] r(dS'^T)[key][q]
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) {
            const a16_bf16x8 dsB = a16_pack(ds + 8 * ks);
            dQ[0] = MFMA_BF16(a16_col(sK[buf], lane, 0, ks), dsB, dQ[0]);
            dQ[1] = MFMA_BF16(a16_col(sK[buf], lane, 32, ks), dsB, dQ[1]);
        }
        if (kh + 1 < 32) store_kv(buf ^ 1);
        __syncthreads();
    }
    // the row-group sums: G_w from the registers (through the scratch: both lane halves need all 32), G_h from the scratch
#pragma unroll
    for (int v = 0; v < 16; ++v) G[r * A16_GLD + A16_SLOT(v, h2)] = gw[v];
    __builtin_amdgcn_wave_barrier();                                   // both lane halves read all 32 below
#pragma unroll
    for (int g4 = 0; g4 < 4; ++g4) {
        *reinterpret_cast<float4 *>(Gw + qi * 32 + 8 * g4 + 4 * h2) = make_float4(gw[4 * g4], gw[4 * g4 + 1], gw[4 * g4 + 2], gw[4 * g4 + 3]);
        const float *gp = &G[r * A16_GLD + 64 + h2 * 16 + 4 * g4];
        *reinterpret_cast<float4 *>(Gh + qi * 32 + h2 * 16 + 4 * g4) = make_float4(gp[0], gp[1], gp[2], gp[3]);
    }
    // the bias term of dq: 32 table rows weighted by r(G_h) (row index uniform in the wave), 32 weighted by r(G_w) (row index per query);
    // every product of two bf16 values is exact in float32
    for (int k = 0; k < 32; ++k) {
        const float g_h = a16_round(G[r * A16_GLD + 64 + k]), g_w = a16_round(G[r * A16_GLD + k]);
        const size_t th = (size_t)(qh - k + 31) * 64, tw = (size_t)(r - k + 31) * 64;
#pragma unroll
        for (int db = 0; db < 2; ++db)
#pragma unroll
            for (int g4 = 0; g4 < 4; ++g4) {
                const int d = db * 32 + 8 * g4 + 4 * h2;
                const float4 a = a16_widen4(relh, th + d), b = a16_widen4(relw, tw + d);
                dQ[db][4 * g4] = fmaf(g_w, b.x, fmaf(g_h, a.x, dQ[db][4 * g4]));
                dQ[db][4 * g4 + 1] = fmaf(g_w, b.y, fmaf(g_h, a.y, dQ[db][4 * g4 + 1]));
                dQ[db][4 * g4 + 2] = fmaf(g_w, b.z, fmaf(g_h, a.z, dQ[db][4 * g4 + 2]));
                dQ[db][4 * g4 + 3] = fmaf(g_w, b.w, fmaf(g_h, a.w, dQ[db][4 * g4 + 3]));
            }
    }
    float *orow = dqkv + (tok0 + qh * 32 + r) * 3072 + head * 64;
#pragma unroll
    for (int db = 0; db < 2; ++db)
#pragma unroll
        for (int g4 = 0; g4 < 4; ++g4)
            *reinterpret_cast<float4 *>(orow + db * 32 + 8 * g4 + 4 * h2) =
                make_float4(dQ[db][4 * g4], dQ[db][4 * g4 + 1], dQ[db][4 * g4 + 2], dQ[db][4 * g4 + 3]);
}

// ---------------------------------------------------------------------------
// dk and dv
// ---------------------------------------------------------------------------
// grid as above; wave w of row group g owns the key row kh = 4 g + w, lane (r, h2) the key kx = r.  Accumulator register v belongs to
// query qx = A16_SLOT(v, h2) of the tile (S', dP) or to channel A16_SLOT(v, h2) (dk^T, dv^T).  The query tiles are staged one ahead
// (registers, then the other LDS buffer): one barrier per tile.
struct A16Side { float bw[32 * 36]; float bh[4][32], m[32], il[32], dl[32]; };
__global__ void __launch_bounds__(256) k_attn_bwd16_dkv(const unsigned short *__restrict__ qkv, const float *__restrict__ dO,
                                                        const float *__restrict__ st_m, const float *__restrict__ st_il,
                                                        const float *__restrict__ st_delta, const float *__restrict__ Bh,
                                                        const float *__restrict__ Bw, float *__restrict__ dqkv) {
    __shared__ __attribute__((aligned(16))) unsigned char sQ[2][A16_TILE];
    __shared__ __attribute__((aligned(16))) unsigned char sD[2][A16_TILE];
    __shared__ __attribute__((aligned(16))) A16Side sS[2];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int r = lane & 31, h2 = lane >> 5;
    const int head = blockIdx.y, s = blockIdx.z, kh = blockIdx.x * 4 + wave;
    const size_t tok0 = (size_t)s * 1024;
    const size_t qi0 = ((size_t)s * 16 + head) * 1024;

    a16_bf16x8 kB[4], vB[4];
    {
        const size_t ko = (tok0 + kh * 32 + r) * 3072 + 1024 + head * 64 + 8 * h2;
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) {
            kB[ks] = *reinterpret_cast<const a16_bf16x8 *>(qkv + ko + 16 * ks);
            vB[ks] = *reinterpret_cast<const a16_bf16x8 *>(qkv + ko + 1024 + 16 * ks);
        }
    }
    f32x16 dK[2], dV[2];
#pragma unroll
    for (int v = 0; v < 16; ++v) { dK[0][v] = 0.f; dK[1][v] = 0.f; dV[0][v] = 0.f; dV[1][v] = 0.f; }

    // staging: thread -> (query tid >> 3, chunk tid & 7) of Q and dO; (query tid >> 3, 4 kx at (tid & 7) * 4) of the Rw bias; one
    // value of the Rh bias (threads 0 .. 127) or of m, 1 / l, delta (128 .. 223)
    const int sq = tid >> 3, sch = tid & 7, sdst = a16_off(sq, sch);
    a16_u32x4 q_r;
    float4 d0_r, d1_r, bw_r;
    float x_r = 0.f;
    auto load_tile = [&](int qt) {
        const size_t row = tok0 + qt * 32 + sq;
        q_r = *reinterpret_cast<const a16_u32x4 *>(qkv + row * 3072 + head * 64 + 8 * sch);
        d0_r = *reinterpret_cast<const float4 *>(dO + row * 1024 + head * 64 + 8 * sch);
        d1_r = *reinterpret_cast<const float4 *>(dO + row * 1024 + head * 64 + 8 * sch + 4);
        bw_r = *reinterpret_cast<const float4 *>(Bw + (qi0 + qt * 32 + sq) * 32 + sch * 4);
        const size_t q1 = qi0 + qt * 32 + (tid & 31);
        if (tid < 128) x_r = Bh[q1 * 32 + blockIdx.x * 4 + (tid >> 5)];
        else if (tid < 160) x_r = st_m[q1];
        else if (tid < 192) x_r = st_il[q1];
        else if (tid < 224) x_r = st_delta[q1];
    };
    auto store_tile = [&](int buf) {
        *reinterpret_cast<a16_u32x4 *>(&sQ[buf][sdst]) = q_r;
        *reinterpret_cast<a16_bf16x8 *>(&sD[buf][sdst]) = a16_pack(d0_r, d1_r);          // dO is rounded here, once
        *reinterpret_cast<float4 *>(&sS[buf].bw[sq * 36 + sch * 4]) = bw_r;
        if (tid < 128) sS[buf].bh[tid >> 5][tid & 31] = x_r;
        else if (tid < 160) sS[buf].m[tid & 31] = x_r;
        else if (tid < 192) sS[buf].il[tid & 31] = x_r;
        else if (tid < 224) sS[buf].dl[tid & 31] = x_r;
    };
    const float cexp = 0.125f * 1.44269504088896340736f;
    load_tile(0);
    store_tile(0);
    __syncthreads();
    for (int qt = 0; qt < 32; ++qt) {
        const int buf = qt & 1;
        if (qt + 1 < 32) load_tile(qt + 1);
        // S'[q][key] = Q . K^T and dP[q][key] = r(dO) . V^T
        f32x16 S, dP;
#pragma unroll
        for (int v = 0; v < 16; ++v) { S[v] = 0.f; dP[v] = 0.f; }
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) {
            S = MFMA_BF16(a16_row(sQ[buf], r, h2, ks), kB[ks], S);
            dP = MFMA_BF16(a16_row(sD[buf], r, h2, ks), vB[ks], dP);
        }
        const A16Side &side = sS[buf];
        float p[16], ds[16];
#pragma unroll
        for (int v = 0; v < 16; ++v) {
            const int q = A16_SLOT(v, h2);
            const float sp = (S[v] + side.bw[q * 36 + r]) + side.bh[wave][q];
            p[v] = __builtin_amdgcn_exp2f((sp - side.m[q]) * cexp) * side.il[q];
            ds[v] = 0.125f * (p[v] * (dP[v] - side.dl[q]));
        }
        // dv^T[d][key] += r(dO)^T[d][q] r(P)[q][key], dk^T[d][key] += Q^T[d][q] r(dS')[q][key]
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) {
            const a16_bf16x8 pB = a16_pack(p + 8 * ks), dsB = a16_pack(ds + 8 * ks);
            dV[0] = MFMA_BF16(a16_col(sD[buf], lane, 0, ks), pB, dV[0]);
            dV[1] = MFMA_BF16(a16_col(sD[buf], lane, 32, ks), pB, dV[1]);
            dK[0] = MFMA_BF16(a16_col(sQ[buf], lane, 0, ks), dsB, dK[0]);
            dK[1] = MFMA_BF16(a16_col(sQ[buf], lane, 32, ks), dsB, dK[1]);
        }
        if (qt + 1 < 32) store_tile(buf ^ 1);
        __syncthreads();
    }
    float *krow = dqkv + (tok0 + kh * 32 + r) * 3072 + 1024 + head * 64, *vrow = krow + 1024;
#pragma unroll
    for (int db = 0; db < 2; ++db)
#pragma unroll
        for (int g4 = 0; g4 < 4; ++g4) {
            const int d = db * 32 + 8 * g4 + 4 * h2;
            *reinterpret_cast<float4 *>(krow + d) = make_float4(dK[db][4 * g4], dK[db][4 * g4 + 1], dK[db][4 * g4 + 2], dK[db][4 * g4 + 3]);
            *reinterpret_cast<float4 *>(vrow + d) = make_float4(dV[db][4 * g4], dV[db][4 * g4 + 1], dV[db][4 * g4 + 2], dV[db][4 * g4 + 3]);
        }
}

// the workspace is cpx_attention_backward's (cpx_attn_bwd_layout): the two modes of the blocks' backward share one region
extern "C" size_t cpx_attention_backward_bf16_workspace_bytes(int n_subtiles) {
    if (n_subtiles <= 0 || n_subtiles > 16383) return 0;
    return cpx_attn_bwd_layout(n_subtiles).total;
}

int cpx_attention_backward_bf16_run(const void *qkv, const void *rel_h, const void *rel_w, const float *dO, int nS, float *dqkv, float *drel_h,
                                    float *drel_w, int add_rel, void *workspace, size_t workspace_bytes, void *stream) {
    CPX_REQUIRE(qkv && rel_h && rel_w && dO && dqkv && drel_h && drel_w && workspace);
    CPX_REQUIRE(nS > 0 && nS <= 16383);
    const AttnBwdLayout L = cpx_attn_bwd_layout(nS);
    CPX_REQUIRE(workspace_bytes >= L.total && ((uintptr_t)workspace & 255) == 0);
    CPX_REQUIRE((((uintptr_t)qkv | (uintptr_t)rel_h | (uintptr_t)rel_w | (uintptr_t)dO | (uintptr_t)dqkv) & 15) == 0);
    CPX_REQUIRE((((uintptr_t)drel_h | (uintptr_t)drel_w) & 3) == 0);
    char *ws = (char *)workspace;
    float *st_m = (float *)(ws + L.off_st[0]), *st_il = (float *)(ws + L.off_st[1]), *st_dl = (float *)(ws + L.off_st[2]);
    float *Bh = (float *)(ws + L.off_b[0]), *Bw = (float *)(ws + L.off_b[1]), *Gh = (float *)(ws + L.off_b[2]), *Gw = (float *)(ws + L.off_b[3]);
    hipStream_t s = (hipStream_t)stream;
    const dim3 grid(8, 16, nS), block(256);
    const unsigned short *q16 = (const unsigned short *)qkv;
    hipLaunchKernelGGL(k_attn_bwd16_dq, grid, block, 0, s, q16, (const unsigned short *)rel_h, (const unsigned short *)rel_w, dO, dqkv, st_m, st_il,
                       st_dl, Bh, Bw, Gh, Gw);
    CPX_CHECK_LAUNCH();
    hipLaunchKernelGGL(k_attn_bwd16_dkv, grid, block, 0, s, q16, dO, st_m, st_il, st_dl, Bh, Bw, dqkv);
    CPX_CHECK_LAUNCH();
    return cpx_attn_rel_grad_run(CPX_DT_BF16, qkv, Gh, Gw, (double *)(ws + L.off_part), nS, add_rel, drel_h, drel_w, stream);
}
extern "C" int cpx_attention_backward_bf16(const void *qkv, const void *rel_h, const void *rel_w, const float *dO, int n_subtiles, float *dqkv,
                                           float *drel_h, float *drel_w, void *workspace, size_t workspace_bytes, void *stream) {
    return cpx_attention_backward_bf16_run(qkv, rel_h, rel_w, dO, n_subtiles, dqkv, drel_h, drel_w, 0, workspace, workspace_bytes, stream);
}
