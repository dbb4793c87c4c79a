// Training the transformer blocks (gfx950): the backward kernels a block needs beyond the GEMMs and LayerNorm of the neck's backward.
//   * cpx_attention_backward   the derivative of the function cpx_attention(CPX_DT_F32, ...) computes (k_attention_f32, cpx_net_f32.hip:
//                              flash_forward with the decomposed rel-pos bias, vit_sam.py:15-65), in float32 on v_mfma_f32_32x32x2_f32
//   * cpx_gelu_backward        the erf GELU of the mlp.lin1 epilogue
// (cpx_layernorm_backward, cpx_train_neck.hip, takes the blocks' C = 1024 as well.)
//
// Attention, per (crop, head): Q, K, V [1024][64] from the stored qkv rows (widened exactly), tables Rh, Rw [64][64] in the operand
// convention of cpx_block_weights.rel_h / rel_w (rel_pos / scale, row 63 zero).  With query i = (qy, qx) and key j = (ky, kx):
//   S'[i][j] = q_i . (k_j + Rh[qy - ky + 31] + Rw[qx - kx + 31]),   P = softmax_j(scale S'),   O = P V,   scale = 64^-1/2
// (the scale multiplies the bias too: that is why the tables hold rel_pos / scale).  The derivative (tests/block_train_reference.py,
// attention_backward, pinned on float64 autograd by tests/test_block_train_host.py):
//   delta_i = dO_i . O_i = sum_j P[i][j] dP[i][j],   dP[i][j] = dO_i . v_j,   dS'[i][j] = scale P[i][j] (dP[i][j] - delta_i)
//   dv_j = sum_i P[i][j] dO_i,   dk_j = sum_i dS'[i][j] q_i
//   G_h[i][ky] = sum_kx dS'[i][(ky, kx)],   G_w[i][kx] = sum_ky dS'[i][(ky, kx)]
//   dq_i = sum_j dS'[i][j] k_j + sum_ky G_h[i][ky] Rh[qy - ky + 31] + sum_kx G_w[i][kx] Rw[qx - kx + 31]
//   dRh[r] = sum over crops, heads, i, ky with qy - ky + 31 = r of G_h[i][ky] q_i        (dRw likewise with qx, kx)
// Three kernels, no atomics, every sum in a fixed order:
//   k_attn_bwd_dq    one wave = one image row of 32 queries (the forward's shape).  Pass 1 over the 32 key tiles: the row maximum m and
//                    the sum l of exp(scale (S' - m)) and delta; pass 2: P recomputed, dS', dq, G_h, G_w.  It leaves m, 1 / l, delta and the bias
//                    values q_i . Rh[..], q_i . Rw[..] for the second kernel.
//   k_attn_bwd_dkv   one wave = one image row of 32 keys, looping over the 32 query tiles: P and dS' recomputed, dk and dv.
//   k_rel_grad       per (crop, four heads, table row): float64 sums in query order; k_rel_finish adds the partials in crop order and
//                    rounds once (row 63, the padding row, is written as zero).
// No query of one crop sees a key of another: every tile index is taken inside the crop's 1024 rows.
//
// The host drivers behind the exported block-training entries, each ONE body: blocks_forward_run (both forwards: one per-block step, with or
// without a layer-drop mask) and blocks_backward_run (all five backwards: one block walk over one precision-dependent Linear layer).
#include "cpx_internal.h"
#include <algorithm>

#define AB_LD 68                        // tile row stride in floats (k_attention_f32's: b128 reads of 16 rows cover all banks)
#define AB_GLD 97                       // per-query scratch row: [0, 64) q . table rows, [64, 96) the G_h sums
#define AB_SLOT(v, h2) (((v) & 3) + 8 * ((v) >> 2) + 4 * (h2))      // the row of accumulator register v in lane half h2

// ---------------------------------------------------------------------------
// dq, the row statistics and the row-group sums of dS'
// ---------------------------------------------------------------------------
// grid (8 row groups, 16 heads, crops), 4 waves: wave w of row group g owns the image row qh = 4 g + w.  Lane (r, h2): query qx = r,
// head channels 32 h2 .. 32 h2 + 31 of Q and dO; accumulator register v belongs to key kx = AB_SLOT(v, h2) of the tile (S'^T, dP^T)
// or to channel AB_SLOT(v, h2) (dq^T), as in k_attention_f32.  st_*, Bh, Bw, Gh, Gw are indexed by (crop * 16 + head) * 1024 + query.
template <int DT>
__global__ void __launch_bounds__(256) k_attn_bwd_dq(const void *__restrict__ qkv, const void *__restrict__ relh, const void *__restrict__ relw,
                                                     const float *__restrict__ dO, float *__restrict__ dqkv,
                                                     float *__restrict__ st_m, float *__restrict__ st_il, float *__restrict__ st_delta,
                                                     float *__restrict__ Bh, float *__restrict__ Bw, float *__restrict__ Gh,
                                                     float *__restrict__ Gw) {
    // 84 480 bytes of static LDS (sK + sV + sG): above the 64 KB of older CDNA parts, inside gfx950's 160 KB per workgroup -- this
    // kernel is gfx950-only, like the library
    __shared__ __attribute__((aligned(16))) float sK[2][32 * AB_LD];
    __shared__ __attribute__((aligned(16))) float sV[2][32 * AB_LD];
    __shared__ float sG[4][32 * AB_GLD];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int r = lane & 31, h2 = lane >> 5;
    const int head = blockIdx.y, s = blockIdx.z, qh = blockIdx.x * 4 + wave;
    const size_t tok0 = (size_t)s * 1024;
    const size_t qi = ((size_t)s * 16 + head) * 1024 + qh * 32 + r;

    float qf[32], dof[32];
    {
        const size_t qo = (tok0 + qh * 32 + r) * 3072 + head * 64 + 32 * h2, oo = (tok0 + qh * 32 + r) * 1024 + head * 64 + 32 * h2;
#pragma unroll
        for (int c = 0; c < 8; ++c) {
            const float4 a = ld4<DT>(qkv, qo + 4 * c);
            qf[4 * c] = a.x; qf[4 * c + 1] = a.y; qf[4 * c + 2] = a.z; qf[4 * c + 3] = a.w;
            const float4 d = *reinterpret_cast<const float4 *>(dO + oo + 4 * c);
            dof[4 * c] = d.x; dof[4 * c + 1] = d.y; dof[4 * c + 2] = d.z; dof[4 * c + 3] = d.w;
        }
    }
    // G[q][j] = q . table[j] -> the wave's scratch
    float *G = sG[wave];
    auto compute_G = [&](const void *table) {
#pragma unroll
        for (int jb = 0; jb < 2; ++jb) {
            f32x16 acc;
#pragma unroll
            for (int v = 0; v < 16; ++v) acc[v] = 0.f;
            const size_t to = (size_t)(jb * 32 + r) * 64 + 32 * h2;
#pragma unroll
            for (int c = 0; c < 8; ++c) {
                const float4 t4 = ld4<DT>(table, to + 4 * c);
                acc = MFMA_F32(t4.x, qf[4 * c], acc); acc = MFMA_F32(t4.y, qf[4 * c + 1], acc);
                acc = MFMA_F32(t4.z, qf[4 * c + 2], acc); acc = MFMA_F32(t4.w, qf[4 * c + 3], acc);
            }
#pragma unroll
            for (int v = 0; v < 16; ++v) G[r * AB_GLD + jb * 32 + AB_SLOT(v, h2)] = acc[v];
        }
        // G belongs to this wave alone, and its lane halves read each other's stores: a wave's LDS operations complete in order; the
        // wave barrier keeps the compiler from moving a load above these stores
        __builtin_amdgcn_wave_barrier();
    };
    compute_G(relw);
    f32x16 GW;
#pragma unroll
    for (int v = 0; v < 16; ++v) GW[v] = G[r * AB_GLD + (r - AB_SLOT(v, h2) + 31)];
#pragma unroll
    for (int g4 = 0; g4 < 4; ++g4)
        *reinterpret_cast<float4 *>(Bw + qi * 32 + 8 * g4 + 4 * h2) = make_float4(GW[4 * g4], GW[4 * g4 + 1], GW[4 * g4 + 2], GW[4 * g4 + 3]);
    __builtin_amdgcn_wave_barrier();                                   // the reads of q . Rw above, before q . Rh overwrites them
    compute_G(relh);
#pragma unroll
    for (int k = 0; k < 16; ++k) Bh[qi * 32 + h2 * 16 + k] = G[r * AB_GLD + (qh - (h2 * 16 + k) + 31)];

    // K / V tiles: 32 keys x 64 channels, thread -> (key = tid >> 4 (+ 16), 4 channels at (tid & 15) * 4)
    const int skey = tid >> 4, sc4 = (tid & 15) * 4;
    const size_t kbase = (tok0 + skey) * 3072 + 1024 + head * 64 + sc4, vbase = kbase + 1024;
    const int sdst0 = skey * AB_LD + sc4, sdst1 = sdst0 + 16 * AB_LD;
    float4 k0r, k1r, v0r, v1r;
    auto load_k = [&](int kh) {
        const size_t o = (size_t)kh * 32 * 3072;
        k0r = ld4<DT>(qkv, kbase + o); k1r = ld4<DT>(qkv, kbase + o + (size_t)16 * 3072);
    };
    auto load_v = [&](int kh) {
        const size_t o = (size_t)kh * 32 * 3072;
        v0r = ld4<DT>(qkv, vbase + o); v1r = ld4<DT>(qkv, vbase + o + (size_t)16 * 3072);
    };
    auto store_k = [&](int buf) {
        *reinterpret_cast<float4 *>(&sK[buf][sdst0]) = k0r; *reinterpret_cast<float4 *>(&sK[buf][sdst1]) = k1r;
    };
    auto store_v = [&](int buf) {
        *reinterpret_cast<float4 *>(&sV[buf][sdst0]) = v0r; *reinterpret_cast<float4 *>(&sV[buf][sdst1]) = v1r;
    };
    // S'^T = K . Q^T + the Rw bias (the Rh bias gh is one number per query and tile)
    auto scores = [&](int buf) {
        f32x16 S = GW;
        const float *kp = &sK[buf][r * AB_LD + 32 * h2];
#pragma unroll
        for (int c = 0; c < 8; ++c) {
            const float4 kf = *reinterpret_cast<const float4 *>(kp + 4 * c);
            S = MFMA_F32(kf.x, qf[4 * c], S); S = MFMA_F32(kf.y, qf[4 * c + 1], S);
            S = MFMA_F32(kf.z, qf[4 * c + 2], S); S = MFMA_F32(kf.w, qf[4 * c + 3], S);
        }
        return S;
    };
    // dP^T = V . dO^T
    auto dprobs = [&](int buf) {
        f32x16 dP;
#pragma unroll
        for (int v = 0; v < 16; ++v) dP[v] = 0.f;
        const float *vp = &sV[buf][r * AB_LD + 32 * h2];
#pragma unroll
        for (int c = 0; c < 8; ++c) {
            const float4 vf = *reinterpret_cast<const float4 *>(vp + 4 * c);
            dP = MFMA_F32(vf.x, dof[4 * c], dP); dP = MFMA_F32(vf.y, dof[4 * c + 1], dP);
            dP = MFMA_F32(vf.z, dof[4 * c + 2], dP); dP = MFMA_F32(vf.w, dof[4 * c + 3], dP);
        }
        return dP;
    };
    const float cexp = 0.125f * 1.44269504088896340736f;      // scale * log2(e)

    // pass 1: m = max_j S'[i][j], l = sum_j exp(scale (S'[i][j] - m)) and delta = sum_j P[i][j] dP[i][j] (= dO_i . O_i with the O of THIS
    // arithmetic: the stored O is rounded to the network dtype, and 2^-9 in delta would be 2^-9 in every dS')
    float m_run = -1e30f, l_run = 0.f, d_run = 0.f;
    load_k(0); load_v(0);
    store_k(0); store_v(0);
    __syncthreads();
    for (int kh = 0; kh < 32; ++kh) {
        const int buf = kh & 1;
        if (kh + 1 < 32) { load_k(kh + 1); load_v(kh + 1); }
        const float gh = G[r * AB_GLD + (qh - kh + 31)];
        const f32x16 S = scores(buf);
        const f32x16 dP = dprobs(buf);
        float mx = S[0];
#pragma unroll
        for (int v = 1; v < 16; ++v) mx = fmaxf(mx, S[v]);
        mx = fmaxf(mx, __shfl_xor(mx, 32)) + gh;
        const float m_new = fmaxf(m_run, mx);
        const float alpha = __builtin_amdgcn_exp2f((m_run - m_new) * cexp);
        m_run = m_new;
        // (S' - m) first, then the one multiplication: S' reaches hundreds, and a product S' * cexp rounded at that size would put its
        // rounding into every exponent; the difference is small where P is not
        const float off = gh - m_new;
        float ps = 0.f, pd = 0.f;
#pragma unroll
        for (int v = 0; v < 16; ++v) { const float p = __builtin_amdgcn_exp2f((S[v] + off) * cexp); ps += p; pd = fmaf(p, dP[v], pd); }
        l_run = fmaf(l_run, alpha, ps);
        d_run = fmaf(d_run, alpha, pd);
        if (kh + 1 < 32) { store_k(buf ^ 1); store_v(buf ^ 1); }
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
    load_k(0); load_v(0);
    store_k(0); store_v(0);
    __syncthreads();
    for (int kh = 0; kh < 32; ++kh) {
        const int buf = kh & 1;
        if (kh + 1 < 32) { load_k(kh + 1); load_v(kh + 1); }
        const float gh = G[r * AB_GLD + (qh - kh + 31)];
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
        if (h2 == 0) G[r * AB_GLD + 64 + kh] = gsum;             // (read after the loop's last __syncthreads)
        // dq^T[d][q] += K^T[d][key] dS'^T[key][q]: the k-slot of step j is the key of accumulator register j
#pragma unroll
        for (int j = 0; j < 16; ++j) {
            const float *kp = &sK[buf][AB_SLOT(j, h2) * AB_LD + r];
            dQ[0] = MFMA_F32(kp[0], ds[j], dQ[0]);
            dQ[1] = MFMA_F32(kp[32], ds[j], dQ[1]);
        }
        if (kh + 1 < 32) { store_k(buf ^ 1); store_v(buf ^ 1); }
        __syncthreads();
    }
    // the row-group sums: G_w from the registers (through the scratch: both lane halves need all 32), G_h from the scratch
#pragma unroll
    for (int v = 0; v < 16; ++v) G[r * AB_GLD + AB_SLOT(v, h2)] = gw[v];
    __builtin_amdgcn_wave_barrier();                                   // both lane halves read all 32 below
#pragma unroll
    for (int g4 = 0; g4 < 4; ++g4) {
        *reinterpret_cast<float4 *>(Gw + qi * 32 + 8 * g4 + 4 * h2) = make_float4(gw[4 * g4], gw[4 * g4 + 1], gw[4 * g4 + 2], gw[4 * g4 + 3]);
        const float *gp = &G[r * AB_GLD + 64 + h2 * 16 + 4 * g4];
        *reinterpret_cast<float4 *>(Gh + qi * 32 + h2 * 16 + 4 * g4) = make_float4(gp[0], gp[1], gp[2], gp[3]);
    }
    // the bias term of dq: 32 table rows weighted by G_h (row index uniform in the wave), 32 weighted by G_w (row index per query)
    for (int k = 0; k < 32; ++k) {
        const float g_h = G[r * AB_GLD + 64 + k], g_w = G[r * AB_GLD + k];
        const size_t th = (size_t)(qh - k + 31) * 64, tw = (size_t)(r - k + 31) * 64;
#pragma unroll
        for (int db = 0; db < 2; ++db)
#pragma unroll
            for (int g4 = 0; g4 < 4; ++g4) {
                const int d = db * 32 + 8 * g4 + 4 * h2;
                const float4 a = ld4<DT>(relh, th + d), b = ld4<DT>(relw, tw + d);
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
// grid as above; wave w of row group g owns the key row kh = 4 g + w: lane (r, h2) holds key kx = r, channels 32 h2 .. of K and V, and
// accumulator register v belongs to query qx = AB_SLOT(v, h2) of the tile (S', dP) or to channel AB_SLOT(v, h2) (dk^T, dv^T).
template <int DT>
__global__ void __launch_bounds__(256) k_attn_bwd_dkv(const void *__restrict__ qkv, const float *__restrict__ dO, const float *__restrict__ st_m,
                                                      const float *__restrict__ st_il, const float *__restrict__ st_delta,
                                                      const float *__restrict__ Bh, const float *__restrict__ Bw, float *__restrict__ dqkv) {
    __shared__ __attribute__((aligned(16))) float sQ[32 * AB_LD];
    __shared__ __attribute__((aligned(16))) float sD[32 * AB_LD];
    __shared__ __attribute__((aligned(16))) float sBw[32 * 36];
    __shared__ float sBh[4][32], sM[32], sIl[32], sDl[32];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int r = lane & 31, h2 = lane >> 5;
    const int head = blockIdx.y, s = blockIdx.z, kh = blockIdx.x * 4 + wave;
    const size_t tok0 = (size_t)s * 1024;
    const size_t qi0 = ((size_t)s * 16 + head) * 1024;

    float kf[32], vf[32];
    {
        const size_t ko = (tok0 + kh * 32 + r) * 3072 + 1024 + head * 64 + 32 * h2;
#pragma unroll
        for (int c = 0; c < 8; ++c) {
            const float4 a = ld4<DT>(qkv, ko + 4 * c), b = ld4<DT>(qkv, ko + 1024 + 4 * c);
            kf[4 * c] = a.x; kf[4 * c + 1] = a.y; kf[4 * c + 2] = a.z; kf[4 * c + 3] = a.w;
            vf[4 * c] = b.x; vf[4 * c + 1] = b.y; vf[4 * c + 2] = b.z; vf[4 * c + 3] = b.w;
        }
    }
    f32x16 dK[2], dV[2];
#pragma unroll
    for (int v = 0; v < 16; ++v) { dK[0][v] = 0.f; dK[1][v] = 0.f; dV[0][v] = 0.f; dV[1][v] = 0.f; }
    const int sq = tid >> 4, sc4 = (tid & 15) * 4;
    const float cexp = 0.125f * 1.44269504088896340736f;
    for (int qt = 0; qt < 32; ++qt) {
        __syncthreads();                                   // the previous tile has been read
        {
            const size_t row = tok0 + qt * 32 + sq;
            *reinterpret_cast<float4 *>(&sQ[sq * AB_LD + sc4]) = ld4<DT>(qkv, row * 3072 + head * 64 + sc4);
            *reinterpret_cast<float4 *>(&sQ[(sq + 16) * AB_LD + sc4]) = ld4<DT>(qkv, (row + 16) * 3072 + head * 64 + sc4);
            *reinterpret_cast<float4 *>(&sD[sq * AB_LD + sc4]) = *reinterpret_cast<const float4 *>(dO + row * 1024 + head * 64 + sc4);
            *reinterpret_cast<float4 *>(&sD[(sq + 16) * AB_LD + sc4]) = *reinterpret_cast<const float4 *>(dO + (row + 16) * 1024 + head * 64 + sc4);
            const int bq = tid >> 3, bc = (tid & 7) * 4;   // the Rw bias of the tile: 32 queries x 32 kx
            *reinterpret_cast<float4 *>(&sBw[bq * 36 + bc]) = *reinterpret_cast<const float4 *>(Bw + (qi0 + qt * 32 + bq) * 32 + bc);
            if (tid < 128) sBh[tid >> 5][tid & 31] = Bh[(qi0 + qt * 32 + (tid & 31)) * 32 + blockIdx.x * 4 + (tid >> 5)];
            else if (tid < 160) sM[tid - 128] = st_m[qi0 + qt * 32 + tid - 128];
            else if (tid < 192) sIl[tid - 160] = st_il[qi0 + qt * 32 + tid - 160];
            else if (tid < 224) sDl[tid - 192] = st_delta[qi0 + qt * 32 + tid - 192];
        }
        __syncthreads();
        // S'[q][key] = Q . K^T and dP[q][key] = dO . V^T
        f32x16 S, dP;
#pragma unroll
        for (int v = 0; v < 16; ++v) { S[v] = 0.f; dP[v] = 0.f; }
        const float *qp = &sQ[r * AB_LD + 32 * h2], *dp = &sD[r * AB_LD + 32 * h2];
#pragma unroll
        for (int c = 0; c < 8; ++c) {
            const float4 a = *reinterpret_cast<const float4 *>(qp + 4 * c), d = *reinterpret_cast<const float4 *>(dp + 4 * c);
            S = MFMA_F32(a.x, kf[4 * c], S); S = MFMA_F32(a.y, kf[4 * c + 1], S);
            S = MFMA_F32(a.z, kf[4 * c + 2], S); S = MFMA_F32(a.w, kf[4 * c + 3], S);
            dP = MFMA_F32(d.x, vf[4 * c], dP); dP = MFMA_F32(d.y, vf[4 * c + 1], dP);
            dP = MFMA_F32(d.z, vf[4 * c + 2], dP); dP = MFMA_F32(d.w, vf[4 * c + 3], dP);
        }
        float p[16], ds[16];
#pragma unroll
        for (int v = 0; v < 16; ++v) {
            const int q = AB_SLOT(v, h2);
            const float sp = (S[v] + sBw[q * 36 + r]) + sBh[wave][q];
            p[v] = __builtin_amdgcn_exp2f((sp - sM[q]) * cexp) * sIl[q];
            ds[v] = 0.125f * (p[v] * (dP[v] - sDl[q]));
        }
        // dv^T[d][key] += dO^T[d][q] P[q][key], dk^T[d][key] += Q^T[d][q] dS'[q][key]: the k-slot of step j is the query of register j
#pragma unroll
        for (int j = 0; j < 16; ++j) {
            const int o = AB_SLOT(j, h2) * AB_LD + r;
            dV[0] = MFMA_F32(sD[o], p[j], dV[0]);
            dV[1] = MFMA_F32(sD[o + 32], p[j], dV[1]);
            dK[0] = MFMA_F32(sQ[o], ds[j], dK[0]);
            dK[1] = MFMA_F32(sQ[o + 32], ds[j], dK[1]);
        }
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

// ---------------------------------------------------------------------------
// the gradients of the two tables
// ---------------------------------------------------------------------------
// grid (63 table rows, 2 tables, crops * 4), 4 waves: wave w takes head 4 * (blockIdx.z & 3) + w, lane d one channel.  Table 0 (Rh):
// the pairs (a, b) = (qy, ky) with qy - ky + 31 = row, summed over qx; table 1 (Rw): (a, b) = (qx, kx), summed over qy.  One float64
// chain per thread in (a, c) order, then wave 0 + 1 + 2 + 3 -> part [crops * 4][2][64][64] float64 (row 63 is never written or read).
template <int DT>
__global__ void __launch_bounds__(256) k_rel_grad(const void *__restrict__ qkv, const float *__restrict__ Gh, const float *__restrict__ Gw,
                                                  double *__restrict__ part) {
    __shared__ double sm[4][64];
    const int d = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int row = blockIdx.x, t = blockIdx.y, s = blockIdx.z >> 2, head = (blockIdx.z & 3) * 4 + wave;
    const float *G = t ? Gw : Gh;
    const size_t qi0 = ((size_t)s * 16 + head) * 1024, tok0 = (size_t)s * 1024;
    double acc = 0;
    for (int a = 0; a < 32; ++a) {
        const int b = a - row + 31;
        if (b < 0 || b >= 32) continue;                    // (uniform in the workgroup)
#pragma unroll 8
        for (int c = 0; c < 32; ++c) {
            const int i = t ? c * 32 + a : a * 32 + c;
            acc += (double)G[(qi0 + i) * 32 + b] * (double)load_f32<DT>(qkv, (tok0 + i) * 3072 + head * 64 + d);
        }
    }
    sm[wave][d] = acc;
    __syncthreads();
    if (wave == 0) part[(((size_t)blockIdx.z * 2 + t) * 64 + row) * 64 + d] = ((sm[0][d] + sm[1][d]) + sm[2][d]) + sm[3][d];
}
// thread = one element of [2][64][64]: the partials in chunk order; `add`: on top of what the output holds (a later slab of crops)
__global__ void __launch_bounds__(256) k_rel_finish(const double *__restrict__ part, int nchunk, int add, float *__restrict__ drel_h,
                                                    float *__restrict__ drel_w) {
    const int e = blockIdx.x * 256 + threadIdx.x, t = e >> 12, o = e & 4095;
    float *out = (t ? drel_w : drel_h) + o;
    if ((o >> 6) == 63) { *out = 0.f; return; }
    double sum = add ? (double)*out : 0.0;
    for (int k = 0; k < nchunk; ++k) sum += part[((size_t)k * 2 + t) * 4096 + o];
    *out = (float)sum;
}

int cpx_attn_rel_grad_run(int dtype, const void *qkv, const float *Gh, const float *Gw, double *part, int nS, int add_rel, float *drel_h,
                          float *drel_w, void *stream) {
    hipStream_t s = (hipStream_t)stream;
    const dim3 block(256);
    CPX_DT_DISPATCH(dtype, DT, hipLaunchKernelGGL(k_rel_grad<DT>, dim3(63, 2, nS * 4), block, 0, s, qkv, Gh, Gw, part));
    CPX_CHECK_LAUNCH();
    hipLaunchKernelGGL(k_rel_finish, dim3(32), block, 0, s, part, nS * 4, add_rel, drel_h, drel_w);
    CPX_CHECK_LAUNCH();
    return CPX_OK;
}

// workspace: cpx_attn_bwd_layout (cpx_internal.h)
extern "C" size_t cpx_attention_backward_workspace_bytes(int n_subtiles) {
    if (n_subtiles <= 0 || n_subtiles > 16383) return 0;              // blockIdx.z = 4 * crops in k_rel_grad
    return cpx_attn_bwd_layout(n_subtiles).total;
}

// `add_rel`: drel_h / drel_w receive their sums on top of what they hold (the caller runs a batch in slabs of crops, in order)
int cpx_attention_backward_run(int dtype, const void *qkv, const void *rel_h, const void *rel_w, const void *O, const float *dO, int nS,
                               float *dqkv, float *drel_h, float *drel_w, int add_rel, void *workspace, size_t workspace_bytes,
                               void *stream) {
    CPX_REQUIRE(qkv && rel_h && rel_w && dO && dqkv && drel_h && drel_w && workspace && dtype_ok(dtype));
    (void)O;                                   // not read: delta comes from the recomputed P (k_attn_bwd_dq, pass 1)
    CPX_REQUIRE(nS > 0 && nS <= 16383);
    const AttnBwdLayout L = cpx_attn_bwd_layout(nS);
    CPX_REQUIRE(workspace_bytes >= L.total && ((uintptr_t)workspace & 255) == 0);
    CPX_REQUIRE((((uintptr_t)qkv | (uintptr_t)rel_h | (uintptr_t)rel_w | (uintptr_t)O | (uintptr_t)dO | (uintptr_t)dqkv) & 15) == 0);
    char *ws = (char *)workspace;
    float *st_m = (float *)(ws + L.off_st[0]), *st_il = (float *)(ws + L.off_st[1]), *st_dl = (float *)(ws + L.off_st[2]);
    float *Bh = (float *)(ws + L.off_b[0]), *Bw = (float *)(ws + L.off_b[1]), *Gh = (float *)(ws + L.off_b[2]), *Gw = (float *)(ws + L.off_b[3]);
    double *part = (double *)(ws + L.off_part);
    hipStream_t s = (hipStream_t)stream;
    const dim3 grid(8, 16, nS), block(256);
    CPX_DT_DISPATCH(dtype, DT, hipLaunchKernelGGL(k_attn_bwd_dq<DT>, grid, block, 0, s, qkv, rel_h, rel_w, dO, dqkv, st_m, st_il, st_dl, Bh, Bw, Gh, Gw));
    CPX_CHECK_LAUNCH();
    CPX_DT_DISPATCH(dtype, DT, hipLaunchKernelGGL(k_attn_bwd_dkv<DT>, grid, block, 0, s, qkv, dO, st_m, st_il, st_dl, Bh, Bw, dqkv));
    CPX_CHECK_LAUNCH();
    return cpx_attn_rel_grad_run(dtype, qkv, Gh, Gw, part, nS, add_rel, drel_h, drel_w, stream);
}
extern "C" int cpx_attention_backward(int dtype, const void *qkv, const void *rel_h, const void *rel_w, const void *O, const float *dO,
                                      int n_subtiles, float *dqkv, float *drel_h, float *drel_w, void *workspace, size_t workspace_bytes,
                                      void *stream) {
    return cpx_attention_backward_run(dtype, qkv, rel_h, rel_w, O, dO, n_subtiles, dqkv, drel_h, drel_w, 0, workspace, workspace_bytes, stream);
}

// ---------------------------------------------------------------------------
// GELU backward
// ---------------------------------------------------------------------------
// gelu(x) = x Phi(x), Phi(x) = erfc(-x / sqrt 2) / 2 (erfc, not 1 + erf: no cancellation in the left tail), so
// gelu'(x) = Phi(x) + x phi(x), phi(x) = exp(-x^2 / 2) / sqrt(2 pi): 0 at -inf, 1 at +inf, never NaN for finite x
__global__ void __launch_bounds__(256) k_gelu_bwd(const float *__restrict__ pre, const float *__restrict__ dh, size_t n4, float *__restrict__ dpre) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n4) return;
    const float4 x = *reinterpret_cast<const float4 *>(pre + 4 * i), g = *reinterpret_cast<const float4 *>(dh + 4 * i);
    auto dg = [](float v) {
        const float Phi = 0.5f * erfcf(-v * 0.70710678118654752440f);
        const float phi = 0.39894228040143267794f * expf(-0.5f * v * v);
        return fmaf(v, phi, Phi);
    };
    *reinterpret_cast<float4 *>(dpre + 4 * i) = make_float4(g.x * dg(x.x), g.y * dg(x.y), g.z * dg(x.z), g.w * dg(x.w));
}
extern "C" int cpx_gelu_backward(const float *pre, const float *dh, size_t n, float *dpre, void *stream) {
    CPX_REQUIRE(pre && dh && dpre && n > 0 && n % 4 == 0 && n / 4 / 256 < 0x7fffffffull);
    CPX_REQUIRE((((uintptr_t)pre | (uintptr_t)dh | (uintptr_t)dpre) & 15) == 0);
    const size_t n4 = n / 4;
    hipLaunchKernelGGL(k_gelu_bwd, dim3((unsigned)((n4 + 255) / 256)), dim3(256), 0, (hipStream_t)stream, pre, dh, n4, dpre);
    CPX_CHECK_LAUNCH();
    return CPX_OK;
}

// ---------------------------------------------------------------------------
// the workspace of the training forward of the last K blocks
// ---------------------------------------------------------------------------
// workspace: per trained block j (block first_block + j) [x_in [M][1024]][qkv [M][3072]][ao [M][1024]][x_mid [M][1024]] in the network
// dtype -- the block's input, its qkv rows, the attention output and the rows after the attention residual --, then x_out [M][1024],
// the last block's output, then the workspace of cpx_neck_forward_train, then what the forward only passes through (V^T, the hidden
// activations, the LayerNorm output of the unfused half path, the row statistics of the fused one).  Nothing kept is overwritten.
// The backward recomputes in float32 from the kept tensors: both LayerNorm outputs, the lin1 pre-activation, the hidden activations
// (rounded to the network dtype, as the forward rounds them) and the softmax.
struct BlocksFwdLayout { size_t stride, o_x, o_qkv, o_ao, o_mid, off_out, off_neck, neck_bytes, off_vt, off_h, off_xn, off_st, total; };
static BlocksFwdLayout blocks_fwd_layout(int nS, int dtype, int K) {
    BlocksFwdLayout L; CpxArena a; const size_t M = (size_t)nS * 1024, es = es_of(dtype);
    L.o_x = a.take(M * 1024 * es); L.o_qkv = a.take(M * 3072 * es); L.o_ao = a.take(M * 1024 * es); L.o_mid = a.take(M * 1024 * es);
    L.stride = a.o;
    a.o = L.stride * (size_t)K;
    L.off_out = a.take(M * 1024 * es);
    L.neck_bytes = cpx_neck_train_workspace_bytes(nS, dtype);
    L.off_neck = a.take(L.neck_bytes);
    L.off_vt = a.take(es == 2 ? M * 1024 * es : 0);
    L.off_h = a.take(M * 4096 * es);
    L.off_xn = a.take(M * 1024 * es);
    L.off_st = a.take(es == 2 ? M * 8 * sizeof(float) : 0);
    L.total = a.o;
    return L;
}
static bool blocks_args_ok(int nS, int dtype, int K) { return cpx_crops_ok(nS) && dtype_ok(dtype) && K > 0 && K <= 4096; }
// off [4 K + 2]: per trained block x_in, qkv, ao, x_mid; then x_out and the workspace of cpx_neck_forward_train
extern "C" int cpx_blocks_train_layout(int nS, int dtype, int K, size_t *off) {
    CPX_REQUIRE(blocks_args_ok(nS, dtype, K) && off);
    const BlocksFwdLayout L = blocks_fwd_layout(nS, dtype, K);
    for (int j = 0; j < K; ++j) {
        const size_t b = L.stride * (size_t)j;
        off[4 * j] = b + L.o_x; off[4 * j + 1] = b + L.o_qkv; off[4 * j + 2] = b + L.o_ao; off[4 * j + 3] = b + L.o_mid;
    }
    off[4 * K] = L.off_out; off[4 * K + 1] = L.off_neck;
    return CPX_OK;
}

// The half-precision qkv GEMM writes the V third transposed into vT [crop][channel 1024][token 1024] INSTEAD of the qkv rows
// (CPX_EPI_QKV_BF16): the kept qkv rows get their V columns from it, an exact copy.  grid (32 token tiles, 32 channel tiles, crops)
__global__ void __launch_bounds__(256) k_vt_to_rows(const unsigned short *__restrict__ vT, unsigned short *__restrict__ qkv) {
    __shared__ unsigned short t[32][33];
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5, t0 = blockIdx.x * 32, c0 = blockIdx.y * 32;
    const size_t s = blockIdx.z;
#pragma unroll
    for (int k = 0; k < 4; ++k) t[ty + 8 * k][tx] = vT[(s * 1024 + c0 + ty + 8 * k) * 1024 + t0 + tx];
    __syncthreads();
#pragma unroll
    for (int k = 0; k < 4; ++k) qkv[(s * 1024 + t0 + ty + 8 * k) * 3072 + 2048 + c0 + tx] = t[tx][ty + 8 * k];
}
static int vt_to_rows_run(const void *vT, void *qkv, int nS, hipStream_t s) {
    hipLaunchKernelGGL(k_vt_to_rows, dim3(32, 32, nS), dim3(256), 0, s, (const unsigned short *)vT, (unsigned short *)qkv);
    CPX_CHECK_LAUNCH();
    return CPX_OK;
}

static bool blocks_weights_ok(const cpx_net_weights *w, int first_block) {
    return w && dtype_ok(w->dtype) && w->blocks && w->depth > 0 && first_block >= 0 && first_block < w->depth &&
           (w->dtype != CPX_DT_F32 || !w->fuse_ln) && w->n_unet_ops == 0;
}

// ---------------------------------------------------------------------------
// crop lists (layer drop, stochastic depth: a block runs on its kept crops alone)
// ---------------------------------------------------------------------------
// The crops named by `crops` (host, n entries, strictly increasing, each < nS) between a full [nS * 1024][1024] buffer and a compact
// [n * 1024][1024] one, in list order from compact crop `first`; the list travels in the kernel arguments, CPX_CROP_LIST crops per launch.
static bool crop_list_ok(int dtype, int nS, const int *crops, int n) {
    if (!dtype_ok(dtype) || !cpx_crops_ok(nS) || n < 0 || n > nS || (n > 0 && !crops)) return false;
    for (int i = 0; i < n; ++i)
        if (crops[i] < 0 || crops[i] >= nS || (i > 0 && crops[i] <= crops[i - 1])) return false;
    return true;
}
static int move_crops(int dtype, const void *src, void *dst, const int *crops, int n, int first, int scatter, float *stats, hipStream_t s) {
    for (int i0 = 0; i0 < n; i0 += CPX_CROP_LIST) {
        CpxCropList l = {};
        l.n = std::min(CPX_CROP_LIST, n - i0); l.first = first + i0;
        for (int i = 0; i < l.n; ++i) l.crop[i] = crops[i0 + i];
        CPX_RUN(cpx_move_crop_rows_run(dtype, src, dst, l, scatter, stats, s));
    }
    return CPX_OK;
}
extern "C" int cpx_gather_crops(int dtype, const void *src, int nS, const int *crops, int n, void *dst, float *stats, void *stream) {
    CPX_REQUIRE(crop_list_ok(dtype, nS, crops, n) && (!stats || dtype != CPX_DT_F32));
    if (n == 0) return CPX_OK;
    CPX_REQUIRE(src && dst && (((uintptr_t)src | (uintptr_t)dst | (uintptr_t)stats) & 15) == 0);
    return move_crops(dtype, src, dst, crops, n, 0, 0, stats, (hipStream_t)stream);
}
extern "C" int cpx_scatter_crops(int dtype, const void *src, int nS, const int *crops, int n, void *dst, void *stream) {
    CPX_REQUIRE(crop_list_ok(dtype, nS, crops, n));
    if (n == 0) return CPX_OK;
    CPX_REQUIRE(src && dst && (((uintptr_t)src | (uintptr_t)dst) & 15) == 0);
    return move_crops(dtype, src, dst, crops, n, 0, 1, nullptr, (hipStream_t)stream);
}

// keep [K][nS], host: keep[j * nS + n] != 0 where block first_block + j runs on crop n.  true: some (block, crop) pair is dropped
static bool keep_drops(const unsigned char *keep, int K, int nS) {
    if (keep)
        for (size_t i = 0; i < (size_t)K * nS; ++i)
            if (!keep[i]) return true;
    return false;
}
// move_crops for the crops a mask row keeps, the list built CPX_CROP_LIST crops at a time (no allocation); *n_keep: how many there are
static int move_kept(int dtype, const unsigned char *kj, int nS, const void *src, void *dst, int scatter, float *stats, hipStream_t s, int *n_keep) {
    int crops[CPX_CROP_LIST], n = 0;
    *n_keep = 0;
    for (int c = 0; c < nS; ++c) {
        if (kj[c]) crops[n++] = c;
        if (n == CPX_CROP_LIST || c + 1 == nS) {
            CPX_RUN(move_crops(dtype, src, dst, crops, n, *n_keep, scatter, stats, s));
            *n_keep += n; n = 0;
        }
    }
    return CPX_OK;
}

// ---------------------------------------------------------------------------
// the training forward of the last K blocks: one body for both entries
// ---------------------------------------------------------------------------
// Trained block j (block first_block + j) on nc crops, from its x_in record into xout: cpx_net_block -- cpx_net_forward's launches in its
// order, with its MLP row parts --, every GEMM writing to a tensor of its own.  For the half types the V columns of the kept qkv rows are
// copied from vT afterwards: nothing reads them before the backward, and the next block's qkv GEMM overwrites vT.
static int block_forward_step(const cpx_net_weights *w, int first_block, int j, int nc, const BlocksFwdLayout &L, char *ws, void *xout, void *stream) {
    char *base = ws + L.stride * (size_t)j;
    const CpxBlockBufs t = {base + L.o_x, base + L.o_mid, xout, ws + L.off_xn, base + L.o_qkv, ws + L.off_vt, base + L.o_ao, ws + L.off_h,
                            (float *)(ws + L.off_st)};
    CPX_RUN(cpx_net_block(w, first_block + j, nc, t, cpx_net_big_stats(w, nc), nullptr, stream));
    if (w->dtype != CPX_DT_F32) CPX_RUN(vt_to_rows_run(t.vt, t.qkv, nc, (hipStream_t)stream));
    return CPX_OK;
}
static size_t blocks_fwd_bytes(int nS, int dtype, int K, bool drop) {
    if (!blocks_args_ok(nS, dtype, K)) return 0;
    // drop: the staging rows of a compacted block's output, behind the workspace as it is without a mask
    return blocks_fwd_layout(nS, dtype, K).total + (drop ? cpx_align_up((size_t)nS * 1024 * 1024 * es_of(dtype), 256) : 0);
}
// Blocks first_block .. depth - 1, then cpx_neck_forward_train.  keep NULL or all non-zero -- no mask: block j writes straight into block
// j + 1's x_in record (the last one into x_out).  Where cpx_net_forward takes a block's row statistics from the GEMM before it (the
// fused half path from 16 crops up), the FIRST trained block takes them from cpx_row_stats, as cpx_net_forward itself does below 16 crops.
// Under a mask, x_{j+1}[n] = keep[j][n] ? block_j(x_j[n]) : x_j[n].  No row of one crop meets a row of another inside a block, so block j
// runs on its kept crops alone: they are gathered, in crop order, out of the running full-batch rows -- the x_out record -- into the
// block's x_in record (with their row statistics where the weights fold LayerNorm: a compacted block has no GEMM before it to emit
// them), the block runs on n_keep crops into the staging rows, and those are scattered back.  qkv, ao and x_mid of block j hold
// n_keep_j * 1024 rows at the front of their records; a block that keeps nothing launches nothing.  The neck runs on all crops.
static int blocks_forward_run(const cpx_net_weights *w, const void *x, int nS, int first_block, const unsigned char *keep, float *head,
                              void *workspace, size_t workspace_bytes, void *stream) {
    CPX_REQUIRE(blocks_weights_ok(w, first_block) && x && head && workspace && blocks_args_ok(nS, w->dtype, w->depth - first_block));
    const int dt = w->dtype, K = w->depth - first_block, M = nS * 1024;
    if (!keep_drops(keep, K, nS)) keep = nullptr;
    const BlocksFwdLayout L = blocks_fwd_layout(nS, dt, K);
    CPX_REQUIRE(workspace_bytes >= blocks_fwd_bytes(nS, dt, K, keep != nullptr) && ((uintptr_t)workspace & 255) == 0 && ((uintptr_t)x & 15) == 0);
    char *ws = (char *)workspace, *state = ws + L.off_out, *stage = ws + L.total;
    hipStream_t hs = (hipStream_t)stream;
    float *st = (float *)(ws + L.off_st);
    CPX_HIP(hipMemcpyAsync(keep ? state : ws + L.o_x, x, (size_t)M * 1024 * es_of(dt), hipMemcpyDeviceToDevice, hs));
    if (!keep && w->fuse_ln) CPX_RUN(cpx_row_stats_half(dt, ws + L.o_x, M, st, stream));
    for (int j = 0; j < K; ++j) {
        char *xin = ws + L.stride * (size_t)j + L.o_x;
        if (!keep) {
            CPX_RUN(block_forward_step(w, first_block, j, nS, L, ws, j + 1 < K ? xin + L.stride : state, stream));
            continue;
        }
        const unsigned char *kj = keep + (size_t)j * nS;
        int nk = 0;
        CPX_RUN(move_kept(dt, kj, nS, state, xin, 0, w->fuse_ln ? st : nullptr, hs, &nk));
        if (!nk) continue;
        CPX_RUN(block_forward_step(w, first_block, j, nk, L, ws, stage, stream));
        CPX_RUN(move_kept(dt, kj, nS, stage, state, 1, nullptr, hs, &nk));
    }
    return cpx_neck_forward_train(w, state, nS, head, ws + L.off_neck, L.neck_bytes, stream);
}
extern "C" size_t cpx_blocks_train_workspace_bytes(int nS, int dtype, int K) { return blocks_fwd_bytes(nS, dtype, K, false); }
extern "C" size_t cpx_blocks_train_workspace_bytes_drop(int nS, int dtype, int K) { return blocks_fwd_bytes(nS, dtype, K, true); }
extern "C" int cpx_blocks_forward_train(const cpx_net_weights *w, const void *x, int nS, int first_block, float *head, void *workspace,
                                        size_t workspace_bytes, void *stream) {
    return blocks_forward_run(w, x, nS, first_block, nullptr, head, workspace, workspace_bytes, stream);
}
extern "C" int cpx_blocks_forward_train_drop(const cpx_net_weights *w, const void *x, int nS, int first_block, const unsigned char *keep,
                                             float *head, void *workspace, size_t workspace_bytes, void *stream) {
    return blocks_forward_run(w, x, nS, first_block, keep, head, workspace, workspace_bytes, stream);
}

// ---------------------------------------------------------------------------
// small kernels of the block backward
// ---------------------------------------------------------------------------
// LayerNorm over 1024 channels of a stored row, two-pass float32 statistics as k_layernorm_f32 -> float32; gamma == nullptr: xhat alone.
// ROUND: the result goes through the network dtype, as the unfused half forward stores it.
template <int DT, bool ROUND>
__global__ void __launch_bounds__(256) k_ln_fwd1024(const void *__restrict__ x, const float *__restrict__ gamma, const float *__restrict__ beta,
                                                    int rows, float eps, float *__restrict__ out) {
    const int lane = threadIdx.x & 63, row = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= rows) return;
    const size_t base = (size_t)row * 1024 + lane * 16;
    float v[16];
#pragma unroll
    for (int i = 0; i < 16; i += 4) { const float4 a = ld4<DT>(x, base + i); v[i] = a.x; v[i + 1] = a.y; v[i + 2] = a.z; v[i + 3] = a.w; }
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < 16; ++i) s += v[i];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
    const float mean = s * (1.0f / 1024);
    float q = 0.f;
#pragma unroll
    for (int i = 0; i < 16; ++i) { const float d = v[i] - mean; q += d * d; }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) q += __shfl_xor(q, o);
    const float rstd = 1.0f / sqrtf(q * (1.0f / 1024) + eps);
#pragma unroll
    for (int i = 0; i < 16; ++i) {
        float y = (v[i] - mean) * rstd;
        if (gamma) y = y * gamma[lane * 16 + i] + beta[lane * 16 + i];
        if constexpr (ROUND && DT == CPX_DT_BF16) y = bf16_to_f32(f32_to_bf16(y));
        if constexpr (ROUND && DT == CPX_DT_F16) y = (float)(_Float16)y;
        out[base + i] = y;
    }
}
// in [R][Cc] of element type DT -> out [Cc][R] float32, 32 x 32 tiles through LDS; R and Cc multiples of 32
template <int DT>
__global__ void __launch_bounds__(256) k_transpose_f32(const void *__restrict__ in, int R, int Cc, float *__restrict__ out) {
    __shared__ float t[32][33];
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5, r0 = blockIdx.y * 32, c0 = blockIdx.x * 32;
#pragma unroll
    for (int k = 0; k < 4; ++k) t[ty + 8 * k][tx] = load_f32<DT>(in, (size_t)(r0 + ty + 8 * k) * Cc + c0 + tx);
    __syncthreads();
#pragma unroll
    for (int k = 0; k < 4; ++k) out[(size_t)(c0 + ty + 8 * k) * R + r0 + tx] = t[tx][ty + 8 * k];
}
template <int DT>
__global__ void __launch_bounds__(256) k_widen_f32(const void *__restrict__ in, size_t n4, float *__restrict__ out) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n4) *reinterpret_cast<float4 *>(out + 4 * i) = ld4<DT>(in, 4 * i);
}
// h = gelu(pre) as the mlp.lin1 epilogue forms it, rounded through the network dtype as the forward stores it
template <int DT>
__global__ void __launch_bounds__(256) k_gelu_fwd_round(const float *__restrict__ pre, size_t n, float *__restrict__ h) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const float x = pre[i];
    float y = 0.5f * x * (1.0f + erff(x * 0.70710678118654752440f));
    if constexpr (DT == CPX_DT_BF16) y = bf16_to_f32(f32_to_bf16(y));
    if constexpr (DT == CPX_DT_F16) y = (float)(_Float16)y;
    h[i] = y;
}
// db[c] += sum over rows of dy[row][c]: one float64 chain per column in row order, added to what db holds, rounded once
__global__ void __launch_bounds__(256) k_colsum_add(const float *__restrict__ dy, int rows, int N, float *__restrict__ db) {
    const int c = blockIdx.x * 256 + threadIdx.x;
    if (c >= N) return;
    double s = 0;
#pragma unroll 8
    for (int r = 0; r < rows; ++r) s += (double)dy[(size_t)r * N + c];
    db[c] = (float)((double)db[c] + s);
}
// The same sums for the bf16 gradient mode, row-parallel.  grid (N / 64, rows / CS_ROWS), 4 waves: lane = one of 64 columns, wave w one
// float64 chain over the rows w, w + 4, ... of the workgroup's CS_ROWS rows in order, then (w0 + w1) + w2 + w3 -> part [rows / CS_ROWS][N];
// k_colsum_finish adds the partials in row order on top of db and rounds once.  A fixed tree per column: no atomics.
#define CS_ROWS 64
__global__ void __launch_bounds__(256) k_colsum_part(const float *__restrict__ dy, int N, double *__restrict__ part) {
    __shared__ double sm[4][64];
    const int l = threadIdx.x & 63, w = threadIdx.x >> 6, c = blockIdx.x * 64 + l;
    const float *p = dy + ((size_t)blockIdx.y * CS_ROWS + w) * N + c;
    double s = 0;
#pragma unroll
    for (int i = 0; i < CS_ROWS / 4; ++i) s += (double)p[(size_t)(4 * i) * N];
    sm[w][l] = s;
    __syncthreads();
    if (w == 0) part[(size_t)blockIdx.y * N + c] = ((sm[0][l] + sm[1][l]) + sm[2][l]) + sm[3][l];
}
__global__ void __launch_bounds__(256) k_colsum_finish(const double *__restrict__ part, int nparts, int N, float *__restrict__ db) {
    const int c = blockIdx.x * 256 + threadIdx.x;
    if (c >= N) return;
    double s = 0;
    for (int k = 0; k < nparts; ++k) s += part[(size_t)k * N + c];
    db[c] = (float)((double)db[c] + s);
}
extern "C" size_t cpx_colsum_workspace_bytes(int rows, int N) {
    if (rows <= 0 || N <= 0 || rows % CS_ROWS || N % 64 || rows / CS_ROWS > 65535) return 0;
    return cpx_align_up((size_t)(rows / CS_ROWS) * N * sizeof(double), 256);
}
extern "C" int cpx_colsum_add(const float *dy, int rows, int N, float *db, void *workspace, size_t workspace_bytes, void *stream) {
    CPX_REQUIRE(dy && db && workspace);
    const size_t need = cpx_colsum_workspace_bytes(rows, N);
    CPX_REQUIRE(need > 0 && workspace_bytes >= need && ((uintptr_t)workspace & 7) == 0);
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(k_colsum_part, dim3(N / 64, rows / CS_ROWS), dim3(256), 0, s, dy, N, (double *)workspace);
    CPX_CHECK_LAUNCH();
    hipLaunchKernelGGL(k_colsum_finish, grid1(N), dim3(256), 0, s, (const double *)workspace, rows / CS_ROWS, N, db);
    CPX_CHECK_LAUNCH();
    return CPX_OK;
}
// W [Npad][Kpad] of a 2-byte type -> wt [Kp128][Npad] of the same type, rows Kpad .. zero (cpx_wt_run's float32 result, kept in 2 bytes:
// the operand cpx_gemm_half takes for dX = dY W); 32 x 32 tiles through LDS, Npad and Kp128 multiples of 32
__global__ void __launch_bounds__(256) k_wt16(const unsigned short *__restrict__ w, int Npad, int Kpad, unsigned short *__restrict__ wt) {
    __shared__ unsigned short t[32][33];
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5, k0 = blockIdx.x * 32, n0 = blockIdx.y * 32;
#pragma unroll
    for (int k = 0; k < 4; ++k) t[ty + 8 * k][tx] = k0 + tx < Kpad ? w[(size_t)(n0 + ty + 8 * k) * Kpad + k0 + tx] : (unsigned short)0;
    __syncthreads();
#pragma unroll
    for (int k = 0; k < 4; ++k) wt[(size_t)(k0 + ty + 8 * k) * Npad + n0 + tx] = t[tx][ty + 8 * k];
}
static int wt16_run(const void *w, int Npad, int Kpad, int Kp128, void *wt, hipStream_t s) {
    CPX_REQUIRE(Npad % 32 == 0 && Kp128 % 32 == 0 && Kpad <= Kp128 && Npad / 32 <= 65535);
    hipLaunchKernelGGL(k_wt16, dim3(Kp128 / 32, Npad / 32), dim3(256), 0, s, (const unsigned short *)w, Npad, Kpad, (unsigned short *)wt);
    CPX_CHECK_LAUNCH();
    return CPX_OK;
}
// out = a + b (out may be a)
__global__ void __launch_bounds__(256) k_add_f32(const float *a, const float *b, size_t n4, float *out) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n4) return;
    const float4 x = *reinterpret_cast<const float4 *>(a + 4 * i), y = *reinterpret_cast<const float4 *>(b + 4 * i);
    *reinterpret_cast<float4 *>(out + 4 * i) = make_float4(x.x + y.x, x.y + y.y, x.z + y.z, x.w + y.w);
}

// Where LayerNorm is folded into the Linear (cpx_fold_layernorm: Wf = round(W diag(gamma)), bf = b + W beta), the backward differentiates
// what the forward multiplied by: the weight-gradient GEMM gives dWf = dpre^T xhat, and the chain rule through the fold (the rounding of
// Wf passed straight through) gives, in place and per column k with one float64 chain over the N rows in order:
//   dW[n][k] = dWf[n][k] gamma[k] + dbf[n] beta[k],   dgamma[k] = sum_n dWf[n][k] W[n][k],   dbeta[k] = sum_n dbf[n] W[n][k]   (db = dbf)
__global__ void __launch_bounds__(256) k_unfold_grads(float *__restrict__ dW, const float *__restrict__ dbf, const float *__restrict__ W,
                                                      const float *__restrict__ gamma, const float *__restrict__ beta, int N,
                                                      float *__restrict__ dgamma, float *__restrict__ dbeta) {
    const int k = blockIdx.x * 256 + threadIdx.x;                      // < 1024
    const float g = gamma[k], b = beta[k];
    double sg = 0, sb = 0;
#pragma unroll 4
    for (int n = 0; n < N; ++n) {
        const size_t i = (size_t)n * 1024 + k;
        const float dwf = dW[i], w = W[i], d = dbf[n];
        sg += (double)dwf * (double)w;
        sb += (double)d * (double)w;
        dW[i] = fmaf(dwf, g, d * b);
    }
    dgamma[k] = (float)sg;
    dbeta[k] = (float)sb;
}
__global__ void __launch_bounds__(256) k_fill_f32(float *__restrict__ p, int n, float v) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < n) p[i] = v;
}

static int transpose_run(int dtype, const void *in, int R, int Cc, float *out, hipStream_t s) {
    CPX_REQUIRE(R % 32 == 0 && Cc % 32 == 0);
    CPX_DT_DISPATCH(dtype, DT, hipLaunchKernelGGL(k_transpose_f32<DT>, dim3(Cc / 32, R / 32), dim3(256), 0, s, in, R, Cc, out));
    CPX_CHECK_LAUNCH();
    return CPX_OK;
}
int cpx_transpose_f32_run(int dtype, const void *in, int R, int Cc, float *out, hipStream_t s) { return transpose_run(dtype, in, R, Cc, out, s); }
static int add_run(const float *a, const float *b, size_t n, float *out, hipStream_t s) {
    hipLaunchKernelGGL(k_add_f32, grid1(n / 4), dim3(256), 0, s, a, b, n / 4, out);
    CPX_CHECK_LAUNCH();
    return CPX_OK;
}

// ---------------------------------------------------------------------------
// the backward of the last K blocks
// ---------------------------------------------------------------------------
// grads / params of one block (float32 elements): ln1 gamma, beta | qkv W [3072][1024], b | rel_h, rel_w [64][64] (the operand tables) |
// proj W [1024][1024], b | ln2 gamma, beta | fc1 W [4096][1024], b | fc2 W [1024][4096], b
#define BLK_N 14
extern "C" long long cpx_block_grad_layout(long long *off) {
    const long long n[BLK_N] = {1024, 1024, 3072ll * 1024, 3072, 4096, 4096, 1024ll * 1024, 1024, 1024, 1024, 4096ll * 1024, 4096, 1024ll * 4096, 1024};
    long long o = 0;
    for (int i = 0; i < BLK_N; ++i) { if (off) off[i] = o; o += n[i]; }
    return o;
}

// The crops are independent from the neck's dy0 down to the first trained block's input, so the backward runs them in slabs of
// BLK_SLAB crops through ALL blocks, and every parameter gradient is the sum over the slabs in slab order: the workspace does not grow
// with the batch.  Per slab of Ms rows (float32): dx, dxl, xn, xhat [Ms][1024]; three [Ms][4096] (pre, then dqkv | h, then dpre | dh);
// two transposed GEMM operands [4096][Ms]; a transposed weight and the widened fc1 operand [4096][1024]; the workspaces of
// cpx_attention_backward and cpx_layernorm_backward; three [1024] vectors.  8 and 32 crops alike: 241 MiB.
#define BLK_SLAB 2
// grad_dtype CPX_DT_BF16 (bf16 operands on the bf16 MFMA): no transposed float32 operands and no widened weights; instead dy, the hidden
// activations and the LayerNorm output rounded to bf16 ([Ms][4096], [Ms][4096], [Ms][1024]), a transposed 2-byte weight [4096][1024] and the
// partials of the column sums: 190 MiB.
struct BlocksBwdLayout { size_t dx, dxl, xn, xh, b1, b2, b3, t1, t2, wt, wop, attn, attn_bytes, ln, ln_bytes, vec, dyb, hb, xb, wt16, cs, cs_bytes, total; };
static BlocksBwdLayout blocks_bwd_layout(int grad_dtype) {
    BlocksBwdLayout L; CpxArena a; const size_t Ms = (size_t)BLK_SLAB * 1024;
    const bool g16 = grad_dtype == CPX_DT_BF16;
    L.dx = a.take(Ms * 1024 * 4); L.dxl = a.take(Ms * 1024 * 4); L.xn = a.take(Ms * 1024 * 4); L.xh = a.take(Ms * 1024 * 4);
    L.b1 = a.take(Ms * 4096 * 4); L.b2 = a.take(Ms * 4096 * 4); L.b3 = a.take(Ms * 4096 * 4);
    L.t1 = a.take(g16 ? 0 : Ms * 4096 * 4); L.t2 = a.take(g16 ? 0 : Ms * 4096 * 4);
    L.wt = a.take(g16 ? 0 : (size_t)4096 * 1024 * 4); L.wop = a.take(g16 ? 0 : (size_t)4096 * 1024 * 4);
    L.attn_bytes = cpx_attention_backward_workspace_bytes(BLK_SLAB); L.attn = a.take(L.attn_bytes);
    L.ln_bytes = cpx_layernorm_backward_bytes((int)Ms, 1024); L.ln = a.take(L.ln_bytes);
    L.vec = a.take(3 * 1024 * 4);
    L.dyb = a.take(g16 ? Ms * 4096 * 2 : 0); L.hb = a.take(g16 ? Ms * 4096 * 2 : 0); L.xb = a.take(g16 ? Ms * 1024 * 2 : 0);
    L.wt16 = a.take(g16 ? (size_t)4096 * 1024 * 2 : 0);
    L.cs_bytes = g16 ? cpx_colsum_workspace_bytes((int)Ms, 4096) : 0; L.cs = a.take(L.cs_bytes);
    L.total = a.o;
    return L;
}
// attn_grad_dtype CPX_DT_BF16 (the attention backward on bf16 operands, cpx_attention_backward_bf16) goes with bf16 gradient GEMMs only
static bool attn_grad_dtype_ok(int grad_dtype, int attn_grad_dtype) {
    return attn_grad_dtype == CPX_DT_F32 || (attn_grad_dtype == CPX_DT_BF16 && grad_dtype == CPX_DT_BF16);
}
// (the two attention backwards share one workspace layout, so attn_grad_dtype does not change the size)
static size_t blocks_bwd_bytes(int nS, int dtype, int grad_dtype, int attn_grad_dtype) {
    if (nS <= 0 || !dtype_ok(dtype) || !cpx_grad_dtype_ok(dtype, grad_dtype) || !attn_grad_dtype_ok(grad_dtype, attn_grad_dtype)) return 0;
    return blocks_bwd_layout(grad_dtype).total;
}
extern "C" size_t cpx_blocks_backward_workspace_bytes(int nS, int dtype) { return blocks_bwd_bytes(nS, dtype, CPX_DT_F32, CPX_DT_F32); }
extern "C" size_t cpx_blocks_backward_workspace_bytes_ex(int nS, int dtype, int grad_dtype) { return blocks_bwd_bytes(nS, dtype, grad_dtype, CPX_DT_F32); }
extern "C" size_t cpx_blocks_backward_workspace_bytes_mp(int nS, int dtype, int grad_dtype, int ad) { return blocks_bwd_bytes(nS, dtype, grad_dtype, ad); }
extern "C" int cpx_blocks_backward_slab_crops(void) { return BLK_SLAB; }

// The slab's crops (c0 and, where nc_slab is 2, c0 + 1) that a block ran on under its mask row kj (NULL: no mask): nc of them -- both
// (adjacent in the block's compact records, which keep crop order), one or none --, from row rb of those records (1024 times the block's
// kept crops before the slab), their gradient rows dx_off floats into the slab's dx (the second crop's half when only that one is kept).
struct SlabKept { int nc; size_t rb, dx_off; };
static SlabKept slab_kept(const unsigned char *kj, int c0, int nc_slab) {
    if (!kj) return {nc_slab, (size_t)c0 * 1024, 0};
    const int k0 = kj[c0] != 0, k1 = nc_slab > 1 && kj[c0 + 1] != 0;
    size_t rb = 0;
    for (int c = 0; c < c0; ++c) rb += kj[c] ? 1024 : 0;
    return {k0 + k1, rb, k0 ? (size_t)0 : (size_t)1024 * 1024};
}
// operands of the backward's products: rows of activations with their element type, and a Linear's weight [N][Kin] -- op, the forward's operand
// in the network dtype; master, its unfolded float32 record in params (NULL: none); folds: the forward may fold LayerNorm into it
struct BwdRows { const void *p; int dt; };
struct BwdWeight { const void *op; const float *master; bool folds; };

// The one body of the five exported backward entries; the contract is at cpx_blocks_backward_drop in include/classpose_hip.h.  w: the
// weights the forward ran with (the operand tables come from it: the rel slots of params are not read); fwd_workspace: what
// blocks_forward_run filled under the same keep.  What grad_dtype changes is in the four lambdas of the Linear layer, what attn_grad_dtype
// changes is the one attention-backward call, what keep changes is slab_kept.  The dx rows of a dropped crop pass down untouched, into dx_all
// and dx_in too (dx_in: record 0 of dx_all alone, copied where that record is); the gradients are added in slab order, with no atomics.
static int blocks_backward_run(const cpx_net_weights *w, const float *params, int nS, int first_block, const unsigned char *keep,
                               const void *fwd_workspace, size_t fwd_workspace_bytes, const float *dy0, int grad_dtype, int attn_grad_dtype,
                               float *grads, float *dx_all, float *dx_in, void *workspace, size_t workspace_bytes, void *stream) {
    CPX_REQUIRE(blocks_weights_ok(w, first_block) && params && fwd_workspace && dy0 && grads && workspace && w->neck0_w);
    CPX_REQUIRE(blocks_args_ok(nS, w->dtype, w->depth - first_block) && cpx_grad_dtype_ok(w->dtype, grad_dtype) && attn_grad_dtype_ok(grad_dtype, attn_grad_dtype));
    const int dt = w->dtype, K = w->depth - first_block;
    if (!keep_drops(keep, K, nS)) keep = nullptr;
    const bool g16 = grad_dtype == CPX_DT_BF16, a16 = attn_grad_dtype == CPX_DT_BF16;
    const BlocksFwdLayout F = blocks_fwd_layout(nS, dt, K);
    const BlocksBwdLayout L = blocks_bwd_layout(grad_dtype);
    CPX_REQUIRE(fwd_workspace_bytes >= F.total && workspace_bytes >= L.total);
    CPX_REQUIRE(((uintptr_t)workspace & 255) == 0 && ((uintptr_t)fwd_workspace & 255) == 0);
    CPX_REQUIRE((((uintptr_t)params | (uintptr_t)dy0 | (uintptr_t)grads | (uintptr_t)dx_all | (uintptr_t)dx_in) & 15) == 0);
    hipStream_t s = (hipStream_t)stream;
    const char *fws = (const char *)fwd_workspace;
    char *ws = (char *)workspace;
    float *dx_slab = (float *)(ws + L.dx), *dxl = (float *)(ws + L.dxl), *xn = (float *)(ws + L.xn), *xh = (float *)(ws + L.xh);
    float *b1 = (float *)(ws + L.b1), *b2 = (float *)(ws + L.b2), *b3 = (float *)(ws + L.b3), *t1 = (float *)(ws + L.t1), *t2 = (float *)(ws + L.t2);
    float *wt = (float *)(ws + L.wt), *wop = (float *)(ws + L.wop), *tg = (float *)(ws + L.vec), *tb = tg + 1024, *ones = tg + 2048;
    void *dyb = ws + L.dyb, *hb = ws + L.hb, *xb = ws + L.xb, *wt16 = ws + L.wt16;
    long long go[BLK_N];
    const long long gn = cpx_block_grad_layout(go);
    const size_t es = es_of(dt), rows_all = (size_t)nS * 1024;
    const bool half = dt != CPX_DT_F32, fuse = half && w->fuse_ln != 0;
    CPX_HIP(hipMemsetAsync(grads, 0, (size_t)gn * K * sizeof(float), s));
    hipLaunchKernelGGL(k_fill_f32, dim3(4), dim3(256), 0, s, ones, 1024, 1.0f);
    CPX_CHECK_LAUNCH();
    // LayerNorm of stored rows, as the forward's GEMM took it -> ln: xhat where the forward folds LayerNorm into the GEMM, else the
    // LayerNorm output, rounded through the network dtype as the unfused half forward stores it
    float *ln = fuse ? xh : xn;
    auto ln_fwd = [&](const void *x, const float *g, const float *b, int Ms) -> int {
        const dim3 grid(cpx_cdiv(Ms, 4)), block(256);
        if (fuse) { g = nullptr; b = nullptr; }
        if (half && !fuse) CPX_DT_DISPATCH(dt, DT, hipLaunchKernelGGL((k_ln_fwd1024<DT, true>), grid, block, 0, s, x, g, b, Ms, 1e-6f, ln));
        else CPX_DT_DISPATCH(dt, DT, hipLaunchKernelGGL((k_ln_fwd1024<DT, false>), grid, block, 0, s, x, g, b, Ms, 1e-6f, ln));
        CPX_CHECK_LAUNCH();
        return CPX_OK;
    };
    // ---- The Linear layer in either gradient precision: everything that depends on grad_dtype is in the next four lambdas. ----
    // Which weight a product multiplies by stays with the mode.  float32 mode: the data gradient takes the master record where the weights
    // are unfolded and the widened folded operand where they are folded (the derivative of what the forward multiplied by); the recomputed
    // product takes the forward's operand, widened for the half types.  bf16 mode: every product takes the forward's own operand, exact in
    // bf16 (for da a transposed 2-byte copy).
    // An activation operand from float32 rows.  float32 mode: the rows as they are; bf16 mode: rounded once into `stage`.  (Stored rows of
    // the network dtype are BwdRows{rows, dt} in both modes: the bf16 mode runs on a bf16 network alone.)
    auto operand = [&](const float *rows, size_t n, void *stage, BwdRows *a) -> int {
        *a = g16 ? BwdRows{stage, CPX_DT_BF16} : BwdRows{rows, CPX_DT_F32};
        return g16 ? cpx_round_weights(rows, stage, (long long)n, CPX_DT_BF16, 0, stream) : CPX_OK;
    };
    // float32 mode: the forward's operand [N][Kin] as float32 -- itself for a float32 network, else widened exactly into wop, once per
    // block body (the walk clears in_wop at its top): fc1's copy serves the recomputed product and, folded, the data gradient
    const void *in_wop = nullptr;
    auto operand_f32 = [&](const void *Wop, int N, int Kin, const float **W32) -> int {
        *W32 = half ? wop : (const float *)Wop;
        if (!half || in_wop == Wop) return CPX_OK;
        const size_t n4 = (size_t)N * Kin / 4;
        CPX_DT_DISPATCH(dt, DT, hipLaunchKernelGGL(k_widen_f32<DT>, grid1(n4), dim3(256), 0, s, Wop, n4, wop));
        CPX_CHECK_LAUNCH();
        in_wop = Wop;
        return CPX_OK;
    };
    // the recomputed forward product pre = a Wop^T + bias, pre [Ms][N] float32
    auto linear_fwd = [&](BwdRows a, const void *Wop, const float *bias, int Ms, int N, int Kin, float *pre) -> int {
        if (g16) return cpx_gemm_half(CPX_DT_BF16, a.p, Wop, Ms, N, Kin, CPX_EPI_F32, bias, nullptr, pre, N, nullptr, nullptr, nullptr, stream);
        const float *W32;
        CPX_RUN(operand_f32(Wop, N, Kin, &W32));
        return cpx_gemm_f32((const float *)a.p, W32, Ms, N, Kin, CPX_EPI_F32, bias, nullptr, pre, N, stream);
    };
    // the backward of a Linear y = a W^T + b with a [Ms][Kin], dy [Ms][N] float32: dW += dy^T a and db += the column sums of the unrounded
    // dy (dW NULL: neither), da = dy W
    auto linear_bwd = [&](const float *dy, BwdRows a, BwdWeight W, int Ms, int N, int Kin, float *dW, float *db, float *da) -> int {
        if (g16) {
            BwdRows d;
            CPX_RUN(operand(dy, (size_t)Ms * N, dyb, &d));
            if (dW) {
                CPX_RUN(cpx_gemm_tn_bf16(d.p, a.p, Ms, N, Kin, 1, dW, Kin, stream));
                CPX_RUN(cpx_colsum_add(dy, Ms, N, db, ws + L.cs, L.cs_bytes, stream));
            }
            CPX_RUN(wt16_run(W.op, N, Kin, Kin, wt16, s));
            return cpx_gemm_half(CPX_DT_BF16, d.p, wt16, Ms, Kin, N, CPX_EPI_F32, nullptr, nullptr, da, Kin, nullptr, nullptr, nullptr, stream);
        }
        const float *W32 = W.master;
        if (W.folds && fuse) CPX_RUN(operand_f32(W.op, N, Kin, &W32));
        if (dW) {
            CPX_RUN(transpose_run(CPX_DT_F32, dy, Ms, N, t1, s));
            CPX_RUN(transpose_run(a.dt, a.p, Ms, Kin, t2, s));
            CPX_RUN(cpx_gemm_f32(t1, t2, N, Kin, Ms, CPX_EPI_RESID_BF16, nullptr, dW, dW, Kin, stream));
            hipLaunchKernelGGL(k_colsum_add, grid1(N), dim3(256), 0, s, dy, Ms, N, db);
            CPX_CHECK_LAUNCH();
        }
        if (W32) CPX_RUN(transpose_run(CPX_DT_F32, W32, N, Kin, wt, s));
        else CPX_RUN(cpx_wt_run(dt, W.op, N, Kin, Kin, wt, s));                // (no master: the operand, widened and transposed in one pass)
        return cpx_gemm_f32(dy, wt, Ms, Kin, N, CPX_EPI_F32, nullptr, nullptr, da, Kin, stream);
    };
    // folded: dout is the gradient of xhat (gamma = 1 here; dgamma and dbeta come from k_unfold_grads after the last slab)
    auto ln_bwd = [&](const void *x, const float *g, const float *dout, int Ms, float *dx, float *dgamma, float *dbeta) -> int {
        CPX_RUN(cpx_layernorm_backward(dt, x, fuse ? ones : g, dout, Ms, 1024, 1e-6f, dxl, tg, tb, ws + L.ln, L.ln_bytes, stream));
        if (!fuse) {
            CPX_RUN(add_run(dgamma, tg, 1024, dgamma, s));
            CPX_RUN(add_run(dbeta, tb, 1024, dbeta, s));
        }
        return add_run(dx, dxl, (size_t)Ms * 1024, dx, s);           // the residual: dx is now the gradient of the LayerNorm's input rows
    };
    for (int c0 = 0; c0 < nS; c0 += BLK_SLAB) {
        const int nc_slab = std::min(BLK_SLAB, nS - c0), Ms_slab = nc_slab * 1024;
        const size_t r0 = (size_t)c0 * 1024;
        // record j of dx_all (and dx_in) takes the slab's rows as block j leaves them, dropped crops included
        auto pass_down = [&](int j) -> int {
            if (dx_all) CPX_HIP(hipMemcpyAsync(dx_all + ((size_t)j * rows_all + r0) * 1024, dx_slab, (size_t)Ms_slab * 4096, hipMemcpyDeviceToDevice, s));
            if (dx_in && j == 0) CPX_HIP(hipMemcpyAsync(dx_in + r0 * 1024, dx_slab, (size_t)Ms_slab * 4096, hipMemcpyDeviceToDevice, s));
            return CPX_OK;
        };
        // the gradient of the last block's output: dy0 W0 (the rounded operand [256][1024], widened and transposed)
        CPX_RUN(linear_bwd(dy0 + r0 * 256, BwdRows{}, BwdWeight{w->neck0_w, nullptr, false}, Ms_slab, 256, 1024, nullptr, nullptr, dx_slab));
        CPX_RUN(pass_down(K));                                     // record K of dx_all: the gradient of x_out
        for (int j = K - 1; j >= 0; --j) {
            const cpx_block_weights &b = w->blocks[first_block + j];
            const float *P = params + (size_t)gn * j;
            float *Gd = grads + (size_t)gn * j;
            const char *base = fws + F.stride * (size_t)j;
            const SlabKept k = slab_kept(keep ? keep + (size_t)j * nS : nullptr, c0, nc_slab);
            if (!k.nc) {
                CPX_RUN(pass_down(j));
                continue;
            }
            const int nc = k.nc, Ms = nc * 1024;
            in_wop = nullptr;
            float *dx = dx_slab + k.dx_off;
            const void *xin = base + F.o_x + k.rb * 1024 * es, *qkv = base + F.o_qkv + k.rb * 3072 * es, *ao = base + F.o_ao + k.rb * 1024 * es,
                       *xmid = base + F.o_mid + k.rb * 1024 * es;
            BwdRows a, h;
            // ---- the MLP: x_out = x_mid + gelu(LN2(x_mid) W1^T + b1) W2^T + b2 ----
            CPX_RUN(ln_fwd(xmid, P + go[8], P + go[9], Ms));
            CPX_RUN(operand(ln, (size_t)Ms * 1024, xb, &a));
            CPX_RUN(linear_fwd(a, b.fc1_w, b.fc1_b, Ms, 4096, 1024, b1));                                                         // pre
            CPX_DT_DISPATCH(dt, DT, hipLaunchKernelGGL(k_gelu_fwd_round<DT>, grid1((size_t)Ms * 4096), dim3(256), 0, s, b1, (size_t)Ms * 4096, b2));   // h
            CPX_CHECK_LAUNCH();
            CPX_RUN(operand(b2, (size_t)Ms * 4096, hb, &h));                                                                      // (exact: h is rounded)
            CPX_RUN(linear_bwd(dx, h, BwdWeight{b.fc2_w, P + go[12], false}, Ms, 1024, 4096, Gd + go[12], Gd + go[13], b3));             // fc2 -> dh
            CPX_RUN(cpx_gelu_backward(b1, b3, (size_t)Ms * 4096, b2, stream));                                                    // dpre
            CPX_RUN(linear_bwd(b2, a, BwdWeight{b.fc1_w, P + go[10], true}, Ms, 4096, 1024, Gd + go[10], Gd + go[11], b3));    // fc1 -> d LN2 output (folded: d xhat)
            CPX_RUN(ln_bwd(xmid, P + go[8], b3, Ms, dx, Gd + go[8], Gd + go[9]));                                                 // dx = d x_mid
            // ---- attention: x_mid = x_in + attention(LN1(x_in) Wqkv^T + bqkv) Wp^T + bp ----
            CPX_RUN(linear_bwd(dx, BwdRows{ao, dt}, BwdWeight{b.proj_w, P + go[6], false}, Ms, 1024, 1024, Gd + go[6], Gd + go[7], b3));  // proj -> dO
            if (a16) CPX_RUN(cpx_attention_backward_bf16_run(qkv, b.rel_h, b.rel_w, b3, nc, b1, Gd + go[4], Gd + go[5], 1, ws + L.attn, L.attn_bytes, stream));
            else CPX_RUN(cpx_attention_backward_run(dt, qkv, b.rel_h, b.rel_w, nullptr, b3, nc, b1, Gd + go[4], Gd + go[5], 1, ws + L.attn, L.attn_bytes, stream));
            CPX_RUN(ln_fwd(xin, P + go[0], P + go[1], Ms));
            CPX_RUN(operand(ln, (size_t)Ms * 1024, xb, &a));
            CPX_RUN(linear_bwd(b1, a, BwdWeight{b.qkv_w, P + go[2], true}, Ms, 3072, 1024, Gd + go[2], Gd + go[3], b3));    // qkv -> d LN1 output (folded: d xhat)
            CPX_RUN(ln_bwd(xin, P + go[0], b3, Ms, dx, Gd + go[0], Gd + go[1]));                                                  // dx = d x_in
            CPX_RUN(pass_down(j));
        }
    }
    if (fuse)                                                          // the W slots hold dWf, the b slots dbf, summed over the slabs
        for (int j = 0; j < K; ++j) {
            const float *P = params + (size_t)gn * j;
            float *Gd = grads + (size_t)gn * j;
            hipLaunchKernelGGL(k_unfold_grads, dim3(4), dim3(256), 0, s, Gd + go[2], Gd + go[3], P + go[2], P + go[0], P + go[1], 3072, Gd + go[0], Gd + go[1]);
            CPX_CHECK_LAUNCH();
            hipLaunchKernelGGL(k_unfold_grads, dim3(4), dim3(256), 0, s, Gd + go[10], Gd + go[11], P + go[10], P + go[8], P + go[9], 4096, Gd + go[8], Gd + go[9]);
            CPX_CHECK_LAUNCH();
        }
    return CPX_OK;
}
// the exported entries: cpx_blocks_backward_drop is blocks_backward_run, each older one that with arguments fixed
extern "C" int cpx_blocks_backward_in(const cpx_net_weights *w, const float *params, int nS, int first_block, const void *fwd_workspace,
                                      size_t fwd_workspace_bytes, const float *dy0, int grad_dtype, int attn_grad_dtype, float *grads,
                                      float *dx_all, float *dx_in, void *workspace, size_t workspace_bytes, void *stream) {
    return blocks_backward_run(w, params, nS, first_block, nullptr, fwd_workspace, fwd_workspace_bytes, dy0, grad_dtype, attn_grad_dtype, grads,
                               dx_all, dx_in, workspace, workspace_bytes, stream);
}
extern "C" int cpx_blocks_backward_drop(const cpx_net_weights *w, const float *params, int nS, int first_block, const unsigned char *keep,
                                        const void *fwd_workspace, size_t fwd_workspace_bytes, const float *dy0, int grad_dtype,
                                        int attn_grad_dtype, float *grads, float *dx_all, float *dx_in, void *workspace, size_t workspace_bytes,
                                        void *stream) {
    return blocks_backward_run(w, params, nS, first_block, keep, fwd_workspace, fwd_workspace_bytes, dy0, grad_dtype, attn_grad_dtype, grads,
                               dx_all, dx_in, workspace, workspace_bytes, stream);
}
extern "C" int cpx_blocks_backward_mp(const cpx_net_weights *w, const float *params, int nS, int first_block, const void *fwd_workspace,
                                      size_t fwd_workspace_bytes, const float *dy0, int grad_dtype, int attn_grad_dtype, float *grads,
                                      float *dx_all, void *workspace, size_t workspace_bytes, void *stream) {
    return blocks_backward_run(w, params, nS, first_block, nullptr, fwd_workspace, fwd_workspace_bytes, dy0, grad_dtype, attn_grad_dtype, grads,
                               dx_all, nullptr, workspace, workspace_bytes, stream);
}
extern "C" int cpx_blocks_backward_ex(const cpx_net_weights *w, const float *params, int nS, int first_block, const void *fwd_workspace,
                                      size_t fwd_workspace_bytes, const float *dy0, int grad_dtype, float *grads, float *dx_all,
                                      void *workspace, size_t workspace_bytes, void *stream) {
    return blocks_backward_run(w, params, nS, first_block, nullptr, fwd_workspace, fwd_workspace_bytes, dy0, grad_dtype, CPX_DT_F32, grads,
                               dx_all, nullptr, workspace, workspace_bytes, stream);
}
extern "C" int cpx_blocks_backward(const cpx_net_weights *w, const float *params, int nS, int first_block, const void *fwd_workspace,
                                   size_t fwd_workspace_bytes, const float *dy0, float *grads, float *dx_all, void *workspace,
                                   size_t workspace_bytes, void *stream) {
    return blocks_backward_run(w, params, nS, first_block, nullptr, fwd_workspace, fwd_workspace_bytes, dy0, CPX_DT_F32, CPX_DT_F32, grads,
                               dx_all, nullptr, workspace, workspace_bytes, stream);
}
