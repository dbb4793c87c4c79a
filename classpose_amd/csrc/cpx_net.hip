// ClassTransformer forward on gfx950 (vit_sam.py:148-197 + flash_forward :15-65):
// LayerNorm, global attention with the decomposed relative-position bias fused
// into the flash loop, the neck (its 3x3 conv is an implicit GEMM), and the launch sequence that
// strings them together with the MFMA GEMM of cpx_gemm.hip.
// One driver for all three dtypes (cpx_net_forward; the float32 kernels are in cpx_net_f32.hip) on one workspace layout (cpx_net_ws).
// Shared with the training forwards: one transformer block as one launch sequence (cpx_net_block; cpx_train_blocks.hip runs it on
// tensors it keeps) and the network tail -- neck, head GEMM, optional UNet head -- as another (cpx_net_tail; cpx_train_neck.hip).
// The UNet head's layout and run read the op geometry the backward reads too (op_dims, cpx_internal.h).
//
// Attention design (T = 32x32 tokens, 16 heads x 64):
//   * one wave owns one IMAGE ROW of queries (32 tokens, same qh) and walks the
//     keys one image row (32 keys, same kh) at a time, so the bias
//        rel_h[q, kh] + rel_w[q, kw]
//     is   Gh[q][qh-kh+31]  (one scalar per lane per key tile)
//        + Gw[q][qw-kw+31]  (16 per-lane constants for the whole loop)
//     where G = Q . table^T is two small MFMA products per wave; the dense
//     [T x T] bias of the reference is never materialised;
//   * S^T = K . Q^T is computed with the accumulator pre-loaded with the bias
//     ("row constants as the initial accumulator"), softmax is per lane (the
//     query is the MFMA column = the lane), and P^T feeds the P.V MFMA straight
//     from the accumulator registers: the key rows of the K operand are loaded
//     in the permuted order pi(r) = swap bits 2,3 so that the accumulator's
//     register order is the natural key order of the V^T operand.
#include "cpx_internal.h"
#include <algorithm>

typedef __attribute__((ext_vector_type(8))) __bf16 bf16x8;
typedef __attribute__((ext_vector_type(8))) _Float16 f16x8;

template <bool F16>
__device__ __forceinline__ f32x16 mfma32(const uint4 &a, const uint4 &b, f32x16 c) {
    if constexpr (F16)
        return __builtin_amdgcn_mfma_f32_32x32x16_f16(*reinterpret_cast<const f16x8 *>(&a),
                                                      *reinterpret_cast<const f16x8 *>(&b), c, 0, 0, 0);
    else
        return __builtin_amdgcn_mfma_f32_32x32x16_bf16(*reinterpret_cast<const bf16x8 *>(&a),
                                                       *reinterpret_cast<const bf16x8 *>(&b), c, 0, 0, 0);
}
template <bool F16>
__device__ __forceinline__ unsigned short h_from_f32(float f) {
    if constexpr (F16) { _Float16 h = (_Float16)f; return *reinterpret_cast<unsigned short *>(&h); }
    else return f32_to_bf16(f);
}
template <bool F16>
__device__ __forceinline__ float f32_from_h(unsigned short u) {
    if constexpr (F16) return (float)*reinterpret_cast<_Float16 *>(&u);
    else return bf16_to_f32(u);
}

// two floats -> one dword of two halves with a single v_cvt_pk_* (vector convert)
typedef __attribute__((ext_vector_type(2))) float f32x2_t;
typedef __attribute__((ext_vector_type(2))) __bf16 bf16x2_t;
typedef __attribute__((ext_vector_type(2))) _Float16 f16x2_t;
template <bool F16>
__device__ __forceinline__ unsigned pack2(float lo, float hi) {
    f32x2_t v = {lo, hi};
    if constexpr (F16) return __builtin_bit_cast(unsigned, __builtin_convertvector(v, f16x2_t));
    else return __builtin_bit_cast(unsigned, __builtin_convertvector(v, bf16x2_t));
}

// ---------------------------------------------------------------------------
// LayerNorm over the last dim (C = 1024 or 256), one wave per row
// ---------------------------------------------------------------------------
template <int C, bool F16>
__global__ void __launch_bounds__(256) k_layernorm(const unsigned short *__restrict__ x,
                                                   const float *__restrict__ w,
                                                   const float *__restrict__ b, int rows, float eps,
                                                   unsigned short *__restrict__ out) {
    constexpr int PER = C / 64;          // elements per lane: 16 or 4
    const int lane = threadIdx.x & 63;
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= rows) return;
    const unsigned short *xr = x + (size_t)row * C + lane * PER;
    float v[PER];
    if constexpr (PER == 16) {
        uint4 a = *reinterpret_cast<const uint4 *>(xr), c = *reinterpret_cast<const uint4 *>(xr + 8);
        unsigned u[8] = {a.x, a.y, a.z, a.w, c.x, c.y, c.z, c.w};
#pragma unroll
        for (int i = 0; i < 8; ++i) { v[2 * i] = f32_from_h<F16>(u[i] & 0xFFFF); v[2 * i + 1] = f32_from_h<F16>(u[i] >> 16); }
    } else {
        uint2 a = *reinterpret_cast<const uint2 *>(xr);
        v[0] = f32_from_h<F16>(a.x & 0xFFFF); v[1] = f32_from_h<F16>(a.x >> 16);
        v[2] = f32_from_h<F16>(a.y & 0xFFFF); v[3] = f32_from_h<F16>(a.y >> 16);
    }
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < PER; ++i) s += v[i];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
    const float mean = s * (1.0f / C);
    float q = 0.f;
#pragma unroll
    for (int i = 0; i < PER; ++i) { float d = v[i] - mean; q += d * d; }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) q += __shfl_xor(q, o);
    const float rstd = rsqrtf(q * (1.0f / C) + eps);
    unsigned short o16[PER];
#pragma unroll
    for (int i = 0; i < PER; ++i) {
        float y = (v[i] - mean) * rstd * w[lane * PER + i] + b[lane * PER + i];
        o16[i] = h_from_f32<F16>(y);
    }
    unsigned short *orow = out + (size_t)row * C + lane * PER;
    if constexpr (PER == 16) {
        uint4 a, c;
        a.x = o16[0] | (o16[1] << 16); a.y = o16[2] | (o16[3] << 16); a.z = o16[4] | (o16[5] << 16); a.w = o16[6] | (o16[7] << 16);
        c.x = o16[8] | (o16[9] << 16); c.y = o16[10] | (o16[11] << 16); c.z = o16[12] | (o16[13] << 16); c.w = o16[14] | (o16[15] << 16);
        *reinterpret_cast<uint4 *>(orow) = a;
        *reinterpret_cast<uint4 *>(orow + 8) = c;
    } else {
        uint2 a;
        a.x = o16[0] | (o16[1] << 16); a.y = o16[2] | (o16[3] << 16);
        *reinterpret_cast<uint2 *>(orow) = a;
    }
}

int cpx_layernorm_half(int dtype, const void *x, const float *w, const float *b, int rows, int C,
                       float eps, void *out, void *stream) {
    CPX_REQUIRE(x && w && b && out && rows > 0 && (C == 1024 || C == 256));
    CPX_REQUIRE(dtype == CPX_DT_BF16 || dtype == CPX_DT_F16);
    hipStream_t s = (hipStream_t)stream;
    dim3 grid(cpx_cdiv(rows, 4)), block(256);
    const bool f16 = dtype == CPX_DT_F16;
    if (C == 1024) {
        if (f16) hipLaunchKernelGGL((k_layernorm<1024, true>), grid, block, 0, s, (const unsigned short *)x, w, b, rows, eps, (unsigned short *)out);
        else hipLaunchKernelGGL((k_layernorm<1024, false>), grid, block, 0, s, (const unsigned short *)x, w, b, rows, eps, (unsigned short *)out);
    } else {
        if (f16) hipLaunchKernelGGL((k_layernorm<256, true>), grid, block, 0, s, (const unsigned short *)x, w, b, rows, eps, (unsigned short *)out);
        else hipLaunchKernelGGL((k_layernorm<256, false>), grid, block, 0, s, (const unsigned short *)x, w, b, rows, eps, (unsigned short *)out);
    }
    CPX_CHECK_LAUNCH();
    return CPX_OK;
}
extern "C" int cpx_layernorm(int dtype, const void *x, const float *w, const float *b, int rows, int C,
                             float eps, void *out, void *stream) {
    if (dtype == CPX_DT_F32) return cpx_layernorm_f32((const float *)x, w, b, rows, C, eps, (float *)out, stream);
    return cpx_layernorm_half(dtype, x, w, b, rows, C, eps, out, stream);
}
extern "C" int cpx_layernorm_bf16(const void *x, const float *w, const float *b, int rows, int C,
                                  float eps, void *out, void *stream) {
    return cpx_layernorm_half(CPX_DT_BF16, x, w, b, rows, C, eps, out, stream);
}

// ---------------------------------------------------------------------------
// V transpose: qkv[., 2048 + h*64 + d] -> vT[s][h][d][t]   (LDS tile transpose)
// ---------------------------------------------------------------------------
__global__ void __launch_bounds__(256) k_v_transpose(const unsigned short *__restrict__ qkv,
                                                     unsigned short *__restrict__ vT) {
    __shared__ unsigned short tile[64][66];
    const int t0 = blockIdx.x * 64, h = blockIdx.y, s = blockIdx.z;
    const int tid = threadIdx.x;
    {   // 64 tokens x 64 d: thread -> (token = tid>>2, 16 d)
        int tok = tid >> 2, c = (tid & 3) * 16;
        const unsigned short *src = qkv + ((size_t)s * 1024 + t0 + tok) * 3072 + 2048 + h * 64 + c;
        uint4 a = *reinterpret_cast<const uint4 *>(src), b = *reinterpret_cast<const uint4 *>(src + 8);
        unsigned u[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
#pragma unroll
        for (int i = 0; i < 8; ++i) { tile[tok][c + 2 * i] = u[i] & 0xFFFF; tile[tok][c + 2 * i + 1] = u[i] >> 16; }
    }
    __syncthreads();
    {   // thread -> (d = tid>>2, 16 tokens)
        int d = tid >> 2, c = (tid & 3) * 16;
        unsigned u[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) u[i] = tile[c + 2 * i][d] | ((unsigned)tile[c + 2 * i + 1][d] << 16);
        unsigned short *dst = vT + (((size_t)s * 16 + h) * 64 + d) * 1024 + t0 + c;
        *reinterpret_cast<uint4 *>(dst) = make_uint4(u[0], u[1], u[2], u[3]);
        *reinterpret_cast<uint4 *>(dst + 8) = make_uint4(u[4], u[5], u[6], u[7]);
    }
}

// ---------------------------------------------------------------------------
// flash attention with decomposed rel-pos bias
// ---------------------------------------------------------------------------
#define ATT_THREADS 256
__device__ __forceinline__ int pi_perm(int r) { return (r & ~12) | ((r & 4) << 1) | ((r & 8) >> 1); }

// ---------------------------------------------------------------------------
// flash attention, 4 waves per workgroup, LDS-DMA ring + software-pipelined S (debug build: variant 7, the bitwise
// reference of tests/test_gpu_attn2w.py; the production kernel of rounds 2-5, replaced by k_attention2w of cpx_attn2w.hip)
// ---------------------------------------------------------------------------
// Same decomposition as the round-1 kernel k_attention (register ring, retired: git show f07d44d:classpose_amd/csrc/cpx_net.hip):
// one wave = one image row of 32 queries, key tiles = image rows, rel-pos bias as MFMA C operand + one scalar per lane, P^T fed
// to the P.V MFMA from the accumulator registers.  What differs:
//   * K / V^T tiles reach LDS by LDS-DMA (global_load_lds_dwordx4, swizzle on the SOURCE address, lane-linear
//     image) into a 4-slot ring, requested three tiles ahead: no staging registers (the register ring of
//     k_attention held 32 VGPRs), no ds_write, one raw s_barrier per tile behind a counted vmcnt;
//   * the freed registers hold a second score tile: S = K_{t+1} Q^T + Gw is issued BEFORE the softmax of tile t,
//     so the dependent QK^T chain (~330 cycles for a lone wave, profiles/r02_attn4_stamps.txt) runs under the
//     softmax's VALU work instead of in front of it;
//   * the per-wave G = Q table^T scratch is kept in fp16 (16.5 KB instead of 33 KB per workgroup), which pays
//     for the deeper ring at three workgroups per CU; row sums are f32 VALU adds (no ones-row MFMA, no Lacc).
// Every LDS read inside the loop is inline asm: with a DMA in flight hipcc drains it (vmcnt(0)) in front of
// ordinary LDS reads of the same array and in front of __syncthreads().
#define A4_SLOT 8192
#define A4_G_LD 66
#define A4_LDS_BYTES (4 * A4_SLOT + 4 * 32 * A4_G_LD * 2)
template <int OFF>
__device__ __forceinline__ uint4 a4_read128(unsigned addr) {
    uint4 v;
    asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(v) : "v"(addr), "n"(OFF));
    return v;
}
template <bool F16>
__global__ void __launch_bounds__(ATT_THREADS, 3) k_attention4p(const unsigned short *__restrict__ qkv,
                                                                const unsigned short *__restrict__ vT,
                                                                const unsigned short *__restrict__ relh,
                                                                const unsigned short *__restrict__ relw,
                                                                unsigned short *__restrict__ out, int xcd_order) {
    extern __shared__ __attribute__((aligned(16))) char a4_smem[];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int r = lane & 31, h2 = lane >> 5;
    const int lin = (blockIdx.z * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x;
    int rg = blockIdx.x, head = blockIdx.y, s = blockIdx.z;
    if (xcd_order) {
        const int j = lin >> 3, pair = (j >> 3) * 8 + (lin & 7);
        rg = j & 7; head = pair & 15; s = pair >> 4;
    }
    const int qh = rg * 4 + wave;
    const size_t tok0 = (size_t)s * 1024;
    // ---- ring requests: thread -> 16 bytes of K (key tid>>3, position tid&7) and of V^T (d tid>>2, position tid&3)
    const int kkey = tid >> 3, vd = tid >> 2;
    // K image: 16-byte chunk c of key row k sits at position c ^ ((k >> 1) & 7): the 16 rows one ds_read_b128 lane group
    // touches ({0-3, 12-15, 20-27} or {4-11, 16-19, 28-31} after the key permutation) then fall on 16 distinct
    // 16-byte slots of the 256-byte bank row (the (k & 7) swizzle of k_attention was 2-way conflicted: rows k and k + 8)
    const unsigned short *ksrc = qkv + (tok0 + kkey) * 3072 + 1024 + head * 64 + (((tid & 7) ^ ((kkey >> 1) & 7)) * 8);
    const unsigned short *vsrc = vT + (((size_t)s * 16 + head) * 64 + vd) * 1024 + (((tid & 3) ^ ((vd >> 2) & 3)) * 8);
    char *dma_dst = a4_smem + wave * 1024;
    auto issue = [&](int kh) {
        char *d = dma_dst + (kh & 3) * A4_SLOT;
        __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void *)(ksrc + (size_t)kh * 32 * 3072),
                                         (__attribute__((address_space(3))) void *)d, 16, 0, 0);
        __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void *)(vsrc + kh * 32),
                                         (__attribute__((address_space(3))) void *)(d + 4096), 16, 0, 0);
    };
    issue(0); issue(1); issue(2);

    const unsigned short *qrow = qkv + (tok0 + qh * 32 + r) * 3072 + head * 64;
    uint4 qf[4];
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) qf[ks] = *reinterpret_cast<const uint4 *>(qrow + 16 * ks + 8 * h2);
    // G = Q . table^T -> this wave's fp16 scratch [q][j] (values are bias / scale, |G| < ~60: fp16 keeps 2^-11 relative)
    _Float16 *G = reinterpret_cast<_Float16 *>(a4_smem + 4 * A4_SLOT) + wave * 32 * A4_G_LD;
    auto compute_G = [&](const unsigned short *table) {
#pragma unroll
        for (int jb = 0; jb < 2; ++jb) {
            f32x16 acc;
#pragma unroll
            for (int i = 0; i < 16; ++i) acc[i] = 0.f;
#pragma unroll
            for (int ks = 0; ks < 4; ++ks) {
                uint4 tf = *reinterpret_cast<const uint4 *>(table + (jb * 32 + r) * 64 + 16 * ks + 8 * h2);
                acc = mfma32<F16>(tf, qf[ks], acc);
            }
#pragma unroll
            for (int i = 0; i < 16; ++i) G[r * A4_G_LD + jb * 32 + (i & 3) + 8 * (i >> 2) + 4 * h2] = (_Float16)acc[i];
        }
    };
    compute_G(relw);
    f32x16 GW;
#pragma unroll
    for (int i = 0; i < 16; ++i) GW[i] = (float)G[r * A4_G_LD + (r - pi_perm((i & 3) + 8 * (i >> 2) + 4 * h2) + 31)];
    compute_G(relh);
    asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");      // tiles 0..2 and this wave's G rows have landed
    __builtin_amdgcn_s_barrier();

    // per-lane LDS byte addresses of the fragments (slot offset added as an immediate)
    const unsigned lds0 = (unsigned)(size_t)(__attribute__((address_space(3))) char *)a4_smem;
    const int krow = pi_perm(r);
    unsigned ka[4], va[4];
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) ka[ks] = lds0 + (unsigned)(krow * 128 + (((2 * ks + h2) ^ ((krow >> 1) & 7)) * 16));
#pragma unroll
    for (int db = 0; db < 2; ++db)
#pragma unroll
        for (int st = 0; st < 2; ++st) {
            const int d = db * 32 + r;
            va[db * 2 + st] = lds0 + 4096u + (unsigned)(d * 64 + (((2 * st + h2) ^ ((d >> 2) & 3)) * 16));
        }
    const unsigned gaddr = lds0 + 4u * A4_SLOT + (unsigned)((wave * 32 * A4_G_LD + r * A4_G_LD + qh + 31) * 2);   // - 2 kh per tile

    auto qk = [&](auto slot_tag) {
        constexpr int SL = decltype(slot_tag)::value;
        const uint4 k0 = a4_read128<SL * A4_SLOT>(ka[0]), k1 = a4_read128<SL * A4_SLOT>(ka[1]);
        const uint4 k2 = a4_read128<SL * A4_SLOT>(ka[2]), k3 = a4_read128<SL * A4_SLOT>(ka[3]);
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_sched_barrier(0);
        f32x16 S = mfma32<F16>(k0, qf[0], GW);
        S = mfma32<F16>(k1, qf[1], S);
        S = mfma32<F16>(k2, qf[2], S);
        S = mfma32<F16>(k3, qf[3], S);
        return S;
    };
    using std::integral_constant;
    f32x16 S = qk(integral_constant<int, 0>{});
    f32x16 O0, O1;
#pragma unroll
    for (int i = 0; i < 16; ++i) { O0[i] = 0.f; O1[i] = 0.f; }
    float m_run = -1e30f, l_run = 0.f;
    const float cexp = 0.125f * 1.44269504088896340736f;
    constexpr float HEADROOM = F16 ? 3.0f : 6.0f;

    // TAIL (compile time): 0 = any key tile up to 28 (every end-of-sequence condition below holds), 1 / 2 / 3 = tiles 29 / 30 / 31 -- the last four
    // tiles are peeled so that the steady-state body carries no scalar branch for them (round 4)
    auto tile = [&](const int kh, auto slot_tag, auto next_tag, auto tail_tag) {
        constexpr int SL = decltype(slot_tag)::value, SN = decltype(next_tag)::value, TAIL = decltype(tail_tag)::value;
        // tile kh + 1 (this thread's part) has landed; after the barrier every part has, and every wave is done with
        // slot (kh - 1) & 3, which the next request overwrites
        if constexpr (TAIL < 2) asm volatile("s_waitcnt vmcnt(2)" ::: "memory");
        else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();
        if constexpr (TAIL == 0) issue(kh + 3);
        unsigned gh_bits;
        asm volatile("ds_read_u16 %0, %1" : "=v"(gh_bits) : "v"(gaddr - 2u * (unsigned)kh));
        f32x16 Sn = S;
        if constexpr (TAIL < 3) Sn = qk(integral_constant<int, SN>{});          // waits lgkmcnt(0): gh is there too
        else {
            // (gh_bits is an inline-asm LDS read: the wait must carry it as an operand, or the compiler is free to schedule its consumer in
            // front of the wait -- it did, in the peeled last tile, and every output was wrong by a few per cent)
            asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(gh_bits)::"memory");
            __builtin_amdgcn_sched_barrier(0);
        }
        const float gh = (float)__builtin_bit_cast(_Float16, (unsigned short)gh_bits);
        float p[16];
        unsigned pk[8];
        {
            const float off = (gh - m_run) * cexp;
#pragma unroll
            for (int i = 0; i < 16; ++i) p[i] = __builtin_amdgcn_exp2f(__builtin_fmaf(S[i], cexp, off));
#pragma unroll
            for (int j = 0; j < 8; ++j) pk[j] = pack2<F16>(p[2 * j], p[2 * j + 1]);
        }
        const bool resc = __builtin_expect(__any(((pk[0] | pk[1] | pk[2]) | (pk[3] | pk[4] | pk[5]) | (pk[6] | pk[7])) & 0x40004000u), 0);
        if (resc) {
            float mx = __builtin_fmaxf(__builtin_fmaxf(S[0], S[1]), S[2]);
#pragma unroll
            for (int i = 3; i < 15; i += 2) mx = __builtin_fmaxf(__builtin_fmaxf(mx, S[i]), S[i + 1]);
            mx = __builtin_fmaxf(mx, S[15]);
            mx = __builtin_fmaxf(mx, __shfl_xor(mx, 32)) + gh + HEADROOM / cexp;
            const float m_new = __builtin_fmaxf(m_run, mx);
            const float alpha = __builtin_amdgcn_exp2f((m_run - m_new) * cexp);
            m_run = m_new;
            l_run *= alpha;
#pragma unroll
            for (int i = 0; i < 16; ++i) { O0[i] *= alpha; O1[i] *= alpha; }
            const float off = (gh - m_run) * cexp;
#pragma unroll
            for (int i = 0; i < 16; ++i) p[i] = __builtin_amdgcn_exp2f(__builtin_fmaf(S[i], cexp, off));
#pragma unroll
            for (int j = 0; j < 8; ++j) pk[j] = pack2<F16>(p[2 * j], p[2 * j + 1]);
        }
        const float a0 = (p[0] + p[1]) + (p[2] + p[3]), a1 = (p[4] + p[5]) + (p[6] + p[7]);
        const float a2 = (p[8] + p[9]) + (p[10] + p[11]), a3 = (p[12] + p[13]) + (p[14] + p[15]);
        l_run += (a0 + a1) + (a2 + a3);
        const uint4 pf0 = make_uint4(pk[0], pk[1], pk[2], pk[3]), pf1 = make_uint4(pk[4], pk[5], pk[6], pk[7]);
        const uint4 v00 = a4_read128<SL * A4_SLOT>(va[0]), v01 = a4_read128<SL * A4_SLOT>(va[1]);
        const uint4 v10 = a4_read128<SL * A4_SLOT>(va[2]), v11 = a4_read128<SL * A4_SLOT>(va[3]);
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_sched_barrier(0);
        O0 = mfma32<F16>(v00, pf0, O0);
        O1 = mfma32<F16>(v10, pf0, O1);
        O0 = mfma32<F16>(v01, pf1, O0);
        O1 = mfma32<F16>(v11, pf1, O1);
        S = Sn;
    };
    using T0 = integral_constant<int, 0>;
    for (int kh0 = 0; kh0 < 28; kh0 += 4) {
        tile(kh0 + 0, integral_constant<int, 0>{}, integral_constant<int, 1>{}, T0{});
        tile(kh0 + 1, integral_constant<int, 1>{}, integral_constant<int, 2>{}, T0{});
        tile(kh0 + 2, integral_constant<int, 2>{}, integral_constant<int, 3>{}, T0{});
        tile(kh0 + 3, integral_constant<int, 3>{}, integral_constant<int, 0>{}, T0{});
    }
    tile(28, integral_constant<int, 0>{}, integral_constant<int, 1>{}, T0{});
    tile(29, integral_constant<int, 1>{}, integral_constant<int, 2>{}, integral_constant<int, 1>{});
    tile(30, integral_constant<int, 2>{}, integral_constant<int, 3>{}, integral_constant<int, 2>{});
    tile(31, integral_constant<int, 3>{}, integral_constant<int, 0>{}, integral_constant<int, 3>{});
    const float inv = 1.0f / (l_run + __shfl_xor(l_run, 32));
    unsigned short *orow = out + (tok0 + qh * 32 + r) * 1024 + head * 64;
    // a lane holds 4 consecutive channels (8 bytes) per group g4, its partner lane + 32 the next 4: one v_permlane32_swap per dword and
    // group pair (vdst = group g4, src = group g4 + 1) leaves the lower half-wave with channels 8 g4 .. + 7 and the upper one with
    // 8 (g4 + 1) .. + 7 -> four 16-byte stores per lane instead of eight 8-byte ones
#pragma unroll
    for (int db = 0; db < 2; ++db)
#pragma unroll
        for (int g4 = 0; g4 < 4; g4 += 2) {
            const f32x16 &O = db ? O1 : O0;
            unsigned ax = pack2<F16>(O[4 * g4 + 0] * inv, O[4 * g4 + 1] * inv), ay = pack2<F16>(O[4 * g4 + 2] * inv, O[4 * g4 + 3] * inv);
            unsigned bx = pack2<F16>(O[4 * g4 + 4] * inv, O[4 * g4 + 5] * inv), by = pack2<F16>(O[4 * g4 + 6] * inv, O[4 * g4 + 7] * inv);
            const auto rx = __builtin_amdgcn_permlane32_swap(ax, bx, false, false);
            const auto ry = __builtin_amdgcn_permlane32_swap(ay, by, false, false);
            *reinterpret_cast<uint4 *>(orow + db * 32 + 8 * g4 + 8 * h2) = make_uint4(rx[0], ry[0], rx[1], ry[1]);
        }
}

CPX_SWITCH(g_att_xcd, 1);          // XCD-aware workgroup order
CPX_SWITCH(g_att_v8, 2);           // 2: two query rows per wave, two workgroups per CU (k_attention2w, production); 7: 4-wave kernel with the
                                   // LDS-DMA ring and software-pipelined S (k_attention4p, rounds 2-5)
#ifdef CPX_DEBUG
extern "C" void cpx_attention_set_variant(int v8) { g_att_v8 = v8; }
extern "C" void cpx_attention_set_xcd_order(int v) { g_att_xcd = v; }
#endif
extern "C" int cpx_attention_relpos(const void *qkv, const void *rel_h, const void *rel_w,
                                    int n_subtiles, void *vT_ws, void *out, void *stream) {
    return cpx_attention_half(CPX_DT_BF16, qkv, rel_h, rel_w, n_subtiles, vT_ws, out, stream, true);
}
extern "C" int cpx_attention(int dtype, const void *qkv, const void *rel_h, const void *rel_w,
                             int n_subtiles, void *vT_ws, void *out, void *stream) {
    if (dtype == CPX_DT_F32)
        return cpx_attention_f32((const float *)qkv, (const float *)rel_h, (const float *)rel_w, n_subtiles, (float *)out, stream);
    return cpx_attention_half(dtype, qkv, rel_h, rel_w, n_subtiles, vT_ws, out, stream, true);
}
// transpose_v = false: vT_ws already holds V^T (written by the qkv GEMM's CPX_EPI_QKV_BF16 epilogue)
int cpx_attention_half(int dtype, const void *qkv, const void *rel_h, const void *rel_w, int n_subtiles,
                       void *vT_ws, void *out, void *stream, bool transpose_v) {
    CPX_REQUIRE(qkv && rel_h && rel_w && vT_ws && out && n_subtiles > 0);
    CPX_REQUIRE(dtype == CPX_DT_BF16 || dtype == CPX_DT_F16);
#ifdef CPX_DEBUG
    CPX_REQUIRE(g_att_v8 == 2 || g_att_v8 == 7);
#endif
    hipStream_t s = (hipStream_t)stream;
    if (transpose_v)
        hipLaunchKernelGGL(k_v_transpose, dim3(16, 16, n_subtiles), dim3(256), 0, s,
                           (const unsigned short *)qkv, (unsigned short *)vT_ws);
    // production: two query rows per wave, two workgroups per CU (cpx_attn2w.hip).  The debug library keeps the round-2/3 kernel
    // k_attention4p as variant 7, the bitwise reference of tests/test_gpu_attn2w.py
#ifdef CPX_DEBUG
    if (g_att_v8 == 7) {
        const dim3 grid4(8, 16, n_subtiles);
        static CpxOncePerDevice once4;
        once4([] {
            (void)hipFuncSetAttribute((const void *)k_attention4p<true>, hipFuncAttributeMaxDynamicSharedMemorySize, A4_LDS_BYTES);
            (void)hipFuncSetAttribute((const void *)k_attention4p<false>, hipFuncAttributeMaxDynamicSharedMemorySize, A4_LDS_BYTES);
        });
        if (dtype == CPX_DT_F16)
            hipLaunchKernelGGL((k_attention4p<true>), grid4, dim3(ATT_THREADS), A4_LDS_BYTES, s, (const unsigned short *)qkv, (const unsigned short *)vT_ws,
                               (const unsigned short *)rel_h, (const unsigned short *)rel_w, (unsigned short *)out, g_att_xcd);
        else
            hipLaunchKernelGGL((k_attention4p<false>), grid4, dim3(ATT_THREADS), A4_LDS_BYTES, s, (const unsigned short *)qkv, (const unsigned short *)vT_ws,
                               (const unsigned short *)rel_h, (const unsigned short *)rel_w, (unsigned short *)out, g_att_xcd);
        CPX_CHECK_LAUNCH();
        return CPX_OK;
    }
#endif
    return cpx_attention2w_launch(dtype, qkv, vT_ws, rel_h, rel_w, n_subtiles, out, g_att_xcd, s);
}

// ---------------------------------------------------------------------------
// forward driver
// ---------------------------------------------------------------------------
// one layout for both drivers: a zero-size request adds nothing to the offset, so the half types (no col) and float32 (no vt, no st)
// each see their requests back to back
NetWs cpx_net_ws(int nS, int dtype) {
    NetWs w; CpxArena a; const size_t M = (size_t)nS * 1024, es = es_of(dtype);
    w.off_x = a.take(M * 1024 * es);
    w.off_xn = a.take(M * 1024 * es);
    w.off_qkv = a.take(M * 3072 * es);
    w.off_vt = a.take(es == 2 ? M * 1024 * es : 0);
    w.off_ao = a.take(M * 1024 * es);
    w.off_h = a.take(M * 4096 * es);
    w.off_neck = a.take(M * 256 * es);
    w.off_neck2 = a.take(M * 256 * es);
    w.off_st = a.take(es == 2 ? M * 8 * sizeof(float) : 0);
    w.off_col = a.take(es == 4 ? M * 2304 * es : 0);
    w.total = a.o;
    return w;
}
extern "C" size_t cpx_net_workspace_bytes(int n_subtiles, int dtype) {
    return n_subtiles > 0 ? cpx_net_ws(n_subtiles, dtype).total : 0;
}

// where cpx_net_forward leaves the neck output [n_subtiles * 1024][256] (element type = network dtype; the operand of the head GEMM) in its
// workspace: the features a frozen-backbone training step starts from (cpx_train.hip).  0 for an invalid argument (the offset is never 0).
extern "C" size_t cpx_net_neck_offset(int n_subtiles, int dtype) {
    if (n_subtiles <= 0 || dtype < CPX_DT_BF16 || dtype > CPX_DT_F32) return 0;
    return cpx_net_ws(n_subtiles, dtype).off_neck2;
}

// where cpx_net_forward leaves the last block's output x [n_subtiles * 1024][1024] (network dtype; the operand of the neck's first GEMM):
// what a step that trains the neck starts from (cpx_train_neck.hip).  The tail only reads it.  (size_t)-1 for an invalid argument: the
// offset itself is 0 in both layouts.
extern "C" size_t cpx_net_backbone_offset(int n_subtiles, int dtype) {
    if (n_subtiles <= 0 || dtype < CPX_DT_BF16 || dtype > CPX_DT_F32) return (size_t)-1;
    return cpx_net_ws(n_subtiles, dtype).off_x;
}

// ---------------------------------------------------------------------------
// optional per-launch timing (bench.py's roofline lines): HIP events recorded on the launch
// stream around the selected kernels of a forward.  The handle is created by the caller (never
// inside the launch path), carried in cpx_net_weights.prof and owned by ONE engine / host thread.
// ---------------------------------------------------------------------------
extern "C" int cpx_prof_create(int max_launches, int stride, unsigned kinds_mask, void **out) {
    CPX_REQUIRE(out && max_launches > 0);
    CpxProf *p = new CpxProf();
    p->ev = new hipEvent_t[2 * (size_t)max_launches];
    p->kind = new int[max_launches];
    for (int i = 0; i < 2 * max_launches; ++i) {
        hipError_t e = hipEventCreate(&p->ev[i]);
        if (e != hipSuccess) {
            for (int j = 0; j < i; ++j) (void)hipEventDestroy(p->ev[j]);
            delete[] p->ev; delete[] p->kind; delete p;
            CPX_HIP(e);
        }
    }
    p->cap = max_launches; p->n = 0; p->stride = stride > 0 ? stride : 1;
    p->kinds_mask = kinds_mask ? kinds_mask : 1u;
    *out = p;
    return CPX_OK;
}
// per kind: sum of elapsed ms and number of timed launches since the last collect; call after a stream sync.
// ms_sum / count: arrays of CPX_PROF_N_KINDS (7) entries: fc1, attention, qkv, proj, fc2, patch embedding, neck + head (one span).
extern "C" int cpx_prof_collect(void *prof, double *ms_sum, int *count) {
    CpxProf *p = (CpxProf *)prof;
    CPX_REQUIRE(p && ms_sum && count);
    for (int k = 0; k < CPX_PROF_KINDS; ++k) { ms_sum[k] = 0.0; count[k] = 0; }
    for (int i = 0; i < p->n; ++i) {
        float ms = 0.f;
        CPX_HIP(hipEventElapsedTime(&ms, p->ev[2 * i], p->ev[2 * i + 1]));
        ms_sum[p->kind[i]] += ms;
        ++count[p->kind[i]];
    }
    p->n = 0;
    return CPX_OK;
}
// every timed launch since the last collect, in launch order: ms[i] / kind[i] for i < min(n, cap), *n_out = n.  Does not reset
// (call it before cpx_prof_collect); after a stream sync.  bench.py turns these into min / median / max per stage.
extern "C" int cpx_prof_collect_launches(void *prof, float *ms, int *kind, int cap, int *n_out) {
    CpxProf *p = (CpxProf *)prof;
    CPX_REQUIRE(p && ms && kind && n_out && cap >= 0);
    for (int i = 0; i < p->n && i < cap; ++i) {
        CPX_HIP(hipEventElapsedTime(&ms[i], p->ev[2 * i], p->ev[2 * i + 1]));
        kind[i] = p->kind[i];
    }
    *n_out = p->n;
    return CPX_OK;
}
extern "C" void cpx_prof_destroy(void *prof) {
    CpxProf *p = (CpxProf *)prof;
    if (!p) return;
    for (int i = 0; i < 2 * p->cap; ++i) (void)hipEventDestroy(p->ev[i]);
    delete[] p->ev; delete[] p->kind; delete p;
}

// number of row parts the MLP of a layer runs in (mlp.lin1 -> mlp.lin2 per part): floor(n_subtiles / 16) parts of 16 384 token rows (the last one with the
// remainder) when the batch has >= 32 sub-tiles (the hidden activations of a part, 134 MB at 2 bytes, then stay in the Infinity Cache between the two GEMMs), else 1.
// bench.py prices an mlp.lin1 / mlp.lin2 launch with n_subtiles / parts * 1024 rows (exact when 16 divides the batch, as in its headline).
CPX_SWITCH(g_mlp_parts, 1);        // 1 = the MLP in row parts (production), 0 = one launch pair over all rows (A/B)
#ifdef CPX_DEBUG
extern "C" void cpx_net_set_mlp_parts(int on) { g_mlp_parts = on; }
#endif
extern "C" int cpx_net_mlp_parts(int n_subtiles, int dtype) {
    if (!g_mlp_parts || dtype == CPX_DT_F32 || n_subtiles < 32) return 1;
    return n_subtiles / 16;
}
// rows of part pt (round 6: ANY batch of >= 32 sub-tiles is split, not only multiples of 16 -- the reference's default 1024-px tile makes 25 sub-tiles,
// 8 tiles per launch = 200: until round 5 their 1.68 GB of hidden activations went out to HBM and back in every layer).  floor(n / 16) parts of exactly
// 16 sub-tiles = 16 384 rows -- mlp.lin2 then has 256 output tiles, one per CU: parts of 18 432 rows (288 tiles) were measured first and cost two rounds of
// workgroups for 1.125 rounds of work -- and the LAST part takes the remainder as well (16 .. 31 sub-tiles)
static void mlp_part_rows(int n_subtiles, int parts, int pt, int &row0, int &rows) {
    row0 = pt * 16384;
    rows = pt + 1 < parts ? 16384 : n_subtiles * 1024 - row0;
}

// the network tail, for cpx_net_forward and the neck's training forward (cpx_train_neck.hip): one launch sequence per dtype.
// The plain GEMMs take one epilogue code for all dtypes: float32 has a single store-as-is instantiation (cpx_gemm_f32)
int cpx_net_tail(const cpx_net_weights *w, const void *x, int nS, void *y0, void *a1, void *y2, void *feat, void *col, float *head,
                 void *unet_ws, size_t unet_ws_bytes, void *stream) {
    const int dt = w->dtype, M = nS * 1024;
    // neck: 1x1 conv -> LN2d -> 3x3 conv -> LN2d
    CPX_RUN(cpx_gemm(dt, x, w->neck0_w, M, 256, 1024, CPX_EPI_BF16, nullptr, nullptr, y0, 256, stream));
    CPX_RUN(cpx_layernorm(dt, y0, w->neck_ln1_w, w->neck_ln1_b, M, 256, 1e-6f, a1, stream));
    if (dt == CPX_DT_F32) {         // im2col [M][9 x 256], then the GEMM
        CPX_RUN(cpx_im2col3_f32((const float *)a1, nS, (float *)col, stream));
        CPX_RUN(cpx_gemm(dt, col, w->neck2_w, M, 256, 2304, CPX_EPI_BF16, nullptr, nullptr, y2, 256, stream));
    } else {                        // an implicit GEMM (K = 9 x 256, the shifted operand is read by the LDS-DMA itself: no im2col buffer)
        CPX_RUN(cpx_conv3_half(dt, a1, w->neck2_w, M, 256, 256, CPX_EPI_BF16, nullptr, y2, 256, stream));
    }
    CPX_RUN(cpx_layernorm(dt, y2, w->neck_ln2_w, w->neck_ln2_b, M, 256, 1e-6f, feat, stream));
    // heads: out (192) | out_class (ncls*64), f32 token-major
    CPX_RUN(cpx_gemm(dt, feat, w->head_w, M, w->ld_head, 256, CPX_EPI_F32, w->head_b, nullptr, head, w->ld_head, stream));
    if (w->n_unet_ops > 0) {        // UNet semantic head overwrites the class columns (head_w rows there are zero)
        const size_t need = cpx_unet_ws_bytes(dt, w->unet_ops, w->n_unet_ops, nS);
        CPX_REQUIRE(unet_ws_bytes >= need);
        CPX_RUN(cpx_unet_head_run(dt, w->unet_ops, w->n_unet_ops, feat, nS, head, w->ld_head, 192, unet_ws, need, stream));
    }
    return CPX_OK;
}

#define TIMED(kind_, layer_, call_) do { const bool t_ = cpx_prof_begin(prof, kind_, layer_, hs); CPX_RUN(call_); if (t_) cpx_prof_end(prof, hs); } while (0)

// LayerNorm fusion: the RESID GEMMs emit partial row statistics of the residual stream, the next GEMM applies (x - mean) * rstd
// algebraically in its epilogue (weights pre-folded) -- where both RESID shapes run on the 256^2 kernel; else cpx_row_stats_half
bool cpx_net_big_stats(const cpx_net_weights *w, int nS) {
    const int M = nS * 1024;
    return w->fuse_ln && w->dtype != CPX_DT_F32 && cpx_gemm_half_uses_big_tile(M, 1024, 1024, CPX_EPI_RESID_BF16) &&
           cpx_gemm_half_uses_big_tile(M, 1024, 4096, CPX_EPI_RESID_BF16);
}

// one block (cpx_internal.h): two launch sequences, LayerNorm folded (half types) and plain (every dtype; float32 keeps its qkv rows
// whole and has an attention kernel of its own)
int cpx_net_block(const cpx_net_weights *w, int layer, int nS, const CpxBlockBufs &t, bool big_stats, CpxProf *prof, void *stream) {
    const cpx_block_weights &b = w->blocks[layer];
    const int dt = w->dtype, M = nS * 1024;
    const bool f32 = dt == CPX_DT_F32;
    hipStream_t hs = (hipStream_t)stream;
    auto attention = [&] {
        return f32 ? cpx_attention_f32((const float *)t.qkv, (const float *)b.rel_h, (const float *)b.rel_w, nS, (float *)t.ao, stream)
                   : cpx_attention_half(dt, t.qkv, b.rel_h, b.rel_w, nS, t.vt, t.ao, stream, false);
    };
    if (w->fuse_ln) {
        TIMED(CPX_PROF_QKV, layer, cpx_gemm_half(dt, t.x_in, b.qkv_w, M, 3072, 1024, CPX_EPI_QKV_BF16, b.qkv_b, t.vt, t.qkv, 3072, t.st, b.qkv_colsum, nullptr, stream));
        TIMED(CPX_PROF_ATTN, layer, attention());
        TIMED(CPX_PROF_PROJ, layer, cpx_gemm_half(dt, t.ao, b.proj_w, M, 1024, 1024, CPX_EPI_RESID_BF16, b.proj_b, t.x_in, t.x_mid, 1024, nullptr, nullptr, big_stats ? t.st : nullptr, stream));
        if (!big_stats) CPX_RUN(cpx_row_stats_half(dt, t.x_mid, M, t.st, stream));
        // the MLP in row parts of 16 384 tokens (cpx_net_mlp_parts): a part's hidden activations (134 MB) are written by mlp.lin1 and read
        // back by mlp.lin2 straight away, from the 256 MB Infinity Cache, and every part re-uses the SAME hidden rows -- over all 32 768 rows
        // the 268 MB hidden tensor goes out to HBM and comes back (one-process A/B, tools/ab_mlp_msplit.py: 451.8 -> 444.0 us per layer's
        // MLP; with a hidden buffer of its own per part 457.5).  Rows are independent: same bits.
        const int parts = big_stats ? cpx_net_mlp_parts(nS, dt) : 1;
        for (int pt = 0; pt < parts; ++pt) {
            int r0, Mp;
            mlp_part_rows(nS, parts, pt, r0, Mp);
            const char *xp = (const char *)t.x_mid + (size_t)r0 * 1024 * 2;
            char *op = (char *)t.x_out + (size_t)r0 * 1024 * 2;
            float *stp = t.st + (size_t)r0 * 8;
            TIMED(CPX_PROF_FC1, layer, cpx_gemm_half(dt, xp, b.fc1_w, Mp, 4096, 1024, CPX_EPI_GELU_BF16, b.fc1_b, nullptr, t.hb, 4096, stp, b.fc1_colsum, nullptr, stream));
            TIMED(CPX_PROF_FC2, layer, cpx_gemm_half(dt, t.hb, b.fc2_w, Mp, 1024, 4096, CPX_EPI_RESID_BF16, b.fc2_b, xp, op, 1024, nullptr, nullptr, big_stats ? stp : nullptr, stream));
        }
        if (!big_stats) CPX_RUN(cpx_row_stats_half(dt, t.x_out, M, t.st, stream));
        return CPX_OK;
    }
    CPX_RUN(cpx_layernorm(dt, t.x_in, b.ln1_w, b.ln1_b, M, 1024, 1e-6f, t.xn, stream));
    TIMED(CPX_PROF_QKV, layer, cpx_gemm(dt, t.xn, b.qkv_w, M, 3072, 1024, f32 ? CPX_EPI_F32 : CPX_EPI_QKV_BF16, b.qkv_b, f32 ? nullptr : t.vt, t.qkv, 3072, stream));
    TIMED(CPX_PROF_ATTN, layer, attention());
    TIMED(CPX_PROF_PROJ, layer, cpx_gemm(dt, t.ao, b.proj_w, M, 1024, 1024, CPX_EPI_RESID_BF16, b.proj_b, t.x_in, t.x_mid, 1024, stream));
    CPX_RUN(cpx_layernorm(dt, t.x_mid, b.ln2_w, b.ln2_b, M, 1024, 1e-6f, t.xn, stream));
    TIMED(CPX_PROF_FC1, layer, cpx_gemm(dt, t.xn, b.fc1_w, M, 4096, 1024, CPX_EPI_GELU_BF16, b.fc1_b, nullptr, t.hb, 4096, stream));
    TIMED(CPX_PROF_FC2, layer, cpx_gemm(dt, t.hb, b.fc2_w, M, 1024, 4096, CPX_EPI_RESID_BF16, b.fc2_b, t.x_mid, t.x_out, 1024, stream));
    return CPX_OK;
}

// ClassTransformer.forward (vit_sam.py:148-197) in w->dtype: patch embedding (+bias +pos_embed), the blocks, the tail
extern "C" int cpx_net_forward(const cpx_net_weights *w, const void *patches, int nS, float *head,
                               void *workspace, size_t workspace_bytes, void *stream) {
    CPX_REQUIRE(w && patches && head && workspace && nS > 0);
    CPX_REQUIRE(w->depth > 0 && w->blocks && w->ld_head % 128 == 0 && w->ld_head >= w->n_head_cols);
    CPX_REQUIRE(dtype_ok(w->dtype) && (w->dtype != CPX_DT_F32 || !w->fuse_ln));
    const int dt = w->dtype, M = nS * 1024;
    const NetWs L = cpx_net_ws(nS, dt);
    CPX_REQUIRE(workspace_bytes >= L.total);
    char *ws = (char *)workspace;
    void *x = ws + L.off_x, *nk = ws + L.off_neck, *nk2 = ws + L.off_neck2;
    float *st = (float *)(ws + L.off_st);
    const CpxBlockBufs t = {x, x, x, ws + L.off_xn, ws + L.off_qkv, ws + L.off_vt, ws + L.off_ao, ws + L.off_h, st};
    CpxProf *prof = (CpxProf *)w->prof;
    if (prof) prof->phase = (prof->phase + 1) % prof->stride;
    hipStream_t hs = (hipStream_t)stream;
    const bool big_stats = cpx_net_big_stats(w, nS);
    // on the 256^2 kernel (three K tiles) the patch embedding emits the first layer's row statistics itself
    const bool pe_stats = big_stats && cpx_gemm_half_uses_big_tile(M, 1024, 192, CPX_EPI_POS_BF16);
    TIMED(CPX_PROF_PE, 0, pe_stats ? cpx_gemm_half(dt, patches, w->pe_w, M, 1024, 192, CPX_EPI_POS_BF16, w->pe_b, w->pos, x, 1024, nullptr, nullptr, st, stream)
                                   : cpx_gemm(dt, patches, w->pe_w, M, 1024, 192, CPX_EPI_POS_BF16, w->pe_b, w->pos, x, 1024, stream));
    if (w->fuse_ln && !pe_stats) CPX_RUN(cpx_row_stats_half(dt, x, M, st, stream));
    for (int i = 0; i < w->depth; ++i) CPX_RUN(cpx_net_block(w, i, nS, t, big_stats, prof, stream));
    TIMED(CPX_PROF_TAIL, 0, cpx_net_tail(w, x, nS, nk, nk2, nk, nk2, ws + L.off_col, head, ws + L.total, workspace_bytes - L.total, stream));
    return CPX_OK;
}
#undef TIMED

// ---------------------------------------------------------------------------
// UNet semantic head (unet.py:121-196) as a list of convolutions on token-major tensors
// of element size ES (2: bf16 / fp16, 4: float32); one 16-byte chunk = 16 / ES channels
// ---------------------------------------------------------------------------
// gather for conv3x3 (pad 1) / conv2x2 stride 2 from up to two channel-concatenated sources
template <int ES>
__global__ void __launch_bounds__(256) k_conv_gather(const char *__restrict__ a, int lda, int ca,
                                                     const char *__restrict__ b, int ldb, int cb,
                                                     int kind, int h, int w, size_t rows_out, int kpad,
                                                     char *__restrict__ out) {
    constexpr int EPC = 16 / ES;                 // elements per 16-byte chunk
    const int ctot = ca + cb, ccn = ctot / EPC, taps = kind == 0 ? 9 : (kind == 1 ? 4 : 1);   // kind 3: plain repack
    const int chunks_per_row = kpad / EPC;
    size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= rows_out * chunks_per_row) return;
    size_t row = i / chunks_per_row;
    int ch = (int)(i - row * chunks_per_row);
    uint4 v = make_uint4(0, 0, 0, 0);
    const int ho = kind == 1 ? h >> 1 : h, wo = kind == 1 ? w >> 1 : w;
    if (ch < taps * ccn) {
        int tap = ch / ccn, cc = ch - tap * ccn;
        size_t s_ = row / (size_t)(ho * wo);
        int t = (int)(row - s_ * ho * wo), y = t / wo, x = t - y * wo;
        int yy, xx;
        if (kind == 0) { yy = y + tap / 3 - 1; xx = x + tap % 3 - 1; }
        else if (kind == 1) { yy = 2 * y + (tap >> 1); xx = 2 * x + (tap & 1); }
        else { yy = y; xx = x; }
        if ((unsigned)yy < (unsigned)h && (unsigned)xx < (unsigned)w) {
            size_t src_row = s_ * h * w + (size_t)yy * w + xx;
            int c = cc * EPC;
            v = c < ca ? *reinterpret_cast<const uint4 *>(a + (src_row * lda + c) * ES)
                       : *reinterpret_cast<const uint4 *>(b + (src_row * ldb + (c - ca)) * ES);
        }
    }
    *reinterpret_cast<uint4 *>(out + (row * kpad + (size_t)ch * EPC) * ES) = v;
}

// depth-to-space for convT2x2 s2: in [rows][ld_in] cols (tap, co) -> [4*rows][ld_out] or f32 head columns
// DT: CPX_DT_BF16 / CPX_DT_F16 / CPX_DT_F32
template <int DT>
__global__ void __launch_bounds__(256) k_depth2space(const char *__restrict__ in, int ld_in, int cout,
                                                     int h, int w, size_t rows_in, char *__restrict__ out,
                                                     int ld_out, float *__restrict__ out_f32, int ld_f32, int col0) {
    constexpr int ES = DT == CPX_DT_F32 ? 4 : 2, EPC = 16 / ES;
    const int ccn = cout / EPC;
    size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= rows_in * 4 * ccn) return;
    size_t row = i / (4 * ccn);
    int rem = (int)(i - row * 4 * ccn), tap = rem / ccn, cc = rem - tap * ccn;
    size_t s_ = row / (size_t)(h * w);
    int t = (int)(row - s_ * h * w), y = t / w, x = t - y * w;
    size_t orow = s_ * 4 * h * w + (size_t)(2 * y + (tap >> 1)) * (2 * w) + 2 * x + (tap & 1);
    uint4 v = *reinterpret_cast<const uint4 *>(in + (row * ld_in + tap * cout + cc * EPC) * ES);
    if (out_f32) {
        float *o = out_f32 + orow * ld_f32 + col0 + cc * EPC;
        if constexpr (DT == CPX_DT_F32) {
            *reinterpret_cast<uint4 *>(o) = v;
        } else {
            const unsigned u[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
            for (int k = 0; k < 4; ++k) { o[2 * k] = f32_from_h<DT == CPX_DT_F16>(u[k] & 0xFFFF); o[2 * k + 1] = f32_from_h<DT == CPX_DT_F16>(u[k] >> 16); }
        }
    } else {
        *reinterpret_cast<uint4 *>(out + (orow * ld_out + cc * EPC) * ES) = v;
    }
}

// workspace layout: [im2col staging][convT GEMM staging][one tensor [rows_out_pad][ld] per op] + 1024 bytes of slack.  The
// LAST op (a convT into the head) gets a slot too but never writes it: its GEMM output stays in the convT staging buffer
// and k_depth2space widens it straight into the head.  One helper for the size, the run and the debug layout entry.
struct UnetLayout {
    size_t col_off, g_off, total;
    size_t off[64];                      // op i's output tensor
    int ld[64];                          // its row stride in elements
};
static void unet_layout(int dtype, const cpx_conv_op *ops, int n_ops, int nS, UnetLayout &L) {
    const size_t es = es_of(dtype);
    size_t col_max = 0, g_max = 0;
    for (int i = 0; i < n_ops; ++i) {     // sizes of the shared staging buffers first
        const OpDims d = op_dims(ops[i], nS);
        col_max = std::max(col_max, (size_t)d.rows_pad * d.Kpad * es);
        if (ops[i].kind == 2) g_max = std::max(g_max, (size_t)d.rows_pad * d.Npad * es);
    }
    CpxArena a;
    L.col_off = a.take(col_max);
    L.g_off = a.take(g_max);
    for (int i = 0; i < n_ops && i < 64; ++i) {
        const OpDims d = op_dims(ops[i], nS);
        L.ld[i] = d.ld;
        L.off[i] = a.take((size_t)d.rows_out_pad * d.ld * es);
    }
    L.total = a.o + 1024;
}

size_t cpx_unet_ws_bytes(int dtype, const cpx_conv_op *ops, int n_ops, int nS) {
    if (!ops || n_ops <= 0 || n_ops > 64 || nS <= 0) return 0;
    UnetLayout L;
    unet_layout(dtype, ops, n_ops, nS, L);
    return L.total;
}
extern "C" size_t cpx_unet_workspace_bytes(const cpx_conv_op *ops, int n_ops, int nS, int dtype) {
    return cpx_unet_ws_bytes(dtype, ops, n_ops, nS);
}
// the saved activations of the head's backward pass (cpx_train_unet.hip): byte offset and row stride of every op's stored output
void cpx_unet_act_layout(int dtype, const cpx_conv_op *ops, int n_ops, int nS, size_t *off, int *ld) {
    UnetLayout L;
    unet_layout(dtype, ops, n_ops, nS, L);
    for (int i = 0; i < n_ops && i < 64; ++i) { off[i] = L.off[i]; ld[i] = L.ld[i]; }
}
#ifdef CPX_DEBUG
// where cpx_unet_head_run leaves each op's output in its workspace: byte offset and row stride (elements).  Op i < n_ops - 1:
// its output tensor [rows_pad][ld], channels 0 .. cout - 1 valid.  The last op (the convT into the head): its GEMM output
// before depth-to-space, [rows_in_pad][ld = up128(4 cout)] with column tap * cout + co, in the convT staging buffer.
extern "C" int cpx_unet_head_layout(const cpx_conv_op *ops, int n_ops, int nS, int dtype, size_t *dst_off, int *ld) {
    CPX_REQUIRE(ops && n_ops > 0 && n_ops <= 64 && nS > 0 && dst_off && ld && ops[n_ops - 1].kind == 2);
    UnetLayout L;
    unet_layout(dtype, ops, n_ops, nS, L);
    for (int i = 0; i < n_ops; ++i) { dst_off[i] = L.off[i]; ld[i] = L.ld[i]; }
    dst_off[n_ops - 1] = L.g_off;
    ld[n_ops - 1] = op_dims(ops[n_ops - 1], nS).Npad;
    return CPX_OK;
}
#endif

// feat: neck output [nS*1024][256] (tensor id 0).  The LAST op must be a convT producing
// ncls*64 channels at 32x32: it is written as float32 into head[:, col0 : col0 + cout].
int cpx_unet_head_run(int dtype, const cpx_conv_op *ops, int n_ops, const void *feat, int nS, float *head,
                      int ld_head, int col0, void *workspace, size_t ws_bytes, void *stream) {
    CPX_REQUIRE(ops && n_ops > 0 && n_ops <= 64 && feat && head && workspace && nS > 0);
    CPX_REQUIRE(ws_bytes >= cpx_unet_ws_bytes(dtype, ops, n_ops, nS));
    hipStream_t s = (hipStream_t)stream;
    const size_t es = es_of(dtype);
    CpxTensor tens[66];
    tens[0] = {(const char *)feat, 256, 256, 32, 32};
    char *ws = (char *)workspace;
    UnetLayout lay;
    unet_layout(dtype, ops, n_ops, nS, lay);
    char *colbuf = ws + lay.col_off, *gbuf = ws + lay.g_off;
    // (named float32 first: the order in which the instantiations have always stood in the code object; CPX_DT_DISPATCH would turn it round)
    const auto gather = es == 4 ? k_conv_gather<4> : k_conv_gather<2>;
    auto d2s = k_depth2space<CPX_DT_F32>;
    if (dtype != CPX_DT_F32) d2s = dtype == CPX_DT_F16 ? k_depth2space<CPX_DT_F16> : k_depth2space<CPX_DT_BF16>;
    for (int i = 0; i < n_ops; ++i) {
        const cpx_conv_op &o = ops[i];
        CPX_REQUIRE(o.dst > 0 && o.dst < 66 && o.src_a >= 0 && o.src_a < 66 && o.src_b < 66);
        CPX_REQUIRE(o.cin_a % 8 == 0 && o.cin_b % 8 == 0 && o.cout % 8 == 0 && o.weight && o.bias);
        const CpxTensor &A = tens[o.src_a];
        const CpxTensor Bz = {nullptr, 0, 0, 0, 0};
        const CpxTensor &B = o.src_b >= 0 ? tens[o.src_b] : Bz;
        CPX_REQUIRE(A.c == o.cin_a && A.h == o.h && A.w == o.w && (o.src_b < 0 || (B.c == o.cin_b && B.h == o.h && B.w == o.w)));
        if (o.kind == 2) CPX_REQUIRE(o.src_b < 0);
        const OpDims d = op_dims(o, nS);
        const bool convT = o.kind == 2;
        // im2col (convT: a plain repack, kind 3) into the staging buffer, then the GEMM: a convT's output goes to its own staging
        const dim3 grid_g((unsigned)((d.rows * (d.Kpad / (16 / es)) + 255) / 256));
        hipLaunchKernelGGL(gather, grid_g, dim3(256), 0, s, A.p, A.ld, o.cin_a, B.p, B.ld, convT ? 0 : o.cin_b, convT ? 3 : o.kind, o.h, o.w, d.rows, d.Kpad, colbuf);
        char *dst = ws + lay.off[i];
        const int rc = cpx_gemm(dtype, colbuf, o.weight, d.rows_pad, d.Npad, d.Kpad, !convT && o.relu ? CPX_EPI_RELU_BF16 : CPX_EPI_BF16, o.bias, nullptr,
                                convT ? gbuf : dst, d.Npad, stream);
        if (rc) return rc;
        if (convT) {                 // depth-to-space; the last op's goes into the head as float32
            const bool last = i == n_ops - 1;
            const dim3 grid((unsigned)((d.rows * 4 * (o.cout / (16 / es)) + 255) / 256));
            hipLaunchKernelGGL(d2s, grid, dim3(256), 0, s, gbuf, d.Npad, o.cout, o.h, o.w, d.rows, dst, d.ld, last ? head : nullptr, ld_head, col0);
        }
        tens[o.dst] = {dst, d.ld, o.cout, d.ho, d.wo};
    }
    CPX_CHECK_LAUNCH();
    return CPX_OK;
}
extern "C" int cpx_unet_head_forward(const cpx_conv_op *ops, int n_ops, const void *feat, int nS, float *head,
                                     int ld_head, int col0, int dtype, void *workspace, size_t ws_bytes, void *stream) {
    return cpx_unet_head_run(dtype, ops, n_ops, feat, nS, head, ld_head, col0, workspace, ws_bytes, stream);
}
