// Flash attention with the decomposed rel-pos bias (vit_sam.py:15-65, flash_forward): TWO image rows of queries per wave,
// TWO workgroups per CU (two waves per SIMD).  The production kernel (variant 2).
//
// The round-2/3 kernel (k_attention4p, cpx_net.hip; debug variant 7) runs one strictly serial chain per wave
// (K reads -> QK^T -> softmax -> V reads -> P.V -> barrier) and hides it behind three co-resident workgroups per CU; the
// round-4 one (k_attention2q, retired: git show f07d44d:classpose_amd/csrc/cpx_attn2q.hip) interleaves two chains per wave
// but runs one wave per SIMD, with nothing to hide its skeleton (ring, waits, barrier, seams) behind.  This kernel is the combination: each wave owns image rows
// 2 w and 2 w + 1 of its workgroup's 8 (chains 0 and 1) and alternates them in half steps --
//   half step A:  matrix pipe  S1 = K(t) Q1^T + Gw1,  O1 += V(t - 1) P1(t - 1)  |  vector pipe  P0(t) = softmax(S0)
//   half step B:  matrix pipe  S0 = K(t + 1) Q0^T + Gw0,  O0 += V(t) P0(t)     |  vector pipe  P1(t) = softmax(S1)
// -- both chains share every K / V^T fragment read, LDS-DMA request and barrier, and the footprint (<= 256 registers,
// 65 KB of LDS) lets two workgroups share a CU, so one wave's skeleton runs under its partner's stream.  The order of
// the two pipes' work inside a half step is left to the compiler (the two halves are fenced by sched_barrier).
//
// Per chain every arithmetic step is the one of k_attention4p, in the same order (S with Gw as the MFMA C operand, the
// exponent offset (gh - m_run) * cexp, the lazy-maximum vote per chain = per 32 queries, the f32 row-sum tree, the P.V
// accumulation order): the outputs are bitwise those of k_attention4p.
#include "cpx_internal.h"
#include <type_traits>

namespace {
typedef __attribute__((ext_vector_type(8))) __bf16 bf16x8;
typedef __attribute__((ext_vector_type(8))) _Float16 f16x8;
typedef __attribute__((ext_vector_type(2))) float f32x2;
typedef __attribute__((ext_vector_type(2))) __bf16 bf16x2;
typedef __attribute__((ext_vector_type(2))) _Float16 f16x2;
typedef __attribute__((ext_vector_type(4))) unsigned u32x4;

template <bool F16>
__device__ __forceinline__ f32x16 mfma32(const u32x4 &a, const u32x4 &b, f32x16 c) {
    if constexpr (F16)
        return __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(f16x8, a), __builtin_bit_cast(f16x8, b), c, 0, 0, 0);
    else
        return __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, a), __builtin_bit_cast(bf16x8, b), c, 0, 0, 0);
}
template <bool F16>
__device__ __forceinline__ unsigned pack2(float lo, float hi) {
    f32x2 v = {lo, hi};
    if constexpr (F16) return __builtin_bit_cast(unsigned, __builtin_convertvector(v, f16x2));
    else return __builtin_bit_cast(unsigned, __builtin_convertvector(v, bf16x2));
}
__device__ __forceinline__ int pi_perm(int r) { return (r & ~12) | ((r & 4) << 1) | ((r & 8) >> 1); }
template <int OFF>
__device__ __forceinline__ u32x4 a2w_read128(unsigned addr) {
    u32x4 v;
    asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(v) : "v"(addr), "n"(OFF));
    return v;
}
}  // namespace

#define A2W_THREADS 256
#define A2W_SLOT 8192                   // K tile (32 keys x 64 d) + V^T tile (64 d x 32 keys), halves
#define A2W_G_LD 66                     // padded row of the fp16 G scratch [wave][chain][32 q][66]
#define A2W_LDS_BYTES (4 * A2W_SLOT + 8 * 32 * A2W_G_LD * 2)
static_assert(A2W_LDS_BYTES <= 80 * 1024, "two workgroups per CU");

// Every LDS read inside the key loop is inline asm (with a DMA in flight hipcc drains it, vmcnt(0), in front of ordinary
// LDS reads of the same array); the counted waits carry the values they cover as operands, so that no consumer is
// scheduled in front of its wait.
template <bool F16>
__global__ void __launch_bounds__(A2W_THREADS, 2) k_attention2w(const unsigned short *__restrict__ qkv,
                                                                 const unsigned short *__restrict__ vT,
                                                                 const unsigned short *__restrict__ relh,
                                                                 const unsigned short *__restrict__ relw,
                                                                 unsigned short *__restrict__ out, int xcd_order) {
    extern __shared__ __attribute__((aligned(16))) char a2w_smem[];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int r = lane & 31, h2 = lane >> 5;
    // grid (4 row groups, 16 heads, n_subtiles); XCD-aware decode: the workgroups of one XCD (lin & 7) take whole
    // (sub-tile, head) pairs, all four row groups of a pair on the same XCD (its K / V^T stay in that L2)
    const int lin = (blockIdx.z * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x;
    int rg = blockIdx.x, head = blockIdx.y, s = blockIdx.z;
    if (xcd_order) {
        const int j = lin >> 3, pair = (j >> 2) * 8 + (lin & 7);
        rg = j & 3; head = pair & 15; s = pair >> 4;
    }
    const int qh0 = rg * 8 + wave * 2;                 // chains 0 / 1: image rows qh0, qh0 + 1
    const size_t tok0 = (size_t)s * 1024;
    // ---- ring requests: thread -> 16 bytes of K (key tid>>3, position tid&7) and of V^T (d tid>>2, position tid&3),
    // the source swizzles of k_attention4p (conflict-free fragment reads)
    const int kkey = tid >> 3, vd = tid >> 2;
    const unsigned short *ksrc = qkv + (tok0 + kkey) * 3072 + 1024 + head * 64 + (((tid & 7) ^ ((kkey >> 1) & 7)) * 8);
    const unsigned short *vsrc = vT + (((size_t)s * 16 + head) * 64 + vd) * 1024 + (((tid & 3) ^ ((vd >> 2) & 3)) * 8);
    char *dma_dst = a2w_smem + wave * 1024;
    auto issue = [&](int kh) {
        char *d = dma_dst + (kh & 3) * A2W_SLOT;
        __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void *)(ksrc + (size_t)kh * 32 * 3072),
                                         (__attribute__((address_space(3))) void *)d, 16, 0, 0);
        __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void *)(vsrc + kh * 32),
                                         (__attribute__((address_space(3))) void *)(d + 4096), 16, 0, 0);
    };
    issue(0); issue(1); issue(2);

    u32x4 qf[2][4];
#pragma unroll
    for (int c = 0; c < 2; ++c) {
        const unsigned short *qrow = qkv + (tok0 + (qh0 + c) * 32 + r) * 3072 + head * 64;
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) qf[c][ks] = *reinterpret_cast<const u32x4 *>(qrow + 16 * ks + 8 * h2);
    }
    // G = Q . table^T -> this wave's fp16 scratch [chain][q][j]; Gw goes to registers (the C operand of S), Gh stays in LDS
    f32x16 GW[2];
#pragma unroll
    for (int c = 0; c < 2; ++c) {
        _Float16 *G = reinterpret_cast<_Float16 *>(a2w_smem + 4 * A2W_SLOT) + (wave * 2 + c) * 32 * A2W_G_LD;
        auto compute_G = [&](const unsigned short *table) {
#pragma unroll
            for (int jb = 0; jb < 2; ++jb) {
                f32x16 acc;
#pragma unroll
                for (int i = 0; i < 16; ++i) acc[i] = 0.f;
#pragma unroll
                for (int ks = 0; ks < 4; ++ks) {
                    const u32x4 tf = *reinterpret_cast<const u32x4 *>(table + (jb * 32 + r) * 64 + 16 * ks + 8 * h2);
                    acc = mfma32<F16>(tf, qf[c][ks], acc);
                }
#pragma unroll
                for (int i = 0; i < 16; ++i) G[r * A2W_G_LD + jb * 32 + (i & 3) + 8 * (i >> 2) + 4 * h2] = (_Float16)acc[i];
            }
        };
        compute_G(relw);
#pragma unroll
        for (int i = 0; i < 16; ++i) GW[c][i] = (float)G[r * A2W_G_LD + (r - pi_perm((i & 3) + 8 * (i >> 2) + 4 * h2) + 31)];
        compute_G(relh);
    }
    asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");      // tiles 0..2 and this wave's G rows have landed
    __builtin_amdgcn_s_barrier();

    // per-lane LDS byte addresses of the fragments (slot offset added as an immediate)
    const unsigned lds0 = (unsigned)(size_t)(__attribute__((address_space(3))) char *)a2w_smem;
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
    // Gh[q][qh - kh + 31] of chain c: the address for kh = 0, minus 2 bytes per key tile
    unsigned gaddr[2];
#pragma unroll
    for (int c = 0; c < 2; ++c)
        gaddr[c] = lds0 + 4u * A2W_SLOT + (unsigned)((((wave * 2 + c) * 32 + r) * A2W_G_LD + qh0 + c + 31) * 2);

    // pipeline fill: K(0) fragments, gh of tile 0 for both chains, S0 = K(0) Q0^T + Gw0
    u32x4 kf[4], vf[4];
    unsigned ghb[2];
    kf[0] = a2w_read128<0>(ka[0]); kf[1] = a2w_read128<0>(ka[1]);
    kf[2] = a2w_read128<0>(ka[2]); kf[3] = a2w_read128<0>(ka[3]);
    asm volatile("ds_read_u16 %0, %1" : "=v"(ghb[0]) : "v"(gaddr[0]));
    asm volatile("ds_read_u16 %0, %1" : "=v"(ghb[1]) : "v"(gaddr[1]));
    asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(kf[0]), "+v"(kf[1]), "+v"(kf[2]), "+v"(kf[3]), "+v"(ghb[0]), "+v"(ghb[1])::"memory");
    f32x16 S[2], O0[2], O1[2];
    S[0] = mfma32<F16>(kf[0], qf[0][0], GW[0]);
    S[0] = mfma32<F16>(kf[1], qf[0][1], S[0]);
    S[0] = mfma32<F16>(kf[2], qf[0][2], S[0]);
    S[0] = mfma32<F16>(kf[3], qf[0][3], S[0]);
#pragma unroll
    for (int c = 0; c < 2; ++c)
#pragma unroll
        for (int i = 0; i < 16; ++i) { O0[c][i] = 0.f; O1[c][i] = 0.f; }
    float m_run[2] = {-1e30f, -1e30f}, l_run[2] = {0.f, 0.f};
    u32x4 pf[2][2];
    const float cexp = 0.125f * 1.44269504088896340736f;
    constexpr float HEADROOM = F16 ? 3.0f : 6.0f;
    using std::integral_constant;

    // softmax of chain C for one key tile (k_attention4p's, step for step): packed P -> pf[C], row sums -> l_run[C]
    auto softmax = [&](auto chain_tag, unsigned gh_bits) {
        constexpr int C = decltype(chain_tag)::value;
        const float gh = (float)__builtin_bit_cast(_Float16, (unsigned short)gh_bits);
        float p[16];
        unsigned pk[8];
        {
            const float off = (gh - m_run[C]) * cexp;
#pragma unroll
            for (int i = 0; i < 16; ++i) p[i] = __builtin_amdgcn_exp2f(__builtin_fmaf(S[C][i], cexp, off));
#pragma unroll
            for (int j = 0; j < 8; ++j) pk[j] = pack2<F16>(p[2 * j], p[2 * j + 1]);
        }
        // the row-sum tree before the vote (the p die early; the rare path below recomputes it)
        float a0 = (p[0] + p[1]) + (p[2] + p[3]), a1 = (p[4] + p[5]) + (p[6] + p[7]);
        float a2 = (p[8] + p[9]) + (p[10] + p[11]), a3 = (p[12] + p[13]) + (p[14] + p[15]);
        if (__builtin_expect(__any(((pk[0] | pk[1] | pk[2]) | (pk[3] | pk[4] | pk[5]) | (pk[6] | pk[7])) & 0x40004000u), 0)) {
            // some p >= 2 (or the reference is still -inf): exact maximum, rescale, recompute
            float mx = __builtin_fmaxf(__builtin_fmaxf(S[C][0], S[C][1]), S[C][2]);
#pragma unroll
            for (int i = 3; i < 15; i += 2) mx = __builtin_fmaxf(__builtin_fmaxf(mx, S[C][i]), S[C][i + 1]);
            mx = __builtin_fmaxf(mx, S[C][15]);
            mx = __builtin_fmaxf(mx, __shfl_xor(mx, 32)) + gh + HEADROOM / cexp;
            const float m_new = __builtin_fmaxf(m_run[C], mx);
            const float alpha = __builtin_amdgcn_exp2f((m_run[C] - m_new) * cexp);
            m_run[C] = m_new;
            l_run[C] *= alpha;
#pragma unroll
            for (int i = 0; i < 16; ++i) { O0[C][i] *= alpha; O1[C][i] *= alpha; }
            const float off = (gh - m_run[C]) * cexp;
#pragma unroll
            for (int i = 0; i < 16; ++i) p[i] = __builtin_amdgcn_exp2f(__builtin_fmaf(S[C][i], cexp, off));
#pragma unroll
            for (int j = 0; j < 8; ++j) pk[j] = pack2<F16>(p[2 * j], p[2 * j + 1]);
            a0 = (p[0] + p[1]) + (p[2] + p[3]); a1 = (p[4] + p[5]) + (p[6] + p[7]);
            a2 = (p[8] + p[9]) + (p[10] + p[11]); a3 = (p[12] + p[13]) + (p[14] + p[15]);
        }
        l_run[C] += (a0 + a1) + (a2 + a3);
        pf[C][0] = (u32x4){pk[0], pk[1], pk[2], pk[3]};
        pf[C][1] = (u32x4){pk[4], pk[5], pk[6], pk[7]};
    };
    // O_C += V(t) P_C(t), the accumulation order of k_attention4p
    auto pv = [&](auto chain_tag) {
        constexpr int C = decltype(chain_tag)::value;
        O0[C] = mfma32<F16>(vf[0], pf[C][0], O0[C]);
        O1[C] = mfma32<F16>(vf[2], pf[C][0], O1[C]);
        O0[C] = mfma32<F16>(vf[1], pf[C][1], O0[C]);
        O1[C] = mfma32<F16>(vf[3], pf[C][1], O1[C]);
    };
    auto qk = [&](auto chain_tag) {
        constexpr int C = decltype(chain_tag)::value;
        S[C] = mfma32<F16>(kf[0], qf[C][0], GW[C]);
        S[C] = mfma32<F16>(kf[1], qf[C][1], S[C]);
        S[C] = mfma32<F16>(kf[2], qf[C][2], S[C]);
        S[C] = mfma32<F16>(kf[3], qf[C][3], S[C]);
    };
    using C0 = integral_constant<int, 0>;
    using C1 = integral_constant<int, 1>;

    // one key tile kh: SL = ring slot of tile kh, SN = of tile kh + 1; FIRST: kh = 0 (chain 1 has no previous P);
    // TAIL (compile time): 0 = kh <= 28, 1 / 2 / 3 = tiles 29 / 30 / 31, peeled
    auto tile = [&](const int kh, auto slot_tag, auto next_tag, auto tail_tag, auto first_tag) {
        constexpr int SL = decltype(slot_tag)::value, SN = decltype(next_tag)::value, TAIL = decltype(tail_tag)::value;
        constexpr bool FIRST = decltype(first_tag)::value;
        // tile kh + 1 (this thread's part) has landed; behind the barrier every part has, and every wave is done with
        // slot (kh - 1) & 3 (read in the middle of tile kh - 1), which the next request overwrites
        if constexpr (TAIL < 2) asm volatile("s_waitcnt vmcnt(2)" ::: "memory");
        else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();
        if constexpr (TAIL == 0) issue(kh + 3);
        unsigned ghn[2] = {0u, 0u};
        if constexpr (TAIL < 3) {
            asm volatile("ds_read_u16 %0, %1" : "=v"(ghn[0]) : "v"(gaddr[0] - 2u * (unsigned)(kh + 1)));
            asm volatile("ds_read_u16 %0, %1" : "=v"(ghn[1]) : "v"(gaddr[1] - 2u * (unsigned)(kh + 1)));
        }
        __builtin_amdgcn_sched_barrier(0);
        // half step A: S1 = K(kh) Q1^T + Gw1, O1 += V(kh - 1) P1(kh - 1) | softmax of chain 0, tile kh
        qk(C1{});
        if constexpr (!FIRST) pv(C1{});
        softmax(C0{}, ghb[0]);
        __builtin_amdgcn_sched_barrier(0);
        // K(kh + 1) and V(kh) into the fragment registers half step A has finished with (tile 31: V only).  (Issuing them
        // right behind half step A's MFMAs instead, under its softmax, measured slower: 201.4 against 196.1 us, and spills.)
        if constexpr (TAIL < 3) {
            kf[0] = a2w_read128<SN * A2W_SLOT>(ka[0]); kf[1] = a2w_read128<SN * A2W_SLOT>(ka[1]);
            kf[2] = a2w_read128<SN * A2W_SLOT>(ka[2]); kf[3] = a2w_read128<SN * A2W_SLOT>(ka[3]);
        }
        vf[0] = a2w_read128<SL * A2W_SLOT>(va[0]); vf[1] = a2w_read128<SL * A2W_SLOT>(va[1]);
        vf[2] = a2w_read128<SL * A2W_SLOT>(va[2]); vf[3] = a2w_read128<SL * A2W_SLOT>(va[3]);
        asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(kf[0]), "+v"(kf[1]), "+v"(kf[2]), "+v"(kf[3]), "+v"(vf[0]), "+v"(vf[1]),
                     "+v"(vf[2]), "+v"(vf[3]), "+v"(ghn[0]), "+v"(ghn[1])::"memory");
        __builtin_amdgcn_sched_barrier(0);
        // half step B: S0 = K(kh + 1) Q0^T + Gw0, O0 += V(kh) P0(kh) | softmax of chain 1, tile kh
        if constexpr (TAIL < 3) qk(C0{});
        pv(C0{});
        softmax(C1{}, ghb[1]);
        __builtin_amdgcn_sched_barrier(0);
        ghb[0] = ghn[0]; ghb[1] = ghn[1];
    };
    using T0 = integral_constant<int, 0>;
    using NF = std::false_type;
    tile(0, integral_constant<int, 0>{}, integral_constant<int, 1>{}, T0{}, std::true_type{});
    tile(1, integral_constant<int, 1>{}, integral_constant<int, 2>{}, T0{}, NF{});
    tile(2, integral_constant<int, 2>{}, integral_constant<int, 3>{}, T0{}, NF{});
    tile(3, integral_constant<int, 3>{}, integral_constant<int, 0>{}, T0{}, NF{});
    for (int kh0 = 4; kh0 < 28; kh0 += 4) {
        tile(kh0 + 0, integral_constant<int, 0>{}, integral_constant<int, 1>{}, T0{}, NF{});
        tile(kh0 + 1, integral_constant<int, 1>{}, integral_constant<int, 2>{}, T0{}, NF{});
        tile(kh0 + 2, integral_constant<int, 2>{}, integral_constant<int, 3>{}, T0{}, NF{});
        tile(kh0 + 3, integral_constant<int, 3>{}, integral_constant<int, 0>{}, T0{}, NF{});
    }
    tile(28, integral_constant<int, 0>{}, integral_constant<int, 1>{}, T0{}, NF{});
    tile(29, integral_constant<int, 1>{}, integral_constant<int, 2>{}, integral_constant<int, 1>{}, NF{});
    tile(30, integral_constant<int, 2>{}, integral_constant<int, 3>{}, integral_constant<int, 2>{}, NF{});
    tile(31, integral_constant<int, 3>{}, integral_constant<int, 0>{}, integral_constant<int, 3>{}, NF{});
    pv(C1{});                                          // pipeline drain: chain 1's last tile (V(31) is in vf)

    // normalise, round, store: a lane holds 4 consecutive channels per group g4, its partner lane + 32 the next 4; one
    // v_permlane32_swap per dword and group pair leaves 8 consecutive channels per lane -> 16-byte stores
#pragma unroll
    for (int c = 0; c < 2; ++c) {
        const float l_tot = l_run[c] + __shfl_xor(l_run[c], 32);
        const float inv = 1.0f / l_tot;
        unsigned short *orow = out + (tok0 + (qh0 + c) * 32 + r) * 1024 + head * 64;
#pragma unroll
        for (int db = 0; db < 2; ++db)
#pragma unroll
            for (int g4 = 0; g4 < 4; g4 += 2) {
                const f32x16 &O = db ? O1[c] : O0[c];
                unsigned ax = pack2<F16>(O[4 * g4 + 0] * inv, O[4 * g4 + 1] * inv), ay = pack2<F16>(O[4 * g4 + 2] * inv, O[4 * g4 + 3] * inv);
                unsigned bx = pack2<F16>(O[4 * g4 + 4] * inv, O[4 * g4 + 5] * inv), by = pack2<F16>(O[4 * g4 + 6] * inv, O[4 * g4 + 7] * inv);
                const auto rx = __builtin_amdgcn_permlane32_swap(ax, bx, false, false);
                const auto ry = __builtin_amdgcn_permlane32_swap(ay, by, false, false);
                *reinterpret_cast<uint4 *>(orow + db * 32 + 8 * g4 + 8 * h2) = make_uint4(rx[0], ry[0], rx[1], ry[1]);
            }
    }
}

// grid (4 row groups, 16 heads, n_subtiles) = 64 n_subtiles workgroups of 4 waves, 65 KB of LDS each; vT holds V^T already
int cpx_attention2w_launch(int dtype, const void *qkv, const void *vT, const void *rel_h, const void *rel_w,
                           int n_subtiles, void *out, int xcd_order, hipStream_t s) {
    static CpxOncePerDevice once;
    once([] {
        (void)hipFuncSetAttribute((const void *)k_attention2w<true>, hipFuncAttributeMaxDynamicSharedMemorySize, A2W_LDS_BYTES);
        (void)hipFuncSetAttribute((const void *)k_attention2w<false>, hipFuncAttributeMaxDynamicSharedMemorySize, A2W_LDS_BYTES);
    });
    const dim3 grid(4, 16, n_subtiles);
    if (dtype == CPX_DT_F16)
        hipLaunchKernelGGL((k_attention2w<true>), grid, dim3(A2W_THREADS), A2W_LDS_BYTES, s, (const unsigned short *)qkv,
                           (const unsigned short *)vT, (const unsigned short *)rel_h, (const unsigned short *)rel_w,
                           (unsigned short *)out, xcd_order);
    else
        hipLaunchKernelGGL((k_attention2w<false>), grid, dim3(A2W_THREADS), A2W_LDS_BYTES, s, (const unsigned short *)qkv,
                           (const unsigned short *)vT, (const unsigned short *)rel_h, (const unsigned short *)rel_w,
                           (unsigned short *)out, xcd_order);
    CPX_CHECK_LAUNCH();
    return CPX_OK;
}
