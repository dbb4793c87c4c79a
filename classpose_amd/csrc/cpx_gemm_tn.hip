// The weight-gradient GEMM of the mixed-precision block backward (gfx950): both operands transposed, bf16 in, float32 out.
//   out[n][k] (+)= sum_m A[m][n] * B[m][k]        A [M][N], B [M][K] bf16, token-major as the backward holds dy and a; out [N][ld_out] float32
// Both MFMA operands are columns of their [m][.] tiles, so no transposing copy is made: the tiles go to LDS as they lie in memory (16-byte
// chunks of a row) and ds_read_b64_tr_b16 delivers them column-major -- per 16-lane group a block of 4 rows x 16 columns, lane i of the
// group receiving column i with row q in element q.
//   tile      128 (n) x 128 (k) outputs per workgroup, 64 rows of m per stage; 4 waves, each 64 x 64 = 2 x 2 v_mfma_f32_32x32x16_bf16 tiles
//   LDS       per stage and operand [64 m][256 B]; two stages: 64 KB.  Chunk ch (16 B) of row m lies at
//             256 m + 16 (ch ^ (((m & 3) << 2) | ((m >> 2) & 3))).  A transposed read takes, per 32-lane half, rows r0 .. r0 + 3 (r0 a
//             multiple of 4) and four chunks c0 .. c0 + 3 (c0 a multiple of 4): the high two bits of the XOR (m & 3) send the four rows to
//             four different 64-byte quarters of the 256-byte bank row and the low two bits permute the chunks inside a quarter, so the 32
//             lanes' 8-byte reads cover the 64 banks once: no conflict.  A row's 16 chunk stores (one per lane of a 16-lane group) are a
//             permutation of the row: no conflict either.
//   operand   lane l of the MFMA holds row / column l & 31 and contraction slots 8 (l >> 5) .. + 7: two transposed reads of 4 rows each.  A
//             and B take their slots from the same rows m, which is all the product needs.
//   schedule  the next stage's 8 chunks per thread are loaded to registers before the current stage's 16 MFMAs per wave and stored after
//             them; one barrier per stage.  Every lane runs every instruction (no bounds branch: the shape requirements make all tiles
//             full), so EXEC is all ones at every transposed read.
//   sums      each output element is one accumulator chain over m in order, float32; `add` adds what out held once at the end.  No
//             atomics: bitwise reproducible.
#include "cpx_internal.h"

typedef __attribute__((ext_vector_type(8))) __bf16 tn_bf16x8;
typedef __attribute__((ext_vector_type(4))) short tn_s16x4;
typedef __attribute__((ext_vector_type(8))) short tn_s16x8;
typedef __attribute__((ext_vector_type(4))) unsigned tn_u32x4;

#define TN_BN 128
#define TN_BK 128
#define TN_BM 64
#define TN_TILE (TN_BM * 256)            // bytes of one operand's stage

__device__ __forceinline__ int tn_off(int row, int ch) { return 256 * row + 16 * (ch ^ (((row & 3) << 2) | ((row >> 2) & 3))); }

__device__ __forceinline__ tn_s16x4 tn_read(const unsigned char *p) {
    return __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) tn_s16x4 *)p);
}

template <bool ADD>
__global__ void __launch_bounds__(256) k_gemm_tn_bf16(const unsigned short *__restrict__ A, const unsigned short *__restrict__ B, int M, int N,
                                                      int K, float *__restrict__ out, int ld_out) {
    __shared__ __attribute__((aligned(16))) unsigned char lds[2][2][TN_TILE];      // [stage][A | B]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int n0 = blockIdx.y * TN_BN, k0 = blockIdx.x * TN_BK;
    const int wn = (wave >> 1) * 64, wk = (wave & 1) * 64;

    // staging: chunk id = tid + 256 j -> row id >> 4 (0 .. 63), chunk id & 15
    tn_u32x4 ra[4], rb[4];
    auto load = [&](int t) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int id = tid + 256 * j, row = id >> 4, ch = id & 15;
            const size_t m = (size_t)t * TN_BM + row;
            ra[j] = *reinterpret_cast<const tn_u32x4 *>(A + m * N + n0 + 8 * ch);
            rb[j] = *reinterpret_cast<const tn_u32x4 *>(B + m * K + k0 + 8 * ch);
        }
    };
    auto store = [&](int buf) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int id = tid + 256 * j, o = tn_off(id >> 4, id & 15);
            *reinterpret_cast<tn_u32x4 *>(&lds[buf][0][o]) = ra[j];
            *reinterpret_cast<tn_u32x4 *>(&lds[buf][1][o]) = rb[j];
        }
    };
    // the transposed read of lane l for the 32 columns from element column cb, contraction rows 16 ks + 8 (l >> 5) [+ 4]: lane 4 q + p of
    // its 16-lane group g supplies row q, columns 4 p .. 4 p + 3 of the block at column cb + 16 (g & 1)
    const int g = lane >> 4, q = (lane >> 2) & 3, p = lane & 3;
    const int rq = 8 * (g >> 1) + q, cg = 2 * (g & 1) + (p >> 1), ob = 8 * (p & 1);
    auto operand = [&](const unsigned char *tile, int cb, int ks) {
        const int c = (cb >> 3) + cg, r = 16 * ks + rq;
        const tn_s16x4 lo = tn_read(tile + tn_off(r, c) + ob), hi = tn_read(tile + tn_off(r + 4, c) + ob);
        const tn_s16x8 v = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
        return __builtin_bit_cast(tn_bf16x8, v);
    };

    f32x16 acc[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int v = 0; v < 16; ++v) acc[i][j][v] = 0.f;

    const int T = M / TN_BM;
    load(0);
    store(0);
    __syncthreads();
    for (int t = 0; t < T; ++t) {
        const int buf = t & 1;
        if (t + 1 < T) load(t + 1);                                   // (uniform in the workgroup)
#pragma unroll
        for (int ks = 0; ks < TN_BM / 16; ++ks) {
            tn_bf16x8 a[2], b[2];
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                a[i] = operand(lds[buf][0], wn + 32 * i, ks);
                b[i] = operand(lds[buf][1], wk + 32 * i, ks);
            }
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int j = 0; j < 2; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[i], b[j], acc[i][j], 0, 0, 0);
        }
        if (t + 1 < T) store(buf ^ 1);
        __syncthreads();
    }
    // accumulator register v of lane l: row (v & 3) + 8 (v >> 2) + 4 (l >> 5), column l & 31 of the 32 x 32 tile
    const int r = lane & 31, h2 = lane >> 5;
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
        {
            // (add: the tile's 16 previous values are loaded before its first store -- one load after another store to the same array
            // would wait for each in turn)
            float *o = out + (size_t)(n0 + wn + 32 * i + 4 * h2) * ld_out + k0 + wk + 32 * j + r;
            float prev[16];
#pragma unroll
            for (int v = 0; v < 16; ++v) prev[v] = ADD ? o[(size_t)((v & 3) + 8 * (v >> 2)) * ld_out] : 0.f;
#pragma unroll
            for (int v = 0; v < 16; ++v) o[(size_t)((v & 3) + 8 * (v >> 2)) * ld_out] = ADD ? prev[v] + acc[i][j][v] : acc[i][j][v];
        }
}

extern "C" int cpx_gemm_tn_bf16(const void *A, const void *B, int M, int N, int K, int add, float *out, int ld_out, void *stream) {
    CPX_REQUIRE(A && B && out && (add == 0 || add == 1));
    CPX_REQUIRE(M > 0 && N > 0 && K > 0 && M % TN_BM == 0 && N % TN_BN == 0 && K % TN_BK == 0);
    CPX_REQUIRE(ld_out >= K && N / TN_BN <= 65535);
    CPX_REQUIRE((((uintptr_t)A | (uintptr_t)B | (uintptr_t)out) & 15) == 0);
    const dim3 grid(K / TN_BK, N / TN_BN), block(256);
    hipStream_t s = (hipStream_t)stream;
    if (add) hipLaunchKernelGGL(k_gemm_tn_bf16<true>, grid, block, 0, s, (const unsigned short *)A, (const unsigned short *)B, M, N, K, out, ld_out);
    else hipLaunchKernelGGL(k_gemm_tn_bf16<false>, grid, block, 0, s, (const unsigned short *)A, (const unsigned short *)B, M, N, K, out, ld_out);
    CPX_CHECK_LAUNCH();
    return CPX_OK;
}
