// Training the neck with the backbone frozen (gfx950): the reference's `--freeze backbone` and `--freeze backbone segmentation_head`
// (classpose/vit_sam.py:216-249, paper_experiments/run_training.py:92-98).  The neck is the tail of cpx_net_forward,
//   y0 = x W0^T  ->  a1 = LayerNorm2d(y0)  ->  y2 = conv3x3(a1, W2)  ->  feat = LayerNorm2d(y2)  ->  head = feat Wh^T + bh,
// on the last block's output x [nS * 1024][1024], which cpx_net_forward leaves in its workspace (cpx_net_backbone_offset).
//   * cpx_neck_forward_train   the tail itself (cpx_net_tail, cpx_net.hip) with four tensors of their own: the saved activations
//   * k_ln_bwd / k_ln_bwd_finish   LayerNorm over channels (256, or the blocks' 1024), backward: one wave per row, everything formed in
//                              float64 and rounded once
//   * cpx_neck_backward        head data gradient -> LN2 -> conv3x3 (weight and data gradient) -> LN1 -> conv1x1 weight gradient; the
//                              convolutions run the kernels of the UNet head's backward (cpx_train_unet.hip, through cpx_internal.h)
// Rounding to the network dtype is the identity in the backward (straight-through).  No gradient leaves towards the backbone.
// Determinism: no atomics; every sum has a fixed order, so a pass is a function of its inputs only, bitwise.
#include "cpx_internal.h"
#include <algorithm>

#define NECK_C 256                 // channels of the neck
#define NECK_K0 1024               // channels of the backbone
#define NECK_K2 (9 * NECK_C)       // im2col width of the 3x3 conv, k = tap * 256 + c
#define LNB_ROWS 64                // rows per workgroup of k_ln_bwd: 16 per wave

// ---------------------------------------------------------------------------
// the training forward
// ---------------------------------------------------------------------------
// workspace: [y0][a1][y2][feat], each [rows][256] in the network dtype; float32 adds the im2col staging [rows][2304]
struct NeckFwdLayout { size_t off[4], off_col, total; };
static NeckFwdLayout neck_fwd_layout(int nS, int dtype) {
    NeckFwdLayout L; CpxArena a; const size_t rows = (size_t)nS * 1024;
    for (int i = 0; i < 4; ++i) L.off[i] = a.take(rows * NECK_C * es_of(dtype));
    L.off_col = a.take(dtype == CPX_DT_F32 ? rows * NECK_K2 * sizeof(float) : 0);
    L.total = a.o;
    return L;
}
extern "C" size_t cpx_neck_train_workspace_bytes(int nS, int dtype) {
    if (nS <= 0 || !dtype_ok(dtype)) return 0;
    return neck_fwd_layout(nS, dtype).total;
}
extern "C" int cpx_neck_train_layout(int nS, int dtype, size_t *off) {
    CPX_REQUIRE(nS > 0 && dtype_ok(dtype) && off);
    const NeckFwdLayout L = neck_fwd_layout(nS, dtype);
    for (int i = 0; i < 4; ++i) off[i] = L.off[i];
    return CPX_OK;
}

static bool neck_weights_ok(const cpx_net_weights *w) {
    return w && dtype_ok(w->dtype) && w->ld_head > 0 && w->ld_head % 128 == 0 && w->ld_head >= w->n_head_cols && w->neck0_w && w->neck_ln1_w &&
           w->neck_ln1_b && w->neck2_w && w->neck_ln2_w && w->neck_ln2_b && w->head_w && w->head_b &&
           w->n_unet_ops == 0;                    // the UNet head's backward gives the neck output no gradient: not trainable together
}

extern "C" int cpx_neck_forward_train(const cpx_net_weights *w, const void *x, int nS, float *head, void *workspace,
                                      size_t workspace_bytes, void *stream) {
    CPX_REQUIRE(neck_weights_ok(w) && x && head && workspace && nS > 0 && (size_t)nS * 1024 < 0x7fffffffull);
    const NeckFwdLayout L = neck_fwd_layout(nS, w->dtype);
    CPX_REQUIRE(workspace_bytes >= L.total && ((uintptr_t)workspace & 255) == 0 && ((uintptr_t)x & 15) == 0);
    char *ws = (char *)workspace;
    return cpx_net_tail(w, x, nS, ws + L.off[0], ws + L.off[1], ws + L.off[2], ws + L.off[3], ws + L.off_col, head, nullptr, 0, stream);
}

// ---------------------------------------------------------------------------
// LayerNorm over channels, backward
// ---------------------------------------------------------------------------
// the lane's four consecutive channels of a stored row, widened exactly: 16 bytes (float32) or 8 bytes (bf16 / fp16) per lane
template <int DT>
__device__ __forceinline__ void load4(const void *y, size_t idx, double v[4]) {
    if constexpr (DT == CPX_DT_F32) {
        const float4 a = *reinterpret_cast<const float4 *>((const float *)y + idx);
        v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w;
    } else {
        const uint2 a = *reinterpret_cast<const uint2 *>((const unsigned short *)y + idx);
        const unsigned short u[4] = {(unsigned short)(a.x & 0xFFFF), (unsigned short)(a.x >> 16), (unsigned short)(a.y & 0xFFFF), (unsigned short)(a.y >> 16)};
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            if constexpr (DT == CPX_DT_F16) { const unsigned short h = u[k]; v[k] = (double)(float)*reinterpret_cast<const _Float16 *>(&h); }
            else v[k] = (double)bf16_to_f32(u[k]);
        }
    }
}

// One wave owns whole rows: lane l holds C / 64 channels, four consecutive ones per group of 256 (channel 256 j + 4 l + k: C = 256, the
// neck, is one group; C = 1024, a transformer block's LayerNorm, four).  A workgroup owns LNB_ROWS consecutive rows, wave w rows
// 16 w .. 16 w + 15 of them.  Per row mean, biased variance and rstd are recomputed from y as stored; part [workgroup][2][C] float64
// receives the workgroup's column sums of dout * xhat and of dout (rows in order inside a wave, then wave 0 + 1 + 2 + 3).
template <int DT, int C>
__global__ void __launch_bounds__(256) k_ln_bwd(const void *__restrict__ y, const float *__restrict__ gamma, const float *__restrict__ dout,
                                                int rows, double eps, float *__restrict__ dy, double *__restrict__ part) {
    constexpr int PER = C / 64, NG = PER / 4;
    __shared__ double sm[4][2][C];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, c0 = lane * 4;
    double ga[PER], dg[PER], db[PER];
#pragma unroll
    for (int j = 0; j < NG; ++j) {
        const float4 gm = *reinterpret_cast<const float4 *>(gamma + 256 * j + c0);
        ga[4 * j] = gm.x; ga[4 * j + 1] = gm.y; ga[4 * j + 2] = gm.z; ga[4 * j + 3] = gm.w;
    }
#pragma unroll
    for (int k = 0; k < PER; ++k) { dg[k] = 0; db[k] = 0; }
    const int row0 = blockIdx.x * LNB_ROWS + wave * (LNB_ROWS / 4);
    const int row1 = min(rows, row0 + LNB_ROWS / 4);
    for (int row = row0; row < row1; ++row) {                         // (wave-uniform bounds)
        const size_t idx = (size_t)row * C + c0;
        double v[PER], d[PER];
#pragma unroll
        for (int j = 0; j < NG; ++j) {
            load4<DT>(y, idx + 256 * j, v + 4 * j);
            const float4 d4 = *reinterpret_cast<const float4 *>(dout + idx + 256 * j);
            d[4 * j] = d4.x; d[4 * j + 1] = d4.y; d[4 * j + 2] = d4.z; d[4 * j + 3] = d4.w;
        }
        double sv = v[0];
#pragma unroll
        for (int k = 1; k < PER; ++k) sv += v[k];
        const double mean = wave_sum(sv) / C;
        double q = 0;
#pragma unroll
        for (int k = 0; k < PER; ++k) { v[k] -= mean; q += v[k] * v[k]; }
        const double rstd = 1.0 / sqrt(wave_sum(q) / C + eps);
        double g[PER], sg = 0, sgx = 0;
#pragma unroll
        for (int k = 0; k < PER; ++k) { v[k] *= rstd; g[k] = d[k] * ga[k]; sg += g[k]; sgx += g[k] * v[k]; }     // v is xhat from here
        sg = wave_sum(sg) / C; sgx = wave_sum(sgx) / C;
#pragma unroll
        for (int j = 0; j < NG; ++j) {
            const int k = 4 * j;
            float4 o;
            o.x = (float)(rstd * ((g[k] - sg) - v[k] * sgx)); o.y = (float)(rstd * ((g[k + 1] - sg) - v[k + 1] * sgx));
            o.z = (float)(rstd * ((g[k + 2] - sg) - v[k + 2] * sgx)); o.w = (float)(rstd * ((g[k + 3] - sg) - v[k + 3] * sgx));
            *reinterpret_cast<float4 *>(dy + idx + 256 * j) = o;
        }
#pragma unroll
        for (int k = 0; k < PER; ++k) { dg[k] += d[k] * v[k]; db[k] += d[k]; }
    }
#pragma unroll
    for (int k = 0; k < PER; ++k) { sm[wave][0][256 * (k >> 2) + c0 + (k & 3)] = dg[k]; sm[wave][1][256 * (k >> 2) + c0 + (k & 3)] = db[k]; }
    __syncthreads();
    double *p = part + (size_t)blockIdx.x * 2 * C;
    for (int c = threadIdx.x; c < C; c += 256) {
        p[c] = ((sm[0][0][c] + sm[1][0][c]) + sm[2][0][c]) + sm[3][0][c];
        p[C + c] = ((sm[0][1][c] + sm[1][1][c]) + sm[2][1][c]) + sm[3][1][c];
    }
}

// workgroups of 512 over the 2 C sums: thread t = j * C + c (the offset inside a workgroup's record) adds sum j of column c over the
// partials in workgroup order, as k_seg_finish adds its records (the loads of eight partials are in flight together; the additions
// keep their order)
__global__ void __launch_bounds__(512) k_ln_bwd_finish(const double *__restrict__ part, int nblk, int C, float *__restrict__ dgamma,
                                                       float *__restrict__ dbeta) {
    const int t = blockIdx.x * 512 + threadIdx.x;
    double s = 0;
#pragma unroll 8
    for (int k = 0; k < nblk; ++k) s += part[(size_t)k * 2 * C + t];
    if (t < C) dgamma[t] = (float)s;
    else dbeta[t - C] = (float)s;
}

static int ln_nblk(int rows) { return (rows + LNB_ROWS - 1) / LNB_ROWS; }
static bool ln_c_ok(int C) { return C == NECK_C || C == NECK_K0; }
// cpx_layernorm_backward_workspace_bytes answers for the neck's C = 256 alone, as it always has; cpx_layernorm_backward_bytes for
// both widths
extern "C" size_t cpx_layernorm_backward_bytes(int rows, int C) {
    if (rows <= 0 || !ln_c_ok(C)) return 0;
    return cpx_align_up((size_t)ln_nblk(rows) * 2 * C * sizeof(double), 256);
}
extern "C" size_t cpx_layernorm_backward_workspace_bytes(int rows, int C) {
    return C == NECK_C ? cpx_layernorm_backward_bytes(rows, C) : 0;
}
extern "C" int cpx_layernorm_backward(int dtype, const void *y, const float *gamma, const float *dout, int rows, int C, float eps,
                                      float *dy, float *dgamma, float *dbeta, void *workspace, size_t workspace_bytes, void *stream) {
    CPX_REQUIRE(y && gamma && dout && dy && dgamma && dbeta && workspace && rows > 0 && dtype_ok(dtype));
    CPX_REQUIRE(ln_c_ok(C));                                           // 4 or 16 channels per lane: LayerNorm2d of the neck, LayerNorm of a block
    CPX_REQUIRE(eps >= 0.f && workspace_bytes >= cpx_layernorm_backward_bytes(rows, C) && ((uintptr_t)workspace & 7) == 0);
    CPX_REQUIRE((((uintptr_t)y | (uintptr_t)gamma | (uintptr_t)dout | (uintptr_t)dy) & 15) == 0);
    hipStream_t s = (hipStream_t)stream;
    const int nblk = ln_nblk(rows);
    double *part = (double *)workspace;
    const dim3 grid(nblk), block(256);
    if (C == NECK_C) CPX_DT_DISPATCH(dtype, DT, hipLaunchKernelGGL((k_ln_bwd<DT, NECK_C>), grid, block, 0, s, y, gamma, dout, rows, (double)eps, dy, part));
    else CPX_DT_DISPATCH(dtype, DT, hipLaunchKernelGGL((k_ln_bwd<DT, NECK_K0>), grid, block, 0, s, y, gamma, dout, rows, (double)eps, dy, part));
    CPX_CHECK_LAUNCH();
    hipLaunchKernelGGL(k_ln_bwd_finish, dim3(2 * C / 512), dim3(512), 0, s, part, nblk, C, dgamma, dbeta);
    CPX_CHECK_LAUNCH();
    return CPX_OK;
}

// ---------------------------------------------------------------------------
// the backward pass
// ---------------------------------------------------------------------------
// grads (float32 elements): W0 [256][1024] | gamma1 [256] | beta1 [256] | W2 [256][2304] | gamma2 [256] | beta2 [256]
extern "C" long long cpx_neck_grad_layout(long long *off) {
    const long long n[6] = {(long long)NECK_C * NECK_K0, NECK_C, NECK_C, (long long)NECK_C * NECK_K2, NECK_C, NECK_C};
    long long o = 0;
    for (int i = 0; i < 6; ++i) { if (off) off[i] = o; o += n[i]; }
    return o;
}

// workspace: [dfeat][dy2][da1][dy0], each [rows][256] float32, then the transposed operand, the LayerNorm partials, a bias-gradient
// sink (the convolutions have no bias) and the weight-gradient partials | dCol
struct NeckBwdLayout { size_t off[4], off_wt, off_ln, off_db, off_big, total; };
static NeckBwdLayout neck_bwd_layout(int nS, int ld_head) {
    NeckBwdLayout L; CpxArena a; const size_t rows = (size_t)nS * 1024;
    for (int i = 0; i < 4; ++i) L.off[i] = a.take(rows * NECK_C * sizeof(float));
    L.off_wt = a.take((size_t)std::max(ld_head, NECK_K2) * NECK_C * sizeof(float));
    L.off_ln = a.take(cpx_layernorm_backward_workspace_bytes((int)rows, NECK_C));
    L.off_db = a.take(NECK_C * sizeof(float));
    L.off_big = a.take(std::max(std::max(cpx_uwgrad_workspace_bytes(rows, NECK_C, NECK_K2), cpx_uwgrad_workspace_bytes(rows, NECK_C, NECK_K0)),
                              rows * NECK_K2 * sizeof(float)));
    L.total = a.o;
    return L;
}
extern "C" size_t cpx_neck_backward_workspace_bytes(int nS, int dtype, int ld_head, size_t *off) {
    if (nS <= 0 || !dtype_ok(dtype) || ld_head <= 0 || ld_head % 128 || (size_t)nS * 1024 >= 0x7fffffffull) return 0;
    const NeckBwdLayout L = neck_bwd_layout(nS, ld_head);
    if (off) for (int i = 0; i < 4; ++i) off[i] = L.off[i];
    return L.total;
}

extern "C" int cpx_neck_backward(const cpx_net_weights *w, const void *x, int nS, const void *fwd_workspace, size_t fwd_workspace_bytes,
                                 const float *dhead, float *grads, void *workspace, size_t workspace_bytes, void *stream) {
    CPX_REQUIRE(neck_weights_ok(w) && x && fwd_workspace && dhead && grads && workspace && nS > 0 && (size_t)nS * 1024 < 0x7fffffffull);
    const int dt = w->dtype, rows = nS * 1024, ldh = w->ld_head;
    const NeckFwdLayout F = neck_fwd_layout(nS, dt);
    const NeckBwdLayout L = neck_bwd_layout(nS, ldh);
    CPX_REQUIRE(fwd_workspace_bytes >= F.total && workspace_bytes >= L.total);
    CPX_REQUIRE(((uintptr_t)workspace & 255) == 0 && ((uintptr_t)fwd_workspace & 255) == 0 && (((uintptr_t)dhead | (uintptr_t)grads) & 15) == 0);
    hipStream_t s = (hipStream_t)stream;
    const char *fws = (const char *)fwd_workspace;
    const void *y0 = fws + F.off[0], *a1 = fws + F.off[1], *y2 = fws + F.off[2];
    char *ws = (char *)workspace;
    float *dfeat = (float *)(ws + L.off[0]), *dy2 = (float *)(ws + L.off[1]), *da1 = (float *)(ws + L.off[2]), *dy0 = (float *)(ws + L.off[3]);
    float *wt = (float *)(ws + L.off_wt), *db_sink = (float *)(ws + L.off_db), *big = (float *)(ws + L.off_big);
    void *ln_ws = ws + L.off_ln;
    const size_t ln_bytes = L.off_db - L.off_ln;
    long long go[6];
    cpx_neck_grad_layout(go);
    // 1. dfeat = dhead Wh: the rounded head operand [ld_head][256] widened and transposed once, then the float32 GEMM
    CPX_RUN(cpx_wt_run(dt, w->head_w, ldh, NECK_C, NECK_C, wt, s));
    CPX_RUN(cpx_gemm_f32(dhead, wt, rows, NECK_C, ldh, CPX_EPI_F32, nullptr, nullptr, dfeat, NECK_C, stream));
    // 2. LayerNorm 2
    CPX_RUN(cpx_layernorm_backward(dt, y2, w->neck_ln2_w, dfeat, rows, NECK_C, 1e-6f, dy2, grads + go[4], grads + go[5], ln_ws, ln_bytes, stream));
    // 3. the 3x3 conv: dW2 [256][2304] = dy2^T im2col(a1), da1 = col2im(dy2 W2)
    UwArgs u;
    u.dy = dy2; u.xa = a1; u.lda = NECK_C; u.ca = NECK_C; u.xb = nullptr; u.ldb = 0; u.cb = 0; u.lh = 5; u.lw = 5;
    u.rows = rows; u.Npad = NECK_C; u.Kpad = NECK_K2; u.k_valid = NECK_K2;
    u.part_w = big; u.part_b = (double *)((char *)big + cpx_uwgrad_part_w_bytes(rows, NECK_C, NECK_K2));
    CPX_RUN(cpx_uwgrad_run(dt, 0, u, NECK_C, 1, NECK_C, grads + go[3], db_sink, s));
    CPX_RUN(cpx_wt_run(dt, w->neck2_w, NECK_C, NECK_K2, NECK_K2, wt, s));
    CPX_RUN(cpx_gemm_f32(dy2, wt, rows, NECK_K2, NECK_C, CPX_EPI_F32, nullptr, nullptr, big, NECK_K2, stream));
    CPX_HIP(hipMemsetAsync(da1, 0, (size_t)rows * NECK_C * sizeof(float), s));
    DxArgs g;
    g.dcol = big; g.ldc = NECK_K2; g.kind = 0; g.ctot = NECK_C; g.coff = 0; g.C = NECK_C; g.lh = 5; g.lw = 5; g.rows_src = (size_t)rows;
    g.gx = da1; g.ld_gx = NECK_C; g.y = nullptr; g.ld_y = 0; g.mask = 0;
    CPX_RUN(cpx_dx_gather_run(dt, g, s));
    // 4. LayerNorm 1
    CPX_RUN(cpx_layernorm_backward(dt, y0, w->neck_ln1_w, da1, rows, NECK_C, 1e-6f, dy0, grads + go[1], grads + go[2], ln_ws, ln_bytes, stream));
    // 5. the 1x1 conv: dW0 [256][1024] = dy0^T x
    u.dy = dy0; u.xa = x; u.lda = NECK_K0; u.ca = NECK_K0; u.Kpad = NECK_K0; u.k_valid = NECK_K0;
    u.part_b = (double *)((char *)big + cpx_uwgrad_part_w_bytes(rows, NECK_C, NECK_K0));
    CPX_RUN(cpx_uwgrad_run(dt, 2, u, NECK_C, 1, NECK_C, grads + go[0], db_sink, s));
    return CPX_OK;
}
