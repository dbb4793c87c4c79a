// Backward pass of the UNet semantic head (classpose/unet.py:121-196) with the backbone and the neck frozen (gfx950).
// What autograd does in the reference for `--feature_transformation_structure` heads (train.py:482-493 down to
// unet.py:175-196), on the op list of cpx_conv_op that cpx_unet_head_forward runs.  The forward leaves every op's output
// in its workspace in the network dtype: those are the saved activations.  Everything here is float32:
//   * k_uwgrad / k_uwgrad_reduce   dW [Npad][Kpad] = dY^T im2col(X), db = column sums of dY (a transposed conv's four per-tap bias copies
//                                  each get the sum over the taps: they are one parameter).  The exact-f32 matrix
//                                  instruction v_mfma_f32_32x32x2_f32 reduces over two ROWS per issue; the im2col operand is
//                                  gathered straight from the stored tensors (3x3 pad-1 taps over a|b, 2x2 stride-2
//                                  space-to-depth, plain), never materialised.  Row slabs of UW_SLAB; the per-slab partials
//                                  are added in slab order in float64 and rounded once.
//   * k_wt                         the op's rounded operand [Npad][Kpad] widened and transposed to float32 [Kpad128][Npad]
//   * cpx_gemm_f32                 dCol [rows][Kpad128] = dY W   (the data gradient in im2col space)
//   * k_dx_gather                  col2im: the taps of dCol that touch an input element are added in tap order, the a|b
//                                  concat is split, a second consumer's contribution is added to the first's, and the LAST
//                                  contribution applies the producer's ReLU mask (stored output > 0)
//   * k_s2d                        space-to-depth of the gradient of a transposed conv's output (dY for both products)
// Rounding to the network dtype is treated as the identity (straight-through).  No gradient for tensor 0 (the neck output).
// Determinism: no atomics; every sum has a fixed order, so a backward pass is a function of its inputs only, bitwise.
// Padding: gradient tensors are zeroed first and only valid channels are ever written; padded weight rows / columns meet
// exact zeros in dY or X, so their gradients are exact zeros.
#include "cpx_internal.h"
#include <algorithm>

#define UNET_MAX_OPS 64

static inline int ilog2(int x) { int l = 0; while ((1 << l) < x) ++l; return l; }
static inline bool is_pow2(int x) { return x > 0 && (x & (x - 1)) == 0; }

// ---------------------------------------------------------------------------
// weight gradient
// ---------------------------------------------------------------------------

// One wave = one (32 columns of dY) x (64 columns of im2col(X)) tile of one slab; lane (r, h2) feeds dY[row + h2][n0 + r] and
// im2col(X)[row + h2][k0 + r], [k0 + 32 + r]: its tap and channel are fixed, only the row moves.
template <int DT, int KIND>
__global__ void __launch_bounds__(256) k_uwgrad(UwArgs g) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, r = lane & 31, h2 = lane >> 5;
    const int n0 = blockIdx.x * 32, k0 = (blockIdx.y * 4 + wave) * 64, slab = blockIdx.z;
    if (k0 >= g.Kpad) return;                                          // (the whole wave: k0 is wave-uniform)
    const int row0 = slab * UW_SLAB, row1 = min(g.rows, row0 + UW_SLAB);
    const int ctot = g.ca + g.cb;
    // the lane's two im2col columns
    const void *src[2]; int ld[2], ch[2], dy_[2], dx_[2]; bool kv[2];
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const int k = k0 + 32 * j + r;
        kv[j] = k < g.k_valid;
        const int tap = kv[j] ? k / ctot : 0, c = kv[j] ? k - tap * ctot : 0;
        const bool in_a = c < g.ca;
        src[j] = in_a ? g.xa : g.xb; ld[j] = in_a ? g.lda : g.ldb; ch[j] = in_a ? c : c - g.ca;
        if (KIND == 0) { dy_[j] = tap / 3 - 1; dx_[j] = tap % 3 - 1; }
        else if (KIND == 1) { dy_[j] = tap >> 1; dx_[j] = tap & 1; }
        else { dy_[j] = 0; dx_[j] = 0; }
    }
    const int lwo = KIND == 1 ? g.lw - 1 : g.lw, lho = KIND == 1 ? g.lh - 1 : g.lh;      // rows run over the conv's OUTPUT grid (kind 2: its input grid)
    const int H = 1 << g.lh, W = 1 << g.lw;
    f32x16 acc0, acc1;
#pragma unroll
    for (int v = 0; v < 16; ++v) { acc0[v] = 0.f; acc1[v] = 0.f; }
    double bsum = 0;
    const int trips = (row1 - row0 + 1) >> 1;                          // (uniform over the workgroup: the MFMA needs every lane)
    for (int i = 0; i < trips; ++i) {
        const int row = row0 + 2 * i + h2;
        const bool in = row < row1;
        const float a = in ? g.dy[(size_t)row * g.Npad + n0 + r] : 0.f;
        float b[2];
        const int s = row >> (lho + lwo), y = (row >> lwo) & ((1 << lho) - 1), x = row & ((1 << lwo) - 1);
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            int yy, xx;
            if (KIND == 0) { yy = y + dy_[j]; xx = x + dx_[j]; }
            else if (KIND == 1) { yy = 2 * y + dy_[j]; xx = 2 * x + dx_[j]; }
            else { yy = y; xx = x; }
            const bool ok = in && kv[j] && (unsigned)yy < (unsigned)H && (unsigned)xx < (unsigned)W;
            const size_t srow = ((size_t)s << (g.lh + g.lw)) + ((size_t)yy << g.lw) + xx;
            b[j] = ok ? load_f32<DT>(src[j], srow * ld[j] + ch[j]) : 0.f;
        }
        acc0 = MFMA_F32(a, b[0], acc0);
        acc1 = MFMA_F32(a, b[1], acc1);
        bsum += (double)a;
    }
    // accumulator register v of lane (r, h2): dY column n0 + (v&3) + 8*(v>>2) + 4*h2, im2col column k0 + r
    float *pw = g.part_w + ((size_t)slab * g.Npad + n0) * g.Kpad + k0 + r;
#pragma unroll
    for (int v = 0; v < 16; ++v) {
        const int n = (v & 3) + 8 * (v >> 2) + 4 * h2;
        pw[(size_t)n * g.Kpad] = acc0[v];
        pw[(size_t)n * g.Kpad + 32] = acc1[v];
    }
    if (k0 == 0) {
        bsum += __shfl_xor(bsum, 32, 64);                              // even rows + odd rows
        if (h2 == 0) g.part_b[(size_t)slab * g.Npad + n0 + r] = bsum;
    }
}

// bias_taps = 4 (transposed conv): the packed bias holds one copy of the conv's bias per tap, rows tap * cout + co.  The four copies
// are ONE parameter: each receives the sum over the taps (slab by slab, tap by tap), so they stay equal under the optimiser.
__global__ void __launch_bounds__(256) k_uwgrad_reduce(const float *__restrict__ part_w, const double *__restrict__ part_b,
                                                       int n_slabs, size_t nw, int N, int n_done, int bias_taps, int cout,
                                                       float *__restrict__ dW, float *__restrict__ db) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    const size_t w_done = nw / N * n_done;                             // rows n_done.. of the partials were never computed: all padding
    if (i < nw) {
        double s = 0;
        if (i < w_done)
            for (int k = 0; k < n_slabs; ++k) s += (double)part_w[(size_t)k * nw + i];
        dW[i] = (float)s;
    }
    if (i < (size_t)N) {
        double s = 0;
        if (i >= (size_t)n_done) {
        } else if (bias_taps > 1 && i < (size_t)bias_taps * cout) {
            const int co = (int)(i % cout);
            for (int k = 0; k < n_slabs; ++k)
                for (int t = 0; t < bias_taps; ++t) s += part_b[(size_t)k * N + t * cout + co];
        } else {
            for (int k = 0; k < n_slabs; ++k) s += part_b[(size_t)k * N + i];
        }
        db[i] = (float)s;
    }
}

// ---------------------------------------------------------------------------
// data gradient
// ---------------------------------------------------------------------------
// W [Npad][Kpad] in the network dtype -> float32 [Kp128][Npad], rows Kpad.. zero
template <int DT>
__global__ void __launch_bounds__(256) k_wt(const void *__restrict__ w, int Npad, int Kpad, int Kp128, float *__restrict__ wt) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (size_t)Kp128 * Npad) return;
    const int k = (int)(i / Npad), n = (int)(i - (size_t)k * Npad);
    wt[i] = k < Kpad ? load_f32<DT>(w, (size_t)n * Kpad + k) : 0.f;
}

// gradient of a transposed conv's output [4 rows][ld_g] -> [rows][Npad], column tap * cout + co; zero from 4 cout on
__global__ void __launch_bounds__(256) k_s2d(const float *__restrict__ gy, int ld_g, int cout, int lh, int lw, size_t rows, int Npad,
                                             float *__restrict__ out) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= rows * Npad) return;
    const size_t row = i / Npad;
    const int n = (int)(i - row * Npad);
    float v = 0.f;
    if (n < 4 * cout) {
        const int tap = n / cout, co = n - tap * cout;
        const size_t s = row >> (lh + lw);
        const int y = (int)(row >> lw) & ((1 << lh) - 1), x = (int)row & ((1 << lw) - 1);
        const size_t orow = (s << (lh + lw + 2)) + ((size_t)(2 * y + (tap >> 1)) << (lw + 1)) + 2 * x + (tap & 1);
        v = gy[orow * ld_g + co];
    }
    out[i] = v;
}

template <int DT>
__global__ void __launch_bounds__(256) k_dx_gather(DxArgs g) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= g.rows_src * g.C) return;
    const size_t row = i / g.C;
    const int c = (int)(i - row * g.C);
    const size_t s = row >> (g.lh + g.lw);
    const int y = (int)(row >> g.lw) & ((1 << g.lh) - 1), x = (int)row & ((1 << g.lw) - 1);
    const int H = 1 << g.lh, W = 1 << g.lw;
    float v = 0.f;
    if (g.kind == 0) {
        for (int tap = 0; tap < 9; ++tap) {                           // output pixel (y - (ty - 1), x - (tx - 1)) read this one through tap (ty, tx)
            const int oy = y - (tap / 3 - 1), ox = x - (tap % 3 - 1);
            if ((unsigned)oy < (unsigned)H && (unsigned)ox < (unsigned)W) {
                const size_t orow = (s << (g.lh + g.lw)) + ((size_t)oy << g.lw) + ox;
                v += g.dcol[orow * g.ldc + tap * g.ctot + g.coff + c];
            }
        }
    } else if (g.kind == 1) {
        const int tap = (y & 1) * 2 + (x & 1);
        const size_t orow = (s << (g.lh + g.lw - 2)) + ((size_t)(y >> 1) << (g.lw - 1)) + (x >> 1);
        v = g.dcol[orow * g.ldc + tap * g.ctot + g.coff + c];
    } else {
        v = g.dcol[row * g.ldc + g.coff + c];
    }
    float *d = g.gx + row * g.ld_gx + c;
    v = *d + v;
    if (g.mask && !(load_f32<DT>(g.y, row * g.ld_y + c) > 0.f)) v = 0.f;
    *d = v;
}

// ---------------------------------------------------------------------------
// launchers (cpx_internal.h): this pass and the neck's backward (cpx_train_neck.hip) run the same kernels
// ---------------------------------------------------------------------------
size_t cpx_uwgrad_part_w_bytes(size_t rows, int Npad, int Kpad) {
    const size_t n_slabs = (rows + UW_SLAB - 1) / UW_SLAB;
    return cpx_align_up(n_slabs * Npad * Kpad * sizeof(float), 256);
}
size_t cpx_uwgrad_workspace_bytes(size_t rows, int Npad, int Kpad) {
    const size_t n_slabs = (rows + UW_SLAB - 1) / UW_SLAB;
    return cpx_uwgrad_part_w_bytes(rows, Npad, Kpad) + cpx_align_up(n_slabs * Npad * sizeof(double), 256);
}
int cpx_uwgrad_run(int dtype, int kind, const UwArgs &u, int n_valid, int bias_taps, int cout, float *dW, float *db, hipStream_t s) {
    const int n_slabs = (u.rows + UW_SLAB - 1) / UW_SLAB;
    CPX_REQUIRE(n_slabs <= 65535 && kind >= 0 && kind <= 2);
    const int n_done = (n_valid + 31) / 32 * 32;                                  // (<= Npad)
    const dim3 grid(n_done / 32, (u.Kpad / 64 + 3) / 4, n_slabs), block(256);
    CPX_DT_DISPATCH(dtype, DT,
                    if (kind == 0) hipLaunchKernelGGL((k_uwgrad<DT, 0>), grid, block, 0, s, u);
                    else if (kind == 1) hipLaunchKernelGGL((k_uwgrad<DT, 1>), grid, block, 0, s, u);
                    else hipLaunchKernelGGL((k_uwgrad<DT, 2>), grid, block, 0, s, u));
    const size_t nw = (size_t)u.Npad * u.Kpad;
    hipLaunchKernelGGL(k_uwgrad_reduce, dim3((unsigned)((nw + 255) / 256)), block, 0, s, u.part_w, u.part_b, n_slabs, nw, u.Npad, n_done,
                       bias_taps, cout, dW, db);
    CPX_CHECK_LAUNCH();
    return CPX_OK;
}
int cpx_wt_run(int dtype, const void *w, int Npad, int Kpad, int Kp128, float *wt, hipStream_t s) {
    const size_t nt = (size_t)Kp128 * Npad;
    const dim3 grid((unsigned)((nt + 255) / 256)), block(256);
    CPX_DT_DISPATCH(dtype, DT, hipLaunchKernelGGL(k_wt<DT>, grid, block, 0, s, w, Npad, Kpad, Kp128, wt));
    CPX_CHECK_LAUNCH();
    return CPX_OK;
}
int cpx_dx_gather_run(int dtype, const DxArgs &g, hipStream_t s) {
    const size_t n = g.rows_src * g.C;
    const dim3 grid((unsigned)((n + 255) / 256)), block(256);
    CPX_DT_DISPATCH(dtype, DT, hipLaunchKernelGGL(k_dx_gather<DT>, grid, block, 0, s, g));
    CPX_CHECK_LAUNCH();
    return CPX_OK;
}

// ---------------------------------------------------------------------------
// layouts
// ---------------------------------------------------------------------------
// workspace: [gradient tensor [rows_out_pad][ld] float32 of every op but the last][space-to-depth staging]
//            [transposed operand][weight-gradient partials | dCol]
struct BwdLayout { size_t g_off[UNET_MAX_OPS]; int g_ld[UNET_MAX_OPS]; size_t g_bytes, s2d_off, wt_off, big_off, total; };
static size_t uw_part_w_bytes(const OpDims &d) { return cpx_uwgrad_part_w_bytes(d.rows, d.Npad, d.Kpad); }
static void bwd_layout(const cpx_conv_op *ops, int n_ops, int nS, BwdLayout &L) {
    CpxArena a; size_t s2d = 0, wt = 0, big = 0;
    for (int i = 0; i < n_ops; ++i) {
        const OpDims d = op_dims(ops[i], nS);
        L.g_off[i] = a.o; L.g_ld[i] = d.ld;
        if (i < n_ops - 1) a.take((size_t)d.rows_out_pad * d.ld * sizeof(float));
        if (ops[i].kind == 2) s2d = std::max(s2d, (size_t)d.rows_pad * d.Npad * sizeof(float));
        wt = std::max(wt, (size_t)d.Kp128 * d.Npad * sizeof(float));
        big = std::max(big, std::max(cpx_uwgrad_workspace_bytes(d.rows, d.Npad, d.Kpad), (size_t)d.rows_pad * d.Kp128 * sizeof(float)));
    }
    L.g_bytes = a.o;
    L.s2d_off = a.take(s2d);
    L.wt_off = a.take(wt);
    L.big_off = a.take(big);
    L.total = a.o;
}
static bool ops_ok(const cpx_conv_op *ops, int n_ops, int nS) {
    if (!ops || n_ops <= 0 || n_ops > UNET_MAX_OPS || nS <= 0 || ops[n_ops - 1].kind != 2) return false;
    for (int i = 0; i < n_ops; ++i) {
        const cpx_conv_op &o = ops[i];
        if (o.kind < 0 || o.kind > 2 || !is_pow2(o.h) || !is_pow2(o.w) || (o.kind == 1 && (o.h < 2 || o.w < 2))) return false;
        if (o.cin_a <= 0 || o.cin_b < 0 || o.cout <= 0 || o.cin_a % 8 || o.cin_b % 8 || o.cout % 8) return false;
        if (o.dst != i + 1 || o.src_a < 0 || o.src_a > i || o.src_b > i || (o.kind == 2 && o.src_b >= 0)) return false;
        if ((size_t)nS * o.h * o.w * 4 >= 0x7fffffffull) return false;
    }
    return true;
}

extern "C" int cpx_unet_wgrad_slab_rows(void) { return UW_SLAB; }
extern "C" size_t cpx_unet_backward_workspace_bytes(const cpx_conv_op *ops, int n_ops, int nS, int dtype) {
    if (!ops_ok(ops, n_ops, nS) || !dtype_ok(dtype)) return 0;
    BwdLayout L;
    bwd_layout(ops, n_ops, nS, L);
    return L.total;
}
// element offsets of every op's packed operand [Npad][Kpad] and bias [Npad] in the flat parameter / gradient buffers
static long long param_layout(const cpx_conv_op *ops, int n_ops, long long *w_off, long long *b_off, int *n_pad, int *k_pad) {
    long long off = 0;
    for (int i = 0; i < n_ops; ++i) {
        const OpDims d = op_dims(ops[i], 1);
        if (w_off) w_off[i] = off;
        off += (long long)d.Npad * d.Kpad;
        if (b_off) b_off[i] = off;
        off += d.Npad;
        if (n_pad) n_pad[i] = d.Npad;
        if (k_pad) k_pad[i] = d.Kpad;
    }
    return off;
}
extern "C" long long cpx_unet_param_layout(const cpx_conv_op *ops, int n_ops, long long *w_off, long long *b_off, int *n_pad, int *k_pad) {
    if (!ops || n_ops <= 0 || n_ops > UNET_MAX_OPS) return 0;
    return param_layout(ops, n_ops, w_off, b_off, n_pad, k_pad);
}
extern "C" int cpx_unet_grad_layout(const cpx_conv_op *ops, int n_ops, int nS, int dtype, size_t *g_off, int *g_ld) {
    CPX_REQUIRE(ops_ok(ops, n_ops, nS) && g_off && g_ld);
    BwdLayout L;
    bwd_layout(ops, n_ops, nS, L);
    for (int i = 0; i < n_ops; ++i) { g_off[i] = L.g_off[i]; g_ld[i] = L.g_ld[i]; }
    return CPX_OK;
}

extern "C" int cpx_unet_refresh_operands(const cpx_conv_op *ops, int n_ops, const float *params, int dtype, void *stream) {
    CPX_REQUIRE(ops && n_ops > 0 && n_ops <= UNET_MAX_OPS && params && ((uintptr_t)params & 15) == 0);
    CPX_REQUIRE(dtype_ok(dtype));
    long long w_off[UNET_MAX_OPS], b_off[UNET_MAX_OPS]; int n_pad[UNET_MAX_OPS], k_pad[UNET_MAX_OPS];
    param_layout(ops, n_ops, w_off, b_off, n_pad, k_pad);
    for (int i = 0; i < n_ops; ++i) {
        CPX_REQUIRE(ops[i].weight && ops[i].bias);
        CPX_RUN(cpx_round_weights(params + w_off[i], const_cast<void *>(ops[i].weight), (long long)n_pad[i] * k_pad[i], dtype, dtype == CPX_DT_F32, stream));
        CPX_RUN(cpx_round_weights(params + b_off[i], const_cast<float *>(ops[i].bias), n_pad[i], dtype, 1, stream));
    }
    return CPX_OK;
}

// ---------------------------------------------------------------------------
// the pass
// ---------------------------------------------------------------------------
template <int DT>
static int unet_backward(const cpx_conv_op *ops, int n_ops, const void *feat, int nS, const char *fws, const float *dlogits,
                         float *grads, char *ws, hipStream_t s) {
    BwdLayout L;
    bwd_layout(ops, n_ops, nS, L);
    size_t a_off[UNET_MAX_OPS]; int a_ld[UNET_MAX_OPS];
    cpx_unet_act_layout(DT, ops, n_ops, nS, a_off, a_ld);
    long long w_off[UNET_MAX_OPS], b_off[UNET_MAX_OPS];
    param_layout(ops, n_ops, w_off, b_off, nullptr, nullptr);
    // tensor id t > 0 is op t - 1's output; its last contribution comes from its consumer with the smallest index
    int last_consumer[UNET_MAX_OPS + 1];
    for (int t = 0; t <= n_ops; ++t) last_consumer[t] = -1;
    for (int i = n_ops - 1; i >= 0; --i) { last_consumer[ops[i].src_a] = i; if (ops[i].src_b >= 0) last_consumer[ops[i].src_b] = i; }
    for (int t = 1; t < n_ops; ++t) CPX_REQUIRE(last_consumer[t] >= 0);          // every tensor but the head is read by somebody
    auto tensor = [&](int id) -> CpxTensor {
        if (id == 0) return {(const char *)feat, 256, 256, 32, 32};
        const cpx_conv_op &p = ops[id - 1];
        const OpDims d = op_dims(p, nS);
        return {fws + a_off[id - 1], a_ld[id - 1], p.cout, d.ho, d.wo};
    };
    CPX_HIP(hipMemsetAsync(ws, 0, L.g_bytes, s));
    float *stage = (float *)(ws + L.s2d_off), *wt = (float *)(ws + L.wt_off), *big = (float *)(ws + L.big_off);
    for (int i = n_ops - 1; i >= 0; --i) {
        const cpx_conv_op &o = ops[i];
        const OpDims d = op_dims(o, nS);
        const CpxTensor A = tensor(o.src_a), Bz = {nullptr, 0, 0, 0, 0}, B = o.src_b >= 0 ? tensor(o.src_b) : Bz;
        CPX_REQUIRE(A.c == o.cin_a && A.h == o.h && A.w == o.w && (o.src_b < 0 || (B.c == o.cin_b && B.h == o.h && B.w == o.w)));
        CPX_REQUIRE(o.weight && d.rows < 0x7fffffffull);
        const int lh = ilog2(o.h), lw = ilog2(o.w);
        const float *gy = i == n_ops - 1 ? dlogits : (const float *)(ws + L.g_off[i]);
        const int ld_gy = i == n_ops - 1 ? o.cout : L.g_ld[i];
        const float *dy = gy;
        if (o.kind == 2) {
            const size_t n = d.rows * d.Npad;
            hipLaunchKernelGGL(k_s2d, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, gy, ld_gy, o.cout, lh, lw, d.rows, d.Npad, stage);
            dy = stage;
        } else CPX_REQUIRE(ld_gy == d.Npad);
        // weight gradient
        UwArgs u;
        u.dy = dy; u.xa = A.p; u.lda = A.ld; u.ca = o.cin_a; u.xb = B.p; u.ldb = B.ld; u.cb = o.cin_b; u.lh = lh; u.lw = lw;
        u.rows = (int)d.rows; u.Npad = d.Npad; u.Kpad = d.Kpad; u.k_valid = d.taps * d.ctot;
        u.part_w = big; u.part_b = (double *)((char *)big + uw_part_w_bytes(d));
        CPX_RUN(cpx_uwgrad_run(DT, o.kind, u, o.kind == 2 ? 4 * o.cout : o.cout, o.kind == 2 ? 4 : 1, o.cout, grads + w_off[i], grads + b_off[i], s));
        // data gradient (none for the frozen neck output)
        if (o.src_a == 0 && o.src_b <= 0) continue;
        CPX_RUN(cpx_wt_run(DT, o.weight, d.Npad, d.Kpad, d.Kp128, wt, s));
        CPX_RUN(cpx_gemm_f32(dy, wt, d.rows_pad, d.Kp128, d.Npad, CPX_EPI_F32, nullptr, nullptr, big, d.Kp128, s));
        for (int side = 0; side < 2; ++side) {
            const int id = side == 0 ? o.src_a : o.src_b;
            if (id <= 0) continue;
            const CpxTensor X = side == 0 ? A : B;
            DxArgs g;
            g.dcol = big; g.ldc = d.Kp128; g.kind = o.kind; g.ctot = d.ctot; g.coff = side == 0 ? 0 : o.cin_a; g.C = X.c;
            g.lh = lh; g.lw = lw; g.rows_src = (size_t)nS * o.h * o.w;
            g.gx = (float *)(ws + L.g_off[id - 1]); g.ld_gx = L.g_ld[id - 1];
            g.y = X.p; g.ld_y = X.ld; g.mask = ops[id - 1].relu && last_consumer[id] == i;
            CPX_RUN(cpx_dx_gather_run(DT, g, s));
        }
    }
    return CPX_OK;
}

extern "C" int cpx_unet_head_backward(const cpx_conv_op *ops, int n_ops, const void *feat, int nS, int dtype,
                                      const void *fwd_workspace, size_t fwd_workspace_bytes, const float *dlogits, float *grads,
                                      void *workspace, size_t workspace_bytes, void *stream) {
    CPX_REQUIRE(ops_ok(ops, n_ops, nS) && feat && fwd_workspace && dlogits && grads && workspace);
    CPX_REQUIRE(dtype_ok(dtype));
    CPX_REQUIRE(ops[n_ops - 1].h == 16 && ops[n_ops - 1].w == 16);                 // the last op writes the 32 x 32 token grid
    CPX_REQUIRE(fwd_workspace_bytes >= cpx_unet_ws_bytes(dtype, ops, n_ops, nS));
    CPX_REQUIRE(workspace_bytes >= cpx_unet_backward_workspace_bytes(ops, n_ops, nS, dtype) && ((uintptr_t)workspace & 255) == 0);
    hipStream_t s = (hipStream_t)stream;
    CPX_DT_DISPATCH(dtype, DT, return unet_backward<DT>(ops, n_ops, feat, nS, (const char *)fwd_workspace, dlogits, grads, (char *)workspace, s));
}
