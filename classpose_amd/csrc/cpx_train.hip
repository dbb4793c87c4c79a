// Training of the 1x1 semantic class head with the backbone frozen (gfx950).
// Replaces, for `--freeze backbone segmentation_head neck`, what classpose/train.py does per step on the
// host framework: `_loss_fn_class` (train.py:156-181), `_loss_fn_tversky` (train.py:108-153), their sum through
// `LossAggregator(optimise=False)` (train.py:482-493), autograd down to `out_class` (vit_sam.py:199-249) and
// `torch.optim.AdamW` (train.py:478-480).  The forward is cpx_net_forward; this file adds
//   * k_patchify_f32     float32 NCHW crops -> patch rows in the network dtype
//   * k_loss_sums / k_loss_finish / k_loss_grad    the two losses and d loss / d logits on the token-major head buffer
//   * k_seg_loss / k_seg_finish                   the flow head's loss (cellpose _loss_fn_seg) and its gradient, columns 0..191
//   * k_wgrad / k_wgrad_reduce                    dW = dlogits^T feat, db = column sums (exact-f32 MFMA, row slabs)
//   * k_adamw                                     the parameter update on float32 master weights
// Determinism: no floating-point atomics anywhere.  Every sum is a fixed tree inside a wave (xor butterfly), a fixed serial
// order across the tokens of a wave, the waves of a workgroup, the workgroups of an image and the images -- the result of a
// step is a function of its inputs only, bitwise.
#include "cpx_internal.h"

#define LOSS_TOK_PER_BLOCK 64      // tokens (8 x 8 pixel patches) per workgroup of the loss passes: 4 waves x 16 tokens
#define LOSS_MAX_CLS 64            // general kernels: lane c of a wave carries class c's sums
#define LOSS_REG_CLS 16            // up to here the per-class values of a lane live in registers (k_loss_*_reg)
#define WG_FEAT 256                // feature channels of the neck

// ---------------------------------------------------------------------------
// patchify
// ---------------------------------------------------------------------------
template <int DT>
__global__ void __launch_bounds__(256) k_patchify_f32(const float *__restrict__ x, int H, int W, size_t n_items, void *__restrict__ out) {
    // one item = 8 consecutive j of one (token row, c, i): 32 contiguous bytes in, 16 / 32 contiguous bytes out
    const size_t it = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (it >= n_items) return;
    const int th = H >> 3, tw = W >> 3;
    const int ci = (int)(it % 24), c = ci >> 3, i = ci & 7;
    const size_t row = it / 24;
    const size_t s = row / ((size_t)th * tw);
    const int t = (int)(row - s * th * tw), ph = t / tw, pw = t - ph * tw;
    const float *src = x + ((s * 3 + c) * H + (size_t)(8 * ph + i)) * W + 8 * pw;
    const float4 a = *reinterpret_cast<const float4 *>(src), b = *reinterpret_cast<const float4 *>(src + 4);
    const float v[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
    const size_t o = row * 192 + (size_t)c * 64 + i * 8;
    if constexpr (DT == CPX_DT_F32) {
        float *d = (float *)out + o;
        *reinterpret_cast<float4 *>(d) = a;
        *reinterpret_cast<float4 *>(d + 4) = b;
    } else {
        unsigned u[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            unsigned short lo, hi;
            if constexpr (DT == CPX_DT_F16) {
                _Float16 h0 = (_Float16)v[2 * k], h1 = (_Float16)v[2 * k + 1];
                lo = *reinterpret_cast<unsigned short *>(&h0); hi = *reinterpret_cast<unsigned short *>(&h1);
            } else {
                lo = f32_to_bf16(v[2 * k]); hi = f32_to_bf16(v[2 * k + 1]);
            }
            u[k] = (unsigned)lo | ((unsigned)hi << 16);
        }
        *reinterpret_cast<uint4 *>((unsigned short *)out + o) = make_uint4(u[0], u[1], u[2], u[3]);
    }
}

extern "C" int cpx_patchify_f32(const float *x, int nS, int H, int W, int dtype, void *patches, void *stream) {
    CPX_REQUIRE(x && patches && nS > 0 && H > 0 && W > 0 && H % 8 == 0 && W % 8 == 0);
    CPX_REQUIRE(dtype_ok(dtype));
    const size_t n_items = (size_t)nS * (H / 8) * (W / 8) * 24;
    CPX_REQUIRE(n_items / 256 < 0x7fffffffull);
    dim3 grid((unsigned)((n_items + 255) / 256)), block(256);
    hipStream_t s = (hipStream_t)stream;
    CPX_DT_DISPATCH(dtype, DT, hipLaunchKernelGGL(k_patchify_f32<DT>, grid, block, 0, s, x, H, W, n_items, patches));
    CPX_CHECK_LAUNCH();
    return CPX_OK;
}

// ---------------------------------------------------------------------------
// losses
// ---------------------------------------------------------------------------
// workspace: per (image, workgroup) a record of double [3 * ncls + 4]: tp, fp, fn per class, then the cross-entropy numerator
// sum w[y] * -log p[y], its denominator sum w[y], the number of annotated pixels and a flag (labels outside [0, ncls));
// then per (image, class) two floats, the factors of the Tversky gradient, and one float 1 / (sum of w[y] over the batch).
struct LossWs { size_t off_part, off_coef, off_scal, total; int nblk, rec; };
static LossWs loss_ws(int nI, int H, int W, int ncls) {
    LossWs w; const int T = (H / 8) * (W / 8);
    w.nblk = (T + LOSS_TOK_PER_BLOCK - 1) / LOSS_TOK_PER_BLOCK;
    w.rec = 3 * ncls + 4;
    w.off_part = 0;
    w.off_coef = cpx_align_up((size_t)nI * w.nblk * w.rec * sizeof(double), 256);
    w.off_scal = cpx_align_up(w.off_coef + (size_t)nI * ncls * 2 * sizeof(float), 256);
    w.total = w.off_scal + 256;
    return w;
}
extern "C" size_t cpx_class_loss_workspace_bytes(int nI, int H, int W, int ncls) {
    if (nI <= 0 || H <= 0 || W <= 0 || H % 8 || W % 8 || ncls < 2 || ncls > LOSS_MAX_CLS) return 0;
    return loss_ws(nI, H, W, ncls).total;
}

struct LossArgs {
    const float *head; int ld_head, col0;
    const int16_t *labels;
    int nI, H, W, ncls, nblk, rec;
    const float *cw;
    float alpha, gamma, eps, w_ce, w_tv;
    double *part; float *coef; float *scal;
    float *ce, *tversky, *tp, *fp, *fn; int32_t *n_annot, *status;
    float *dlogits;
};

// the lane's pixel of token t of image b: lane = 8 i + j -> pixel (8 ph + i, 8 pw + j)
__device__ __forceinline__ int lane_label(const LossArgs &g, int b, int t, int lane) {
    const int tw = g.W >> 3, ph = t / tw, pw = t - ph * tw;
    return g.labels[((size_t)b * g.H + 8 * ph + (lane >> 3)) * g.W + 8 * pw + (lane & 7)];
}
// log-sum-exp of the lane's pixel in two parts, the maximum and ls = log sum exp(z - max).  They are kept apart: the sum max + ls is
// rounded at the size of the logits (2^-18 at |z| = 80), and that rounding would be a relative error of every p = exp(z - lse) of the
// pixel, the same for all pixels with the same logits; p = exp((z - max) - ls) and -log p[y] = ls - (z[y] - max) round at their own size
__device__ __forceinline__ void lane_lse(const float *z, int ncls, float &mx, float &ls) {
    mx = z[0];
    for (int c = 1; c < ncls; ++c) mx = fmaxf(mx, z[c * 64]);
    float s = 0.f;
    for (int c = 0; c < ncls; ++c) s += expf(z[c * 64] - mx);
    ls = logf(s);
}

__global__ void __launch_bounds__(256) k_loss_sums(LossArgs g) {
    __shared__ double sm[4][3 * LOSS_MAX_CLS + 4];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, b = blockIdx.y, blk = blockIdx.x;
    const int T = (g.H >> 3) * (g.W >> 3);
    const int t_end = min(T, (blk + 1) * LOSS_TOK_PER_BLOCK);
    double a_tp = 0, a_fp = 0, a_fn = 0, ce_num = 0, ce_den = 0, cnt = 0, bad = 0;     // a_*: class `lane`'s sums
    for (int t = blk * LOSS_TOK_PER_BLOCK + wave; t < t_end; t += 4) {
        int y = lane_label(g, b, t, lane);
        const bool valid = y != -100;
        if (valid && (y < 0 || y >= g.ncls)) bad = 1;
        const bool use = valid && y >= 0 && y < g.ncls;
        const float *z = g.head + ((size_t)b * T + t) * g.ld_head + g.col0 + lane;
        float mx, ls;
        lane_lse(z, g.ncls, mx, ls);
        if (use) {
            const float wy = g.cw ? g.cw[y] : 1.f;
            ce_num += (double)wy * (double)(ls - (z[y * 64] - mx));
            ce_den += (double)wy;
            cnt += 1;
        }
        for (int c = 0; c < g.ncls; ++c) {
            const float p = expf((z[c * 64] - mx) - ls);
            const double s_tp = wave_sum(use && y == c ? (double)p : 0.0);
            const double s_fp = wave_sum(use && y != c ? (double)p : 0.0);
            const double s_fn = wave_sum(use && y == c ? (double)(1.f - p) : 0.0);
            if (lane == c) { a_tp += s_tp; a_fp += s_fp; a_fn += s_fn; }
        }
    }
    ce_num = wave_sum(ce_num); ce_den = wave_sum(ce_den); cnt = wave_sum(cnt); bad = wave_sum(bad);
    if (lane < g.ncls) { sm[wave][3 * lane] = a_tp; sm[wave][3 * lane + 1] = a_fp; sm[wave][3 * lane + 2] = a_fn; }
    if (lane == 0) { double *e = &sm[wave][3 * g.ncls]; e[0] = ce_num; e[1] = ce_den; e[2] = cnt; e[3] = bad; }
    __syncthreads();
    if ((int)threadIdx.x < g.rec) {
        const int k = threadIdx.x;
        g.part[((size_t)b * g.nblk + blk) * g.rec + k] = ((sm[0][k] + sm[1][k]) + sm[2][k]) + sm[3][k];
    }
}

// ncls <= NC (the reference's 7- and 10-class heads): a lane's logits and its per-class sums stay in registers (fully unrolled class
// loops, no indexed arrays), every logit is read once and the cross-lane sums are taken once per wave instead of once per token
template <int NC>
__global__ void __launch_bounds__(256) k_loss_sums_reg(LossArgs g) {
    __shared__ double sm[4][3 * NC + 4];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, b = blockIdx.y, blk = blockIdx.x;
    const int T = (g.H >> 3) * (g.W >> 3);
    const int t_end = min(T, (blk + 1) * LOSS_TOK_PER_BLOCK);
    double a_tp[NC], a_fp[NC], a_fn[NC], ce_num = 0, ce_den = 0, cnt = 0, bad = 0;
#pragma unroll
    for (int c = 0; c < NC; ++c) { a_tp[c] = 0; a_fp[c] = 0; a_fn[c] = 0; }
    for (int t = blk * LOSS_TOK_PER_BLOCK + wave; t < t_end; t += 4) {
        const int y = lane_label(g, b, t, lane);
        if (y != -100 && (y < 0 || y >= g.ncls)) bad = 1;
        const bool use = y >= 0 && y < g.ncls;
        const float *zp = g.head + ((size_t)b * T + t) * g.ld_head + g.col0 + lane;
        float z[NC], mx = zp[0], s = 0.f, zy = 0.f;
#pragma unroll
        for (int c = 0; c < NC; ++c) { z[c] = c < g.ncls ? zp[c * 64] : 0.f; if (c < g.ncls) mx = fmaxf(mx, z[c]); }
#pragma unroll
        for (int c = 0; c < NC; ++c) { if (c < g.ncls) s += expf(z[c] - mx); if (c == y) zy = z[c]; }
        const float ls = logf(s);
        if (use) {
            const float wy = g.cw ? g.cw[y] : 1.f;
            ce_num += (double)wy * (double)(ls - (zy - mx));
            ce_den += (double)wy;
            cnt += 1;
#pragma unroll
            for (int c = 0; c < NC; ++c) {
                if (c < g.ncls) {
                    const float p = expf((z[c] - mx) - ls);
                    if (c == y) { a_tp[c] += (double)p; a_fn[c] += (double)(1.f - p); }
                    else a_fp[c] += (double)p;
                }
            }
        }
    }
#pragma unroll
    for (int c = 0; c < NC; ++c) {
        if (c < g.ncls) {
            const double s0 = wave_sum(a_tp[c]), s1 = wave_sum(a_fp[c]), s2 = wave_sum(a_fn[c]);
            if (lane == 0) { sm[wave][3 * c] = s0; sm[wave][3 * c + 1] = s1; sm[wave][3 * c + 2] = s2; }
        }
    }
    ce_num = wave_sum(ce_num); ce_den = wave_sum(ce_den); cnt = wave_sum(cnt); bad = wave_sum(bad);
    if (lane == 0) { double *e = &sm[wave][3 * g.ncls]; e[0] = ce_num; e[1] = ce_den; e[2] = cnt; e[3] = bad; }
    __syncthreads();
    if ((int)threadIdx.x < g.rec) {
        const int k = threadIdx.x;
        g.part[((size_t)b * g.nblk + blk) * g.rec + k] = ((sm[0][k] + sm[1][k]) + sm[2][k]) + sm[3][k];
    }
}

// one workgroup: thread (b, c) reduces the workgroup records of its image in order and derives the Tversky term and its
// gradient factors; thread 0 then adds the terms, the cross-entropy sums and the status in index order
__global__ void __launch_bounds__(256) k_loss_finish(LossArgs g) {
    __shared__ double s_l[256];
    const int n_bc = g.nI * g.ncls;
    double ce_num = 0, ce_den = 0, tv = 0;
    int flags = 0, first = -1;
    for (int base = 0; base < n_bc; base += 256) {
        const int i = base + threadIdx.x;
        if (i < n_bc) {
            const int b = i / g.ncls, c = i - b * g.ncls;
            double tp = 0, fp = 0, fn = 0;
            for (int k = 0; k < g.nblk; ++k) {
                const double *r = g.part + ((size_t)b * g.nblk + k) * g.rec + 3 * c;
                tp += r[0]; fp += r[1]; fn += r[2];
            }
            g.tp[i] = (float)tp; g.fp[i] = (float)fp; g.fn[i] = (float)fn;
            const double al = g.alpha, be = 1.0 - al, D = tp + al * fp + be * fn;
            const double w = g.cw ? (double)g.cw[c] : 1.0, ig = 1.0 / (double)g.gamma;
            double l = 0, ga = 0, gb = 0;
            if (D > 0) {                                   // (D == 0: the image has no annotated pixel; flagged below)
                const double raw = 1.0 - tp / D, lo = g.eps, hi = 1.0 - (double)g.eps;
                const double cl = fmin(fmax(raw, lo), hi);
                l = pow(cl, ig) * w;
                if (raw >= lo && raw <= hi) {              // the clip passes no gradient outside [eps, 1 - eps]
                    const double dl = ig * pow(raw, ig - 1.0) * w * (double)g.w_tv / (double)n_bc;
                    const double d_tp = -(al * fp + be * fn) / (D * D), d_fp = al * tp / (D * D), d_fn = be * tp / (D * D);
                    ga = dl * (d_tp - d_fn);               // d loss / d p[c] on pixels of class c  (tp and fn = sum of 1 - p)
                    gb = dl * d_fp;                        // ... on annotated pixels of any other class
                }
            }
            g.coef[2 * i] = (float)ga; g.coef[2 * i + 1] = (float)gb;
            s_l[threadIdx.x] = l;
        }
        __syncthreads();
        if (threadIdx.x == 0)
            for (int k = 0; k < 256 && base + k < n_bc; ++k) tv += s_l[k];
        __syncthreads();
    }
    // the cross-entropy sums and the checks: thread b adds image b's workgroup records in order, thread 0 the images in order
    __shared__ double s_img[256][4];
    for (int base = 0; base < g.nI; base += 256) {
        const int b = base + threadIdx.x;
        if (b < g.nI) {
            double e0 = 0, e1 = 0, e2 = 0, e3 = 0;
            for (int k = 0; k < g.nblk; ++k) {
                const double *e = g.part + ((size_t)b * g.nblk + k) * g.rec + 3 * g.ncls;
                e0 += e[0]; e1 += e[1]; e2 += e[2]; e3 += e[3];
            }
            g.n_annot[b] = (int32_t)e2;
            s_img[threadIdx.x][0] = e0; s_img[threadIdx.x][1] = e1; s_img[threadIdx.x][2] = e2; s_img[threadIdx.x][3] = e3;
        }
        __syncthreads();
        if (threadIdx.x == 0)
            for (int k = 0; k < 256 && base + k < g.nI; ++k) {
                ce_num += s_img[k][0]; ce_den += s_img[k][1];
                if (s_img[k][2] == 0) { flags |= CPX_LOSS_EMPTY_IMAGE; if (first < 0) first = base + k; }
                if (s_img[k][3] > 0) { flags |= CPX_LOSS_BAD_LABEL; if (first < 0) first = base + k; }
            }
        __syncthreads();
    }
    if (threadIdx.x != 0) return;
    *g.ce = (float)(ce_num / ce_den);
    *g.tversky = (float)(tv / (double)n_bc);
    g.scal[0] = (float)((double)g.w_ce / ce_den);
    g.status[0] = flags; g.status[1] = first;
}

__global__ void __launch_bounds__(256) k_loss_grad(LossArgs g) {
    __shared__ float s_ga[LOSS_MAX_CLS], s_gb[LOSS_MAX_CLS];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, b = blockIdx.y, blk = blockIdx.x;
    const int T = (g.H >> 3) * (g.W >> 3);
    const int t_end = min(T, (blk + 1) * LOSS_TOK_PER_BLOCK);
    if ((int)threadIdx.x < g.ncls) {
        s_ga[threadIdx.x] = g.coef[2 * (b * g.ncls + threadIdx.x)];
        s_gb[threadIdx.x] = g.coef[2 * (b * g.ncls + threadIdx.x) + 1];
    }
    __syncthreads();
    const float ce_scale = g.scal[0];
    for (int t = blk * LOSS_TOK_PER_BLOCK + wave; t < t_end; t += 4) {
        const int y = lane_label(g, b, t, lane);
        const bool use = y >= 0 && y < g.ncls;
        const size_t row = (size_t)b * T + t;
        float *d = g.dlogits + row * ((size_t)g.ncls * 64) + lane;
        if (!use) {                                         // not annotated: exactly zero
            for (int c = 0; c < g.ncls; ++c) d[c * 64] = 0.f;
            continue;
        }
        const float *z = g.head + row * g.ld_head + g.col0 + lane;
        float mx, ls;
        lane_lse(z, g.ncls, mx, ls);
        float S = 0.f;                                      // sum_c p[c] G[c],  G[c] = d loss / d p[c] of this pixel
        for (int c = 0; c < g.ncls; ++c) S += expf((z[c * 64] - mx) - ls) * (c == y ? s_ga[c] : s_gb[c]);
        const float wy = (g.cw ? g.cw[y] : 1.f) * ce_scale;
        for (int c = 0; c < g.ncls; ++c) {
            const float p = expf((z[c * 64] - mx) - ls);
            const float G = c == y ? s_ga[c] : s_gb[c];
            d[c * 64] = p * (G - S) + wy * (p - (c == y ? 1.f : 0.f));
        }
    }
}

template <int NC>
__global__ void __launch_bounds__(256) k_loss_grad_reg(LossArgs g) {
    __shared__ float s_ga[NC], s_gb[NC];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, b = blockIdx.y, blk = blockIdx.x;
    const int T = (g.H >> 3) * (g.W >> 3);
    const int t_end = min(T, (blk + 1) * LOSS_TOK_PER_BLOCK);
    if ((int)threadIdx.x < NC) {
        const bool in = (int)threadIdx.x < g.ncls;
        s_ga[threadIdx.x] = in ? g.coef[2 * (b * g.ncls + threadIdx.x)] : 0.f;
        s_gb[threadIdx.x] = in ? g.coef[2 * (b * g.ncls + threadIdx.x) + 1] : 0.f;
    }
    __syncthreads();
    const float ce_scale = g.scal[0];
    for (int t = blk * LOSS_TOK_PER_BLOCK + wave; t < t_end; t += 4) {
        const int y = lane_label(g, b, t, lane);
        const bool use = y >= 0 && y < g.ncls;
        const size_t row = (size_t)b * T + t;
        float *d = g.dlogits + row * ((size_t)g.ncls * 64) + lane;
        const float *zp = g.head + row * g.ld_head + g.col0 + lane;
        float z[NC], mx = zp[0], s = 0.f, S = 0.f;
#pragma unroll
        for (int c = 0; c < NC; ++c) { z[c] = c < g.ncls ? zp[c * 64] : 0.f; if (c < g.ncls) mx = fmaxf(mx, z[c]); }
#pragma unroll
        for (int c = 0; c < NC; ++c) if (c < g.ncls) s += expf(z[c] - mx);
        const float ls = logf(s);
#pragma unroll
        for (int c = 0; c < NC; ++c) { z[c] = expf((z[c] - mx) - ls); if (c < g.ncls) S += z[c] * (c == y ? s_ga[c] : s_gb[c]); }     // z[c] is p[c] from here
        const float wy = use ? (g.cw ? g.cw[y] : 1.f) * ce_scale : 0.f;
#pragma unroll
        for (int c = 0; c < NC; ++c) {
            if (c < g.ncls) {
                const float G = c == y ? s_ga[c] : s_gb[c];
                d[c * 64] = use ? z[c] * (G - S) + wy * (z[c] - (c == y ? 1.f : 0.f)) : 0.f;       // not annotated: exactly zero
            }
        }
    }
}

extern "C" int cpx_class_loss(const float *head, int ld_head, int col0, const int16_t *labels, int nI, int H, int W, int ncls,
                              const float *class_weights, float alpha, float gamma, float eps, float w_ce, float w_tv,
                              float *ce, float *tversky, float *tp, float *fp, float *fn, int32_t *n_annot, float *dlogits,
                              int32_t *status, void *workspace, size_t workspace_bytes, void *stream) {
    CPX_REQUIRE(head && labels && ce && tversky && tp && fp && fn && n_annot && dlogits && status && workspace);
    CPX_REQUIRE(nI > 0 && nI <= 65535 && H > 0 && W > 0 && H % 8 == 0 && W % 8 == 0 && ncls >= 2 && ncls <= LOSS_MAX_CLS);
    CPX_REQUIRE(col0 >= 0 && ld_head >= col0 + ncls * 64 && gamma > 0.f && eps >= 0.f && eps < 0.5f);
    CPX_REQUIRE((size_t)nI * (H / 8) * (W / 8) < 0x7fffffffull);
    const LossWs L = loss_ws(nI, H, W, ncls);
    CPX_REQUIRE(workspace_bytes >= L.total && ((uintptr_t)workspace & 7) == 0);
    LossArgs g;
    g.head = head; g.ld_head = ld_head; g.col0 = col0; g.labels = labels; g.nI = nI; g.H = H; g.W = W; g.ncls = ncls;
    g.nblk = L.nblk; g.rec = L.rec; g.cw = class_weights; g.alpha = alpha; g.gamma = gamma; g.eps = eps; g.w_ce = w_ce; g.w_tv = w_tv;
    g.part = (double *)((char *)workspace + L.off_part); g.coef = (float *)((char *)workspace + L.off_coef);
    g.scal = (float *)((char *)workspace + L.off_scal);
    g.ce = ce; g.tversky = tversky; g.tp = tp; g.fp = fp; g.fn = fn; g.n_annot = n_annot; g.status = status; g.dlogits = dlogits;
    hipStream_t s = (hipStream_t)stream;
    dim3 grid(L.nblk, nI), block(256);
    const bool reg = ncls <= LOSS_REG_CLS;            // else the general kernels: class loops at run time, logits re-read from the cache
    if (reg) hipLaunchKernelGGL(k_loss_sums_reg<LOSS_REG_CLS>, grid, block, 0, s, g);
    else hipLaunchKernelGGL(k_loss_sums, grid, block, 0, s, g);
    CPX_CHECK_LAUNCH();
    hipLaunchKernelGGL(k_loss_finish, dim3(1), block, 0, s, g);
    CPX_CHECK_LAUNCH();
    if (reg) hipLaunchKernelGGL(k_loss_grad_reg<LOSS_REG_CLS>, grid, block, 0, s, g);
    else hipLaunchKernelGGL(k_loss_grad, grid, block, 0, s, g);
    CPX_CHECK_LAUNCH();
    return CPX_OK;
}

// ---------------------------------------------------------------------------
// segmentation loss of the flow head (`--freeze backbone neck`: seg_trainable, classpose/train.py:482-489)
// ---------------------------------------------------------------------------
// cellpose train._loss_fn_seg (restated from cellpose 4.0.x): MSELoss(mean)(flow logits, 5 * flow targets) / 2 +
// BCEWithLogitsLoss(mean)(cellprob logits, mask > 0.5).  Neither mean depends on the data, so one pass writes the gradient and the
// per-workgroup float64 partial sums; k_seg_finish adds them per image and then over the images, both in index order.
struct SegArgs {
    const float *head; int ld_head;
    const float *tgt;
    int nI, H, W, nblk;
    float g_flow, g_cp;             // w_seg / (2 nI H W), w_seg / (nI H W)
    double *part;
    float *flow, *cp, *dlogits;
};

__global__ void __launch_bounds__(256) k_seg_loss(SegArgs g) {
    __shared__ double sm[4][2];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, b = blockIdx.y, blk = blockIdx.x;
    const int tw = g.W >> 3, T = (g.H >> 3) * tw;
    const int t_end = min(T, (blk + 1) * LOSS_TOK_PER_BLOCK);
    const size_t HW = (size_t)g.H * g.W;
    double s_flow = 0, s_cp = 0;
    for (int t = blk * LOSS_TOK_PER_BLOCK + wave; t < t_end; t += 4) {
        const int ph = t / tw, pw = t - ph * tw;
        const size_t px = (size_t)(8 * ph + (lane >> 3)) * g.W + 8 * pw + (lane & 7);
        const float *tg = g.tgt + (size_t)b * 3 * HW + px;
        const float y = tg[0] > 0.5f ? 1.f : 0.f, ty = tg[HW], tx = tg[2 * HW];
        const size_t row = (size_t)b * T + t;
        const float *z = g.head + row * g.ld_head + lane;
        const float zy = z[0], zx = z[64], zc = z[128];
        const float dy = zy - 5.f * ty, dx = zx - 5.f * tx;
        s_flow += 0.5 * ((double)dy * (double)dy) + 0.5 * ((double)dx * (double)dx);
        const float e = expf(-fabsf(zc));                          // in (0, 1]: nothing overflows at any logit
        s_cp += (double)(fmaxf(zc, 0.f) - zc * y) + (double)log1pf(e);
        const float sig = zc >= 0.f ? 1.f / (1.f + e) : e / (1.f + e);
        float *d = g.dlogits + row * 192 + lane;
        d[0] = dy * g.g_flow; d[64] = dx * g.g_flow; d[128] = (sig - y) * g.g_cp;
    }
    s_flow = wave_sum(s_flow); s_cp = wave_sum(s_cp);
    if (lane == 0) { sm[wave][0] = s_flow; sm[wave][1] = s_cp; }
    __syncthreads();
    if (threadIdx.x < 2) {
        const int k = threadIdx.x;
        g.part[((size_t)b * g.nblk + blk) * 2 + k] = ((sm[0][k] + sm[1][k]) + sm[2][k]) + sm[3][k];
    }
}

__global__ void __launch_bounds__(256) k_seg_finish(SegArgs g) {
    __shared__ double s_img[256][2];
    double flow = 0, cp = 0;
    for (int base = 0; base < g.nI; base += 256) {
        const int b = base + threadIdx.x;
        if (b < g.nI) {
            double e0 = 0, e1 = 0;
            for (int k = 0; k < g.nblk; ++k) {
                const double *e = g.part + ((size_t)b * g.nblk + k) * 2;
                e0 += e[0]; e1 += e[1];
            }
            s_img[threadIdx.x][0] = e0; s_img[threadIdx.x][1] = e1;
        }
        __syncthreads();
        if (threadIdx.x == 0)
            for (int k = 0; k < 256 && base + k < g.nI; ++k) { flow += s_img[k][0]; cp += s_img[k][1]; }
        __syncthreads();
    }
    if (threadIdx.x != 0) return;
    const double n = (double)g.nI * (double)g.H * (double)g.W;
    *g.flow = (float)(flow / (2.0 * n));
    *g.cp = (float)(cp / n);
}

static int seg_nblk(int H, int W) { return ((H / 8) * (W / 8) + LOSS_TOK_PER_BLOCK - 1) / LOSS_TOK_PER_BLOCK; }
extern "C" size_t cpx_seg_loss_workspace_bytes(int nI, int H, int W) {
    if (nI <= 0 || H <= 0 || W <= 0 || H % 8 || W % 8) return 0;
    return cpx_align_up((size_t)nI * seg_nblk(H, W) * 2 * sizeof(double), 256);
}
extern "C" int cpx_seg_loss(const float *head, int ld_head, const float *targets, int nI, int H, int W, float w_seg, float *flow,
                            float *cp, float *dlogits, void *workspace, size_t workspace_bytes, void *stream) {
    CPX_REQUIRE(head && targets && flow && cp && dlogits && workspace);
    CPX_REQUIRE(nI > 0 && nI <= 65535 && H > 0 && W > 0 && H % 8 == 0 && W % 8 == 0 && ld_head >= 192);
    CPX_REQUIRE((size_t)nI * (H / 8) * (W / 8) < 0x7fffffffull);
    CPX_REQUIRE(workspace_bytes >= cpx_seg_loss_workspace_bytes(nI, H, W) && ((uintptr_t)workspace & 7) == 0);
    SegArgs g;
    g.head = head; g.ld_head = ld_head; g.tgt = targets; g.nI = nI; g.H = H; g.W = W; g.nblk = seg_nblk(H, W);
    const double n = (double)nI * (double)H * (double)W;
    g.g_flow = (float)((double)w_seg / (2.0 * n)); g.g_cp = (float)((double)w_seg / n);
    g.part = (double *)workspace; g.flow = flow; g.cp = cp; g.dlogits = dlogits;
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(k_seg_loss, dim3(g.nblk, nI), dim3(256), 0, s, g);
    CPX_CHECK_LAUNCH();
    hipLaunchKernelGGL(k_seg_finish, dim3(1), dim3(256), 0, s, g);
    CPX_CHECK_LAUNCH();
    return CPX_OK;
}

// ---------------------------------------------------------------------------
// weight gradient of the 1x1 head: dW [N][256] = dlogits^T feat, db [N] = column sums of dlogits
// ---------------------------------------------------------------------------
// One workgroup = one (32-column tile of dlogits, slab of UW_SLAB rows); wave w owns feature channels [64 w, 64 w + 64).
// v_mfma_f32_32x32x2_f32 reduces over two ROWS per issue: lane (r, h2) feeds dlogits[row + h2][n0 + r] and
// feat[row + h2][k0 + r] straight from global memory (128-byte row segments), the features widened exactly to float32.
// Partials [slab][N][256] float32 and [slab][N] float64, added by k_wgrad_reduce in slab order in float64, rounded once.
template <int DT>
__global__ void __launch_bounds__(256) k_wgrad(const float *__restrict__ dl, const void *__restrict__ feat, int rows, int N,
                                               float *__restrict__ part_w, double *__restrict__ part_b) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, r = lane & 31, h2 = lane >> 5;
    const int n0 = blockIdx.x * 32, slab = blockIdx.y, k0 = wave * 64;
    const int row0 = slab * UW_SLAB, row1 = min(rows, row0 + UW_SLAB);
    f32x16 acc0, acc1;
#pragma unroll
    for (int v = 0; v < 16; ++v) { acc0[v] = 0.f; acc1[v] = 0.f; }
    double bsum = 0;
#pragma unroll 8
    for (int i = 0; i < UW_SLAB / 2; ++i) {                           // (uniform trip count: the MFMA needs every lane)
        const int row = row0 + 2 * i + h2;
        const bool in = row < row1;
        const float a = in ? dl[(size_t)row * N + n0 + r] : 0.f;
        const float b0 = in ? load_f32<DT>(feat, (size_t)row * WG_FEAT + k0 + r) : 0.f;
        const float b1 = in ? load_f32<DT>(feat, (size_t)row * WG_FEAT + k0 + 32 + r) : 0.f;
        acc0 = MFMA_F32(a, b0, acc0);
        acc1 = MFMA_F32(a, b1, acc1);
        bsum += (double)a;
    }
    // accumulator register v of lane (r, h2): dlogits column n0 + (v&3) + 8*(v>>2) + 4*h2, feature k0 + r
    float *pw = part_w + ((size_t)slab * N + n0) * WG_FEAT + k0 + r;
#pragma unroll
    for (int v = 0; v < 16; ++v) {
        const int n = (v & 3) + 8 * (v >> 2) + 4 * h2;
        pw[(size_t)n * WG_FEAT] = acc0[v];
        pw[(size_t)n * WG_FEAT + 32] = acc1[v];
    }
    if (wave == 0) {
        bsum += __shfl_xor(bsum, 32, 64);                              // even rows + odd rows
        if (h2 == 0) part_b[(size_t)slab * N + n0 + r] = bsum;
    }
}

__global__ void __launch_bounds__(256) k_wgrad_reduce(const float *__restrict__ part_w, const double *__restrict__ part_b,
                                                      int n_slabs, int N, float *__restrict__ dW, float *__restrict__ db) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x, nw = (size_t)N * WG_FEAT;
    if (i < nw) {
        double s = 0;
        for (int k = 0; k < n_slabs; ++k) s += (double)part_w[(size_t)k * nw + i];
        dW[i] = (float)s;
    }
    if (i < (size_t)N) {
        double s = 0;
        for (int k = 0; k < n_slabs; ++k) s += part_b[(size_t)k * N + i];
        db[i] = (float)s;
    }
}

static size_t wgrad_part_b_off(int rows, int N) {
    const size_t n_slabs = (size_t)(rows + UW_SLAB - 1) / UW_SLAB;
    return cpx_align_up(n_slabs * N * WG_FEAT * sizeof(float), 256);
}
extern "C" int cpx_head_wgrad_slab_rows(void) { return UW_SLAB; }
extern "C" size_t cpx_head_wgrad_workspace_bytes(int rows, int n_cols) {
    if (rows <= 0 || n_cols <= 0 || n_cols % 32) return 0;
    const size_t n_slabs = (size_t)(rows + UW_SLAB - 1) / UW_SLAB;
    return wgrad_part_b_off(rows, n_cols) + cpx_align_up(n_slabs * n_cols * sizeof(double), 256);
}
extern "C" int cpx_head_wgrad(const float *dlogits, const void *feat, int dtype, int rows, int n_cols, float *dW, float *db,
                              void *workspace, size_t workspace_bytes, void *stream) {
    CPX_REQUIRE(dlogits && feat && dW && db && workspace && rows > 0 && n_cols > 0 && n_cols % 32 == 0);
    CPX_REQUIRE(dtype_ok(dtype));
    CPX_REQUIRE(workspace_bytes >= cpx_head_wgrad_workspace_bytes(rows, n_cols) && ((uintptr_t)workspace & 7) == 0);
    const int n_slabs = (rows + UW_SLAB - 1) / UW_SLAB;
    CPX_REQUIRE(n_slabs <= 65535);
    float *part_w = (float *)workspace;
    double *part_b = (double *)((char *)workspace + wgrad_part_b_off(rows, n_cols));
    hipStream_t s = (hipStream_t)stream;
    dim3 grid(n_cols / 32, n_slabs), block(256);
    CPX_DT_DISPATCH(dtype, DT, hipLaunchKernelGGL(k_wgrad<DT>, grid, block, 0, s, dlogits, feat, rows, n_cols, part_w, part_b));
    CPX_CHECK_LAUNCH();
    hipLaunchKernelGGL(k_wgrad_reduce, dim3(cpx_cdiv((long long)n_cols * WG_FEAT, 256)), block, 0, s, part_w, part_b, n_slabs, n_cols, dW, db);
    CPX_CHECK_LAUNCH();
    return CPX_OK;
}

// ---------------------------------------------------------------------------
// AdamW
// ---------------------------------------------------------------------------
__global__ void __launch_bounds__(256) k_adamw(float *__restrict__ p, const float *__restrict__ g, float *__restrict__ m,
                                               float *__restrict__ v, long long n, double decay, double beta1, double beta2,
                                               double eps, double step_size, double bc2_sqrt) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const double gi = g[i];
    const double mi = (double)m[i] + (gi - (double)m[i]) * (1.0 - beta1);
    const double vi = (double)v[i] * beta2 + gi * gi * (1.0 - beta2);
    const float mf = (float)mi, vf = (float)vi;                       // the moments are kept in float32, as torch keeps them
    m[i] = mf; v[i] = vf;
    const double denom = sqrt((double)vf) / bc2_sqrt + eps;
    p[i] = (float)((double)p[i] * decay - step_size * ((double)mf / denom));
}

extern "C" int cpx_adamw_step(float *param, const float *grad, float *exp_avg, float *exp_avg_sq, long long n, double lr,
                              double beta1, double beta2, double eps, double weight_decay, double bias_correction1,
                              double bias_correction2, void *stream) {
    CPX_REQUIRE(param && grad && exp_avg && exp_avg_sq && n > 0 && n / 256 < 0x7fffffffLL);
    CPX_REQUIRE(lr >= 0 && beta1 >= 0 && beta1 < 1 && beta2 >= 0 && beta2 < 1 && eps > 0 && weight_decay >= 0);
    CPX_REQUIRE(bias_correction1 > 0 && bias_correction2 > 0);
    hipLaunchKernelGGL(k_adamw, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, param, grad, exp_avg, exp_avg_sq, n,
                       1.0 - lr * weight_decay, beta1, beta2, eps, lr / bias_correction1, sqrt(bias_correction2));
    CPX_CHECK_LAUNCH();
    return CPX_OK;
}
