/*
 * classpose_hip.h -- C ABI of libclasspose_hip.so (MI355X / gfx950 only).
 *
 * Drop-in boundary for the `classpose-predict-wsi` tile path of
 * sohmandal/classpose.  The reference is pure Python; every entry point below
 * replaces one library call the reference makes on that path (cited per
 * function as /root/reference/<file>:<line>, or as the cellpose==4.0.8 /
 * segment-anything==1.0 symbol that call bottoms out in).  INTEGRATION.md shows
 * the ctypes binding a maintainer of the reference would add.
 *
 * Conventions
 *   - every pointer is a DEVICE pointer unless the name ends in `_host`;
 *   - `stream` is a hipStream_t passed as void* (0 = null stream);
 *   - return 0 on success, a negative CPX_E* code otherwise; nothing throws,
 *     nothing allocates: the caller supplies workspaces sized by the
 *     *_workspace_bytes() queries (graph-capture safe);
 *   - tiles are batched: leading dimension nT, then the reference's layout;
 *   - thread-safe for distinct streams + distinct workspaces: the library keeps no mutable
 *     process-global compute state (the element type travels in cpx_net_weights.dtype / the
 *     `dtype` arguments, the optional timing handle in cpx_net_weights.prof); a bf16, an fp16
 *     and an fp32 engine may run from different host threads.  The A/B and ablation switches
 *     of include/classpose_hip_debug.h are process-global test hooks and are NOT covered.
 */
#ifndef CLASSPOSE_HIP_H
#define CLASSPOSE_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define CPX_OK 0
#define CPX_EINVAL (-22)
#define CPX_ENOMEM (-12)
#define CPX_EHIP (-5)

/* element types of the network path (cpx_net_weights.dtype and the `dtype` arguments) */
#define CPX_DT_BF16 0
#define CPX_DT_F16 1
#define CPX_DT_F32 2   /* --precision fp32: exact-f32 MFMA (v_mfma_f32_32x32x2_f32), f32 activations */

/* Library / device identification. Returns the ABI version (this header: 3).
 * Version history: 2 = no process-global compute state (round 2); round 4 ADDED cpx_build_id, cpx_compute_masks_records and
 * cpx_prof_collect_launches without a bump (additive); 3 (round 5) = cpx_prof_collect fills CPX_PROF_N_KINDS = 7 entries (was 5) and
 * the post-processing workspace of cpx_postproc_workspace_bytes holds six table sets per tile -- callers compiled against version 2
 * must be rebuilt, and classpose_amd/_lib.py refuses a library whose version differs.  cpx_pq_workspace_bytes and cpx_pq_stats (the
 * panoptic-quality statistics) and the head-training entry points of section t1 were ADDED later without a bump, like the round-4 additions. */
int cpx_abi_version(void);
/* Last HIP error string recorded by a failing call on this thread (host ptr). */
const char *cpx_last_error(void);
/* which sources this binary was built from: first 16 hex digits of the sha256 over classpose_amd/csrc/{*.hip,*.cpp,*.h,
 * Makefile} (sorted by name) + include/classpose_hip.h + include/classpose_hip_debug.h ("+debug" appended by the
 * -DCPX_DEBUG library).  classpose_amd._lib.source_build_id() recomputes it from the files on disk. */
const char *cpx_build_id(void);

/* ------------------------------------------------------------------------
 * a6  image normalisation
 * replaces cellpose.transforms.normalize_img as called from
 * ClassposeModel.eval, /root/reference/src/classpose/models.py:642-666
 * ---------------------------------------------------------------------- */
/* Per tile and channel: 1st / 99th percentile of the uint8 pixels with numpy's
 * float32 'linear' quantile arithmetic (prev-index + gamma supplied by the host
 * because they only depend on H*W), then x01 / (x99-x01) / mode.
 * tiles_u8 [nT][H][W][3];  stats [nT][3][4] = {x01, x99-x01, mode, unused},
 * mode 0: ptp==0 -> channel left untouched, 1: (x-x01)/(x99-x01), 2: zeros.
 * hist_ws: nT*3*256 uint32.                                               */
int cpx_normalize_stats_u8(const uint8_t *tiles_u8, int nT, int H, int W,
                           int lo_prev, float lo_gamma, int hi_prev, float hi_gamma,
                           float *stats, uint32_t *hist_ws, void *stream);
/* Applies the stats: out_f32 [nT][H][W][3] float32 (what normalize_img returns). */
int cpx_normalize_apply_u8(const uint8_t *tiles_u8, const float *stats, int nT, int H, int W,
                           float *out_f32, void *stream);

/* ------------------------------------------------------------------------
 * a3  residual rescale of a tile read from the pyramid level to the model mpp
 * replaces resize_tile_to_target_mpp -> cv2.resize(tile, (dw, dh), INTER_LINEAR),
 * /root/reference/src/classpose/entrypoints/predict_wsi.py:102-123 (and 462-483)
 * ---------------------------------------------------------------------- */
/* src_u8 [nT][sh][sw][3] -> dst_u8 [nT][dh][dw][3], OpenCV's 8-bit fixed-point
 * bilinear (11-bit weights from the float32 source coordinate, exact 2x2
 * decimation dispatched to the area average like cv::resize does).  Equal sizes
 * copy.  The caller computes dw = max(1, round(sw * resize_factor)) as the
 * reference does.                                                          */
int cpx_resize_linear_u8(const uint8_t *src_u8, int nT, int sh, int sw,
                         uint8_t *dst_u8, int dh, int dw, void *stream);

/* ------------------------------------------------------------------------
 * a7  sub-tiling and taper blending
 * replaces transforms.get_pad_yx + np.pad + transforms.make_tiles in
 * core.run_net, /root/reference/src/classpose/core.py:129-178, and
 * unaugment_tiles / unaugment_class_tiles / average_tiles + crop,
 * core.py:197-231 and transforms/transforms.py:4-21
 * ---------------------------------------------------------------------- */
typedef struct cpx_tiling {
    int H, W;            /* WSI tile size (pixels)                              */
    int ypad1, xpad1;    /* leading zero pad (get_pad_yx)                       */
    int Ly, Lx;          /* padded size                                         */
    int ny, nx;          /* sub-tile grid                                       */
    int bsize;           /* sub-tile size, 256                                  */
    int augment;         /* TTA flips by (j,i) parity                           */
    int ystart[16];      /* np.linspace(0, Ly-bsize, ny).astype(int)            */
    int xstart[16];
} cpx_tiling;

/* Normalised pixels (from stats) -> zero pad -> sub-tile -> flip -> 8x8 patch
 * rows (im2col of the patch-embed conv) in bf16.
 * patches [nT*ny*nx][1024][192], k = c*64 + i*8 + j.                       */
int cpx_make_subtiles(const uint8_t *tiles_u8, const float *stats, int nT,
                      const cpx_tiling *tiling_host, void *patches_bf16, void *stream);
/* Same with the element type of the patch rows chosen by `dtype` (CPX_DT_*): what
 * core._forward's X.to(dtype=net dtype) produces, core.py:61-63.             */
int cpx_make_patches(const uint8_t *tiles_u8, const float *stats, int nT,
                     const cpx_tiling *tiling_host, int dtype, void *patches, void *stream);
/* Same but float32 NCHW sub-tiles [nT*ny*nx][3][bsize][bsize] (what
 * make_tiles returns; used by parity tests and the fp32 debug path).        */
int cpx_make_subtiles_f32(const uint8_t *tiles_u8, const float *stats, int nT,
                          const cpx_tiling *tiling_host, float *subtiles, void *stream);
/* Head outputs of all sub-tiles -> per WSI tile dP/cellprob/logits.
 * head [nT*ny*nx][1024][ld_head] float32 token-major; column c*64+i*8+j of the
 * flow block (cols 0..191: dY,dX,cellprob) and of the class block (cols
 * 192..192+ncls*64) is pixel (8*ph+i, 8*pw+j) of channel c (pixel shuffle W2/W3,
 * vit_sam.py:181-188).  taper1d_host: 1-D cellpose taper (float64, bsize).
 * Outputs float32: dP [nT][2][H][W], cellprob [nT][H][W], logits [nT][ncls][H][W]. */
int cpx_blend_subtiles(const float *head, int ld_head, int ncls, int nT,
                       const cpx_tiling *tiling_host, const double *taper1d,
                       float *dP, float *cellprob, float *logits, void *stream);
/* Same from NCHW sub-tile outputs y [nS][3][b][b], y_class [nS][ncls][b][b]
 * (the arrays core.run_net holds before average_tiles).                      */
int cpx_blend_subtiles_nchw(const float *y, const float *y_class, int ncls, int nT,
                            const cpx_tiling *tiling_host, const double *taper1d,
                            float *dP, float *cellprob, float *logits, void *stream);

/* ------------------------------------------------------------------------
 * a9/a10  network forward (ClassTransformer.forward,
 * /root/reference/src/classpose/vit_sam.py:148-197 with flash_forward :15-65)
 * ---------------------------------------------------------------------- */
typedef struct cpx_block_weights {
    const float *ln1_w, *ln1_b;          /* [1024]                            */
    const void *qkv_w;  const float *qkv_b;   /* bf16 [3072][1024], [3072]    */
    const void *proj_w; const float *proj_b;  /* bf16 [1024][1024]            */
    const void *rel_h, *rel_w;           /* bf16 [64][64]: rows 0..62 = table
                                            interpolated to 63 rows, /scale   */
    const float *ln2_w, *ln2_b;
    const void *fc1_w;  const float *fc1_b;   /* bf16 [4096][1024]            */
    const void *fc2_w;  const float *fc2_b;   /* bf16 [1024][4096]            */
    /* LayerNorm folded into the consuming GEMM (cpx_net_weights.fuse_ln = 1): qkv_w / fc1_w
     * hold W * diag(gamma), qkv_b / fc1_b hold b + W.beta, and these are the row sums of the
     * folded (half-rounded) weights; ln*_w / ln*_b are then unused.                        */
    const float *qkv_colsum, *fc1_colsum;     /* [3072], [4096]               */
} cpx_block_weights;

/* Optional UNet semantic head (classpose/unet.py:121-196, chosen when the checkpoint has
 * out_class.encoder_blocks.* keys, predict_wsi.py:1393-1405).  The host flattens it into a list
 * of convolutions over token-major [sub-tile*h*w][C] half tensors; each runs as (im2col |
 * space-to-depth | nothing) + the MFMA GEMM (+ depth-to-space for the transposed convs).    */
typedef struct cpx_conv_op {
    int kind;              /* 0: conv3x3 pad 1, 1: conv2x2 stride 2, 2: convT2x2 stride 2      */
    int src_a, src_b;      /* tensor ids (src_b = -1: none; channel concat a|b); 0 = neck output */
    int dst;               /* tensor id produced (> 0)                                         */
    int cin_a, cin_b, cout;
    int h, w;              /* INPUT spatial size per sub-tile                                  */
    int relu;
    const void *weight;    /* half [Npad][Kpad]; k = tap*(cin_a+cin_b)+c (kinds 0,1), n = tap*cout+co (kind 2) */
    const float *bias;     /* [Npad]                                                           */
} cpx_conv_op;

typedef struct cpx_net_weights {
    int depth;              /* 24 for vit_l                                    */
    int ncls;               /* n_cell_classes (W3.shape[1])                    */
    int n_head_cols;        /* 192 + ncls*64                                   */
    int ld_head;            /* n_head_cols rounded up to 128                   */
    int dtype;              /* CPX_DT_BF16 / CPX_DT_F16 / CPX_DT_F32: element type of every "void *"
                               GEMM operand below (vectors are always float32)            */
    int fuse_ln;            /* 1: norm1 / norm2 are folded into qkv / mlp.lin1 (half types only) */
    const void *pe_w;       /* [1024][192]                                     */
    const float *pe_b;      /* [1024]                                          */
    const float *pos;       /* [1024 tokens][1024] float32                     */
    const cpx_block_weights *blocks;   /* HOST array of depth entries          */
    const void *neck0_w;    /* [256][1024]                                     */
    const float *neck_ln1_w, *neck_ln1_b;
    const void *neck2_w;    /* [256][9*256], k = (ky*3+kx)*256 + c             */
    const float *neck_ln2_w, *neck_ln2_b;
    const void *head_w;     /* [ld_head][256] rows: out (192) then out_class   */
    const float *head_b;    /* [ld_head]                                       */
    int n_unet_ops;         /* 0: 1x1-conv class head inside head_w; > 0: UNet head below      */
    const cpx_conv_op *unet_ops;   /* HOST array; the last op writes the ncls*64 class columns  */
    void *prof;             /* NULL, or a handle from cpx_prof_create: per-launch HIP-event timing   */
} cpx_net_weights;

/* ------------------------------------------------------------------------
 * a5  checkpoint -> kernel operands on the device (round 6, additive: no ABI bump)
 * replaces the host-side `net.to(torch.bfloat16 | torch.float16)` of ClassposeModel.__init__ as driven by
 * /root/reference/src/classpose/entrypoints/predict_wsi.py:659-727 (`resolve_precision`, models.py:37-69): the float32
 * checkpoint is uploaded as stored and rounded here.
 *   cpx_round_weights   dst[i] = round-to-nearest-even(src[i]) in `dtype`; keep_f32 = 0: stored as 2-byte elements (GEMM operands),
 *                       keep_f32 = 1: widened back to float32 (epilogue vectors).  dtype = CPX_DT_F32: a copy (keep_f32 must be 1).
 *                       src and dst 16-byte aligned; dst may not alias src unless keep_f32.
 *   cpx_fold_layernorm  LayerNorm folded into the Linear that consumes it (cpx_net_weights.fuse_ln): with every input first rounded to
 *                       `dtype`, w_folded[n][k] = round(w[n][k] * gamma[k]), b_folded[n] = b[n] + sum_k w[n][k] beta[k],
 *                       colsum[n] = sum_k w_folded[n][k]; both sums in float64 (fixed order), rounded once to float32.
 *                       w [N][K] float32, w_folded [N][K] 2-byte elements.                                                        */
int cpx_round_weights(const float *src, void *dst, long long n, int dtype, int keep_f32, void *stream);
int cpx_fold_layernorm(const float *w, const float *b, const float *gamma, const float *beta, int N, int K, int dtype,
                       void *w_folded, float *b_folded, float *colsum, void *stream);
/* The whole checkpoint in one call: job i streams its float32 HOST source(s) into the device staging area (stage_base + stage_off[k],
 * 16-byte aligned offsets, disjoint per job) with hipMemcpyAsync on `stream` and queues the kernel above behind the copy.
 *   CPX_WJ_ROUND_HALF / CPX_WJ_ROUND_F32  src_host[0] [n] -> dst[0] (cpx_round_weights, keep_f32 = 0 / 1)
 *   CPX_WJ_COPY_F32                       src_host[0] [n] -> dst[0] float32 as stored (no staging)
 *   CPX_WJ_FOLD_LN                        src_host = {w [n][K], b [n], gamma [K], beta [K]} -> dst = {w_folded, b_folded, colsum}
 * The sources may be pageable (the pages of a memory-mapped checkpoint); they must stay valid until the stream has run.       */
#define CPX_WJ_ROUND_HALF 0
#define CPX_WJ_ROUND_F32 1
#define CPX_WJ_COPY_F32 2
#define CPX_WJ_FOLD_LN 3
typedef struct cpx_weight_job {
    int op;                     /* CPX_WJ_*                                             */
    int dtype;                  /* CPX_DT_BF16 / CPX_DT_F16 (CPX_WJ_COPY_F32: ignored)  */
    long long n;                /* elements; CPX_WJ_FOLD_LN: rows N                     */
    int K;                      /* CPX_WJ_FOLD_LN: columns                              */
    int reserved;
    const void *src_host[4];
    size_t stage_off[4];
    void *dst[3];
} cpx_weight_job;
int cpx_weights_build(const cpx_weight_job *jobs_host, int n_jobs, void *stage_base, size_t stage_bytes, void *stream);

size_t cpx_net_workspace_bytes(int n_subtiles, int dtype);
/* extra bytes (appended to the network workspace) when w->n_unet_ops > 0 */
size_t cpx_unet_workspace_bytes(const cpx_conv_op *ops_host, int n_ops, int n_subtiles, int dtype);
int cpx_unet_head_forward(const cpx_conv_op *ops_host, int n_ops, const void *feat, int n_subtiles,
                          float *head, int ld_head, int col0, int dtype, void *workspace,
                          size_t workspace_bytes, void *stream);
/* patches [nS*1024][192] of w_host->dtype -> head [nS*1024][ld_head] float32
 * (the .float() of core._forward, core.py:67).                               */
/* row parts the MLP of every layer is run in by cpx_net_forward (1, or floor(n_subtiles / 16) for >= 32 sub-tiles: parts of 16 384 token rows, the last
 * one with the remainder, whose hidden activations stay in the Infinity Cache between mlp.lin1 and mlp.lin2) -- what a profiled mlp.lin1 / mlp.lin2
 * launch covers is n_subtiles / parts sub-tiles (exactly, when 16 divides n_subtiles)                                                           */
int cpx_net_mlp_parts(int n_subtiles, int dtype);
int cpx_net_forward(const cpx_net_weights *w_host, const void *patches, int n_subtiles,
                    float *head, void *workspace, size_t workspace_bytes, void *stream);

/* Per-launch timing of the dominant kernels of cpx_net_forward (bench.py's roofline lines): HIP
 * events recorded on the launch stream around every `stride`-th layer's kernels (the sampled layers
 * rotate by one per forward, so every layer is covered equally over `stride` forwards) of the kinds in
 * kinds_mask (bit 0 mlp.lin1, 1 attention, 2 qkv, 3 attn.proj, 4 mlp.lin2; once per forward, whatever the
 * stride: 5 the patch embedding, 6 ONE span over neck + head = the launches behind the last block).  The handle
 * is carried in cpx_net_weights.prof and belongs to one engine / host thread.  cpx_prof_collect (after a stream
 * sync) fills ms_sum[CPX_PROF_N_KINDS] / count[CPX_PROF_N_KINDS] per kind and resets the handle.  */
#define CPX_PROF_N_KINDS 7
int cpx_prof_create(int max_launches, int stride, unsigned kinds_mask, void **prof_out);
int cpx_prof_collect(void *prof, double *ms_sum, int *count);
/* the same launches one by one (launch order; ms[i], kind[i] for i < min(n, cap); *n_out = n; no reset: call it before
 * cpx_prof_collect) -- bench.py reports min / median / max per stage from these                                      */
int cpx_prof_collect_launches(void *prof, float *ms, int *kind, int cap, int *n_out);
void cpx_prof_destroy(void *prof);

/* ------------------------------------------------------------------------
 * a20  GrandQC tissue / artefact networks: UNet++ decoder on an EfficientNet-B0 encoder
 * replaces model.predict(x_tensor) + np.argmax in detect_tissue_wsi / detect_artefacts_wsi,
 * /root/reference/src/classpose/grandqc/wsi_tissue_detection.py:153-158 and
 * wsi_artefact_detection.py:190-195 (smp.UnetPlusPlus("timm-efficientnet-b0"), float32)
 * ---------------------------------------------------------------------- */
/* The host flattens the network into float32 NHWC operations over one workspace (BatchNorm
 * folded into weights/bias; byte offsets, (size_t)-1 = none).
 *  kind 0  dense k x k convolution as an implicit GEMM on v_mfma_f32_32x32x2_f32.  Input
 *          channels = source A (c_a channels, row stride ld_a floats, read through a nearest
 *          x2 upsample if up_a, scaled by gate[n][c] if gate) followed by source B (c_b, ld_b;
 *          the UNet++ concat buffer slice).  w [c_out rounded up to 32|64][k*k][pad16(c_a)+pad16(c_b)],
 *          bias [same rounding]; out = act(acc + bias) (+ res) -> dst with row stride ld_dst.
 *  kind 1  depthwise k x k convolution over source A; w [k*k][c_a], bias [c_a]; dst stride c_a.
 *  kind 2  squeeze-excite gate of source A: dst [nB][c_a] = sigmoid(w2 silu(w mean + bias) + bias2),
 *          w [c_red][c_a], w2 [c_a][c_red]; res = scratch of 16*nB*c_a floats.
 * h_in/w_in are the LOGICAL input grid (after the upsample).  act: 0 none, 1 ReLU, 2 SiLU.   */
typedef struct cpx_qc_op {
    int kind, k, stride, pad, act;
    int h_in, w_in, h_out, w_out;
    size_t src_a, src_b, gate, res, dst;
    int c_a, ld_a, up_a, c_b, ld_b, ld_res, c_out, ld_dst, c_red;
    const float *w, *bias, *w2, *bias2;
} cpx_qc_op;
/* patches_u8 [nB][H][W][3] (H, W multiples of 32) -> ImageNet preprocessing into
 * workspace+input_off ([nB][H][W][4] float, 4th channel 0) -> ops -> argmax of the first
 * n_classes floats of each ld_logits-wide row at workspace+logits_off -> class_map int8
 * [nB][H][W] (first maximum wins, like np.argmax); logits_out (optional) [nB][H][W][n_classes]. */
int cpx_qc_forward(const cpx_qc_op *ops_host, int n_ops, const uint8_t *patches_u8, int nB, int H, int W,
                   size_t input_off, size_t logits_off, int n_classes, int ld_logits,
                   int8_t *class_map, float *logits_out, void *workspace, size_t workspace_bytes,
                   void *stream);

/* Building blocks (exposed for parity tests / rooflines).
 * C[M][N] = A[M][K] * W[N][K]^T (+epilogue).  M%128==0, N%128==0, K%64==0.    */
#define CPX_EPI_BF16 0            /* out bf16 = acc (+bias if bias)            */
#define CPX_EPI_GELU_BF16 1       /* out bf16 = gelu_erf(acc + bias)           */
#define CPX_EPI_RESID_BF16 2      /* out bf16 = resid + acc + bias             */
#define CPX_EPI_F32 3             /* out f32  = acc (+bias)                    */
#define CPX_EPI_POS_BF16 4        /* out bf16 = acc + bias + pos[row%1024]     */
#define CPX_EPI_RELU_BF16 5
#define CPX_EPI_QKV_BF16 6        /* out bf16 [M][3072] = acc + bias; the V third (cols >= 2048) is
                                     ALSO/INSTEAD written transposed to aux = vT [M/1024][16][64][1024] */
int cpx_gemm_bf16(const void *A, const void *Wt, int M, int N, int K, int epilogue,
                  const float *bias, const void *resid_or_pos, void *out, int ld_out,
                  void *stream);
/* Same for any element type.  CPX_DT_F32: A, Wt, resid and out are float32 (out always f32, the
 * QKV epilogue is the plain one: the f32 attention reads V from the qkv rows), K % 16 == 0.  */
int cpx_gemm(int dtype, const void *A, const void *Wt, int M, int N, int K, int epilogue,
             const float *bias, const void *resid_or_pos, void *out, int ld_out, void *stream);

/* 3x3 convolution, padding 1, over 32 x 32-token images as an IMPLICIT GEMM (the neck's Conv2d(256, 256, 3, padding=1,
 * bias=False) of the SAM image encoder; cellpose vit_sam.Transformer): x [M = S*1024][C] token-major
 * (token = 32 y + x), Wt [N][9*C] with k = (3 ky + kx) * C + c, out [M][ld_out] bf16 / fp16.  No im2col buffer: the
 * LDS-DMA of every K tile reads the shifted token's chunk, or a zero chunk outside the image; the accumulation order is
 * that of cpx_gemm on the materialised [M][9*C] operand (bitwise equal).  M % 1024 == 0, N % 128 == 0, C % 64 == 0,
 * epilogue CPX_EPI_BF16 or CPX_EPI_RELU_BF16, dtype CPX_DT_BF16 / CPX_DT_F16.                                      */
int cpx_conv3x3(int dtype, const void *x, const void *Wt, int M, int N, int C, int epilogue, const float *bias,
                void *out, int ld_out, void *stream);
int cpx_gemm_uses_big_tile(int M, int N, int K, int epilogue);
/* Same with a LayerNorm over the K = 1024 input row folded in (consumer) and/or partial row
 * statistics of the output emitted (producer, RESID epilogue, N = 1024, 256^2-tile shapes):
 *   out = rstd[m] * (acc - mean[m] * ln_colsum[n]) + bias[n]     (then the epilogue)
 * ln_stats / stats_out: [M][4][2] float partial (sum, sum of squares); cpx_row_stats fills
 * slot 0 from a [rows][1024] half matrix.  vit_sam.py:175-176 (SAM Block: norm1/norm2). */
int cpx_gemm_ln(const void *A, const void *Wt, int M, int N, int K, int epilogue,
                const float *bias, const void *resid_or_pos, void *out, int ld_out,
                const float *ln_stats, const float *ln_colsum, float *stats_out, void *stream);
int cpx_row_stats(const void *x, int rows, float *stats, void *stream);
int cpx_layernorm_bf16(const void *x, const float *w, const float *b, int rows, int C,
                       float eps, void *out, void *stream);
/* qkv [nS*1024][3072] bf16 (q|k|v, head-major inside) -> attn out [nS*1024][1024]. */
int cpx_attention_relpos(const void *qkv, const void *rel_h, const void *rel_w, int n_subtiles,
                         void *vT_ws, void *out, void *stream);
/* any element type (CPX_DT_F32: float32 qkv / tables [64][64] / out; vT_ws unused)           */
int cpx_layernorm(int dtype, const void *x, const float *w, const float *b, int rows, int C,
                  float eps, void *out, void *stream);
int cpx_attention(int dtype, const void *qkv, const void *rel_h, const void *rel_w, int n_subtiles,
                  void *vT_ws, void *out, void *stream);

/* ------------------------------------------------------------------------
 * a11-a16  flows -> instance ids -> classes
 * ---------------------------------------------------------------------- */
size_t cpx_postproc_workspace_bytes(int nT, int H, int W);
int cpx_postproc_max_labels(int H, int W);
/* Diagnostic, read-only: number of kernel launches this THREAD has issued from the a11-a17 entry points since it first
 * called into the library (difference of two reads = launches of the calls in between).  bench.py reports it next to
 * the device / host times of the dispatch-bound post-processing stage.  Replaces nothing in the reference. */
unsigned long long cpx_postproc_launch_count(void);

/* cellpose.dynamics.follow_flows (steps_interp) as driven by
 * dynamics.compute_masks; call site models.py:149-159.
 * dP [nT][2][H][W] (dY,dX) raw network flows, cellprob [nT][H][W].
 * p_final [nT][H*W] int32: (y<<16)|x of the truncated end point, -1 where
 * cellprob <= threshold.  p_float (nullable) [nT][2][H*W] float end points. */
int cpx_follow_flows(const float *dP, const float *cellprob, int nT, int H, int W,
                     float cellprob_threshold, int niter, int32_t *p_final, float *p_float,
                     void *workspace, void *stream);
/* cellpose.dynamics.get_masks_torch: histogram, 5x5 NMS seeds (>10), 11x11
 * seeded growth (h>2, 5 iters), label gather, big-mask removal, renumber.
 * masks [nT][H*W] int32, nlabels [nT].                                      */
int cpx_get_masks(const int32_t *p_final, int nT, int H, int W, double max_size_fraction,
                  int32_t *masks, int32_t *nlabels, void *workspace, void *stream);
/* cellpose.dynamics.remove_bad_flow_masks (metrics.flow_error +
 * masks_to_flows_gpu, fp64 diffusion).  flow_errors (nullable) [nT][max_labels]. */
int cpx_remove_bad_flow_masks(int32_t *masks, const float *dP, int nT, int H, int W,
                              double threshold, double *flow_errors, void *workspace,
                              void *stream);
/* cellpose.utils.fill_holes_and_remove_small_masks, in place; nlabels (nullable) [nT].
 * Precondition: every id of every tile satisfies 0 <= id < cpx_postproc_max_labels(H, W); the
 * per-label tables are indexed by the id without a check, so an id outside that range writes out
 * of bounds.
 * min_size > 0: small labels out (the reference's positional count quirk included), holes filled
 * label by label, small labels out again; ids 1..n by first raster appearance, nlabels = n.
 * min_size <= 0: no filter and no renumbering by appearance; like the reference's fill loop, the
 * output id of a label is the rank of its id among the ids present BEFORE the fill (ids {2, 5} come
 * back as {1, 2}) and nlabels is their number -- a label that another label's fill overwrites
 * still counts, so the largest id of the output can be smaller than nlabels.               */
int cpx_fill_holes_and_remove_small_masks(int32_t *masks, int nT, int H, int W, int min_size,
                                          int32_t *nlabels, void *workspace, void *stream);
/* classpose.models.compute_class_masks, models.py:191-230.
 * logits [nT][ncls][H][W]; class_masks [nT][H*W] uint8.                      */
int cpx_compute_class_masks(const int32_t *masks, const float *logits, int nT, int ncls, int H,
                            int W, uint8_t *class_masks, void *workspace, void *stream);
/* classpose.metrics.pq.remove_border_instances, metrics/pq.py:65-92
 * (class_masks nullable = the (H,W) form; else the (H,W,2) form).            */
int cpx_remove_border_instances(int32_t *masks, uint8_t *class_masks, int nT, int H, int W,
                                void *workspace, void *stream);
/* The whole of dynamics.resize_and_compute_masks + compute_class_masks
 * (models.py:750-768): masks_u16 [nT][H*W] uint16, class_masks [nT][H*W] uint8. */
int cpx_compute_masks(const float *dP, const float *cellprob, const float *logits, int nT,
                      int ncls, int H, int W, float cellprob_threshold, double flow_threshold,
                      int niter, int min_size, double max_size_fraction, uint16_t *masks_u16,
                      uint8_t *class_masks, int32_t *nlabels, void *workspace, void *stream);


/* Compact per-instance records: what leaves the device in place of the pickled
 * (masks, class_masks) arrays of predict_wsi.py:757-763 / :595-652.          */
typedef struct cpx_record {
    int32_t tile;        /* index in the batch                                 */
    int32_t label;       /* instance id inside the tile                        */
    int32_t cls;         /* class of its first raster pixel (predict_wsi.py:634) */
    int32_t area;        /* pixel count                                        */
    int32_t y0, x0, y1, x1;   /* bbox, end exclusive                           */
    int64_t sum_y, sum_x;     /* pixel-coordinate sums (centroid = sum/area)   */
} cpx_record;
int cpx_instance_records(const uint16_t *masks_u16, const uint8_t *class_masks, int nT, int H,
                         int W, int max_records_per_tile, cpx_record *records,
                         int32_t *counts, void *workspace, void *stream);
/* The same chain with the per-cell records of cpx_instance_records produced by its last pass (records / rec_counts / max_rec
 * as there; both NULL: exactly cpx_compute_masks).  One launch sequence of 22 kernels per batch of tiles (the stage-wise
 * entry points above, called one after the other, need 38): one initialisation for all stages, relabelling rides on the next
 * stage's pixel pass, removals go through the rank table, the records leave with the final pass.  Bit-identical outputs.
 * Replaces: dynamics.resize_and_compute_masks + compute_class_masks (models.py:750-768) and the (masks, class_masks) ->
 * per-cell table step of PostProcessor.__call__ (predict_wsi.py:595-652) for one batch of tiles.                        */
int cpx_compute_masks_records(const float *dP, const float *cellprob, const float *logits, int nT,
                              int ncls, int H, int W, float cellprob_threshold,
                              double flow_threshold, int niter, int min_size,
                              double max_size_fraction, uint16_t *masks_u16,
                              uint8_t *class_masks, int32_t *nlabels, int max_rec, cpx_record *records,
                              int32_t *rec_counts, void *workspace, void *stream);

/* Per-cell class confidence (csrc/cpx_confidence.hip): the vote table behind a record's class, the summed softmax of the
 * class logits and the summed sigmoid of cellprob, per instance.  The reference has nothing like it (its cells carry one
 * hard class name).  A stand-alone pass that runs AFTER cpx_compute_masks_records on what that call read and wrote: the
 * final masks_u16 [nT][H][W], logits [nT][ncls][H][W] float32, cellprob [nT][H][W] float32, rec_counts [nT] (device).
 * For tile t and every label v in 1 .. min(rec_counts[t], max_rec), over the pixels with masks_u16 == v:
 *   votes[t][v-1][c]   int32   pixels whose arg-max class is c -- the rule of the class vote: the first maximum wins, a NaN
 *                              beats every number, the first NaN wins;
 *   prob_q[t][v-1][c]  uint64  sum over pixels of q(p_c), in float64: m = max_c z_c; e_c = exp((double)z_c - m);
 *                              s = sum_c e_c added in class order; p_c = e_c / s; q(p) = llrint(p * 2^24), round half to even.
 *                              A pixel with any non-finite logit adds 0 to every prob_q (it still votes; the denominator
 *                              stays the pixel count);
 *   cellprob_q[t][v-1] uint64  sum over pixels of q(1 / (1 + exp(-(double)z))); a non-finite z adds 0.
 * The sums are exact integers (at most 2^20 pixels * 2^24 per instance), integer atomics only: the result does not depend on
 * arrival order, two runs give the same bits.  Derived per cell on the host in float64, n = sum_c votes[c] (== cpx_record.area):
 *   class_vote_fraction = votes[cls] / n, class_probability = prob_q[cls] / (n * 2^24), detection_probability =
 *   cellprob_q / (n * 2^24), cls the record's class-map value (classpose_amd/confidence.py).
 * votes, prob_q [nT][max_rec][ncls], cellprob_q [nT][max_rec].  Rows < min(rec_counts[t], max_rec) are fully defined: the
 * entry clears exactly those rows itself on the device; every other row is left untouched.  An id of 0, an id above
 * rec_counts[t] and an id above max_rec are background: nothing is read or written through them (any uint16 value is safe).
 * logits == NULL or ncls <= 1: no class part (votes / prob_q untouched, may be NULL); cellprob == NULL: no detection part
 * (cellprob_q untouched, may be NULL); neither part, ncls outside 0 .. 32 (the vote table's class limit) or a short
 * workspace: CPX_EINVAL, nothing is launched.  Two launches on `stream`, allocates nothing.                             */
size_t cpx_instance_confidence_workspace_bytes(int nT, int ncls, int H, int W, int max_rec);
int cpx_instance_confidence(const uint16_t *masks_u16, const float *logits, const float *cellprob,
                            const int32_t *rec_counts, int nT, int ncls, int H, int W, int max_rec,
                            int32_t *votes, uint64_t *prob_q, uint64_t *cellprob_q,
                            void *workspace, size_t workspace_bytes, void *stream);

/* ------------------------------------------------------------------------
 * a10b  eval(diameter=): network-size fields and maps back to the image size
 * replaces transforms.resize_image on dP / cellprob / y_class
 * (/root/reference/src/classpose/models.py:733-748 with resample=True, the
 * _resize_gradients / _resize_cellprob calls of models.py:782-792 otherwise)
 * and on masks / class_masks with cv2.INTER_NEAREST (models.py:804-820)
 * ---------------------------------------------------------------------- */
/* src [n_planes][sh][sw] -> dst [n_planes][dh][dw] float32, every plane on its own: cv2.resize(..., INTER_LINEAR) on
 * float32.  Equal sizes copy.  sh == 2 dh && sw == 2 dw is the area path, ((a + b) + (c + d)) * 0.25f with a, b the
 * upper and c, d the lower pair of the 2 x 2 block, summed in that order.  Otherwise, per axis, scale = 1.0 / ((double)d /
 * (double)s), f = (float)((i + 0.5) * scale - 0.5), s0 = floor(f), f -= s0; in x (s0 < 0) -> (0, 0) and
 * (s0 >= sw - 1) -> (sw - 1, 0); in y the weight is kept and only the two row indices are clipped to [0, sh - 1];
 * h = S[x0] * (1 - fx) + S[x1] * fx on both rows, then h0 * (1 - fy) + h1 * fy, every product and every sum rounded to
 * float32 (no FMA).  Taps and weights are computed in the kernel: no table, no workspace, one launch.               */
int cpx_resize_linear_f32(const float *src, int n_planes, int sh, int sw, float *dst, int dh, int dw, void *stream);
/* The same geometry with cv2.INTER_NEAREST for elements of elem_bytes = 1 (class maps) or 2 (uint16 ids):
 * sx = min((int)floor(x * (1.0 / ((double)dw / sw))), sw - 1), likewise in y.  Equal sizes copy.                    */
int cpx_resize_nearest(const void *src, int elem_bytes, int n_planes, int sh, int sw, void *dst, int dh, int dw,
                       void *stream);

/* ------------------------------------------------------------------------
 * a16b  panoptic-quality statistics (offline evaluation against an annotated set)
 * replaces, per image pair, filter_out_unlabelled_cells (/root/reference/src/classpose/metrics/utils.py:162-252),
 * remove_border_instances (metrics/pq.py:65-92), get_multi_pq_info (metrics/stats_utils.py:8-61) and the pairing of
 * get_pq (stats_utils.py:64-178) as driven by compute_multiclass_pq_metrics / compute_binary_pq_metrics
 * (metrics/pq.py:95-290)
 * ---------------------------------------------------------------------- */
/* true_ids / pred_ids [nI][H][W] instance ids >= 0, 0 = background: int32 (id_bytes 4) or uint16 (id_bytes 2, what cpx_compute_masks
 * writes); true_cls / pred_cls [nI][H][W] uint8, or both NULL = binary mode (one pseudo-class, nr_classes 1, no filter).  Inputs are
 * not modified (the reference edits its arrays in place).  Stages, all on the device:
 *   filter_unlabelled    a true instance without a class > 0 pixel leaves, with every predicted instance whose class-agnostic IoU
 *                        with it is > 0.5 (utils.py:203-244; the reference's early exits remove nothing either);
 *   no_border_instances  then ids with a pixel on the first / last row / column leave, each map on its own (pq.py:56-58);
 *   per class c = 1..nr_classes over the one-class maps inst * (cls == c): iou = inter / (area_true + area_pred - inter) as one
 *                        float64 division of exactly converted integers; a pair counts when iou > match_iou.
 * Outputs [nI][nr_classes]: tp = pairs, fp / fn = predicted / true instances of the class in no pair (int32), iou_sum = the sum of
 * the pairs' iou (float64): accumulated exactly in integer fixed point and rounded once, so it does not depend on the order of
 * arrival and two runs give the same bits.  Reference quirk kept: a one-class map WITHOUT a zero pixel loses its first-appearing
 * instance from the id list (`true_id_list[1:]`, stats_utils.py:108,161-162): a true one is neither paired nor fn, a predicted
 * one is never fp.  nobg (nullable) [nI][2] receives that class per (image, side: 0 true, 1 predicted), else 0.
 * The tables are hash tables of table_cap slots (a power of two >= 16) per image and kind; status [nI] is set to 1 for an image
 * whose tables filled up -- its outputs are then void and the call is to be repeated with a larger table_cap; 2 * H * W slots
 * (rounded up to a power of two) always suffice.
 * Optional lists for the match_iou == 0 branch (scipy's linear_sum_assignment needs the dense matrix, stats_utils.py:144-158; host
 * side): every overlapping same-class pair and every (side, class, instance), in no particular order, an instance identified by the
 * index of its first raster pixel in the one-class map (their order is the reference's row / column order); list_counts [2] = the
 * number of pairs and instances found (may exceed max_pairs / max_insts: then the lists are truncated and the caller enlarges them). */
typedef struct cpx_pq_pair {
    int32_t image, cls;
    int32_t first_true, first_pred;      /* first raster pixel (y * W + x) of the two instances in their one-class maps */
    int32_t inter, area_true, area_pred, reserved;
} cpx_pq_pair;
typedef struct cpx_pq_inst {
    int32_t image, side, cls;            /* side 0 = true, 1 = predicted */
    int32_t first, area, reserved;
} cpx_pq_inst;
size_t cpx_pq_workspace_bytes(int nI, int H, int W, int nr_classes, int table_cap);
int cpx_pq_stats(const void *true_ids, const void *pred_ids, int id_bytes, const uint8_t *true_cls, const uint8_t *pred_cls,
                 int nI, int H, int W, int nr_classes, double match_iou, int filter_unlabelled, int no_border_instances,
                 int table_cap, int32_t *tp, int32_t *fp, int32_t *fn, double *iou_sum, int32_t *status, int32_t *nobg,
                 cpx_pq_pair *pairs, int max_pairs, cpx_pq_inst *insts, int max_insts, int32_t *list_counts,
                 void *workspace, size_t workspace_bytes, void *stream);

/* ------------------------------------------------------------------------
 * t1  training the 1x1 semantic class head with the backbone frozen (csrc/cpx_train.hip; additive, no ABI bump)
 * replaces, for `--freeze backbone segmentation_head neck` (paper_experiments/run_training.py:92-98,354-358,
 * classpose/vit_sam.py:199-249), one step of train_class_seg (classpose/train.py:606-655):
 * net(X) is cpx_net_forward; the rest is below.  Every entry point takes a stream and allocates nothing; no floating-point atomics:
 * every result is bitwise reproducible run to run.
 *
 * cpx_net_neck_offset: byte offset, inside the workspace of cpx_net_forward for the same (n_subtiles, dtype), of the neck output
 *   [n_subtiles * 1024][256] (element type = network dtype) -- the operand of the head GEMM, i.e. the input of out / out_class
 *   (vit_sam.py:233-249).  It is valid after cpx_net_forward has run on the stream and until the next forward on that workspace.
 *   0 = invalid argument.
 * cpx_patchify_f32: float32 NCHW crops x [nS][3][H][W], already normalised (what the reference's loader hands to net(X),
 *   train.py:617-620) -> patch rows [nS * (H/8) * (W/8)][192], k = c*64 + i*8 + j, rounded to `dtype` as X.to(dtype) rounds
 *   (core.py:61-63).  H, W multiples of 8 (the network takes 256).                                                              */
size_t cpx_net_neck_offset(int n_subtiles, int dtype);
int cpx_patchify_f32(const float *x, int nS, int H, int W, int dtype, void *patches, void *stream);

/* cpx_class_loss: _loss_fn_class (train.py:156-181: nn.CrossEntropyLoss(reduction="mean", weight, ignore_index=-100)) and
 *   _loss_fn_tversky (train.py:108-153), their weighted sum as LossAggregator(optimise=False) forms it (train.py:41-84,482-493,642; both
 *   multipliers 1 there) and d(w_ce * CE + w_tv * Tversky) / d logits (what loss.backward(), train.py:645, leaves at out_class's output).
 *   head [nI * (H/8) * (W/8)][ld_head] float32 token-major: column col0 + c*64 + i*8 + j of token (ph, pw) is the class-c logit of
 *   pixel (8 ph + i, 8 pw + j) -- the layout cpx_blend_subtiles reads, col0 = 192 for the head buffer of cpx_net_forward.
 *   labels [nI][H][W] int16, -100 = not annotated; class_weights [ncls] or NULL; 2 <= ncls <= 64.
 *     CE      = sum w[y] * (-log softmax(z)[y]) / sum w[y]                      over the annotated pixels of the batch
 *     Tversky = mean over (image b, class c) of clip(1 - tp / (tp + alpha fp + (1 - alpha) fn), eps, 1 - eps)^(1/gamma) * w[c],
 *               tp = sum p[c] [y = c], fp = sum p[c] [y != c], fn = sum (1 - p[c]) [y = c] over the annotated pixels of image b;
 *               the clip passes no gradient outside [eps, 1 - eps]: a class absent from an image (raw loss exactly 1) contributes
 *               (1 - eps)^(1/gamma) * w[c] and a zero gradient.
 *   Out: ce [1], tversky [1], tp / fp / fn [nI][ncls] float32, n_annot [nI] annotated pixels per image, dlogits
 *   [rows][ncls * 64] float32 in the same column order (rows of pixels that are not annotated are exactly zero), status [2]:
 *   status[0] = CPX_LOSS_* flags, status[1] = the first image they apply to (or -1).  An image without annotated pixels makes the
 *   reference return NaN; here it is flagged (the outputs are then undefined) and the Python layer raises.
 *   Two passes over the logits with a one-workgroup kernel between them; sums are float64, added in a fixed order.                 */
#define CPX_LOSS_EMPTY_IMAGE 1    /* an image has no annotated pixel                    */
#define CPX_LOSS_BAD_LABEL 2      /* a label other than -100 lies outside [0, ncls)     */
size_t cpx_class_loss_workspace_bytes(int nI, int H, int W, int ncls);
int cpx_class_loss(const float *head, int ld_head, int col0, const int16_t *labels, int nI, int H, int W, int ncls,
                   const float *class_weights, float alpha, float gamma, float eps, float w_ce, float w_tv,
                   float *ce, float *tversky, float *tp, float *fp, float *fn, int32_t *n_annot, float *dlogits,
                   int32_t *status, void *workspace, size_t workspace_bytes, void *stream);

/* cpx_head_wgrad: the backward of out_class = nn.Conv2d(256, ncls * 64, 1) (vit_sam.py:199-249) for its own parameters:
 *   dW [n_cols][256] = dlogits^T feat, db [n_cols] = column sums of dlogits; dlogits [rows][n_cols] float32, feat [rows][256] of
 *   `dtype` (widened exactly), n_cols % 32 == 0, float32 out.  v_mfma_f32_32x32x2_f32 (exact float32) over slabs of
 *   cpx_head_wgrad_slab_rows rows; the per-slab partials are added in slab order in float64 and rounded once.                    */
int cpx_head_wgrad_slab_rows(void);
size_t cpx_head_wgrad_workspace_bytes(int rows, int n_cols);
int cpx_head_wgrad(const float *dlogits, const void *feat, int dtype, int rows, int n_cols, float *dW, float *db,
                   void *workspace, size_t workspace_bytes, void *stream);

/* cpx_adamw_step: torch.optim.AdamW (train.py:478-480,648; amsgrad off) on float32 parameters with float32 moments, in place:
 *   p *= 1 - lr * weight_decay;  m += (g - m)(1 - beta1);  v = beta2 v + (1 - beta2) g^2;
 *   p -= lr / bias_correction1 * m / (sqrt(v) / sqrt(bias_correction2) + eps),  bias_correction_i = 1 - beta_i^step from the host.
 *   lr = 0 (the first epoch of the schedule, train.py:460) leaves the parameters bitwise unchanged.                               */
int cpx_adamw_step(float *param, const float *grad, float *exp_avg, float *exp_avg_sq, long long n, double lr,
                   double beta1, double beta2, double eps, double weight_decay, double bias_correction1,
                   double bias_correction2, void *stream);

/* Training the UNet semantic head (csrc/cpx_train_unet.hip): what autograd does for classpose.unet.UNet (unet.py:121-196) under
 * train_class_seg (train.py:482-493) with the backbone and the neck frozen, on the op list that cpx_unet_head_forward runs.  That
 * forward leaves every op's output, in the network dtype, in its workspace: those are the saved activations.
 *   Parameters, gradients and the AdamW moments are ONE flat float32 buffer each: per op its packed operand [Npad][Kpad] (the
 *   layout of cpx_conv_op.weight) followed by its bias [Npad]; cpx_unet_param_layout returns the element count and, where the
 *   pointers are not NULL, the element offsets and the padded sizes per op.
 *   cpx_unet_refresh_operands rounds the flat master parameters into the operands the ops point at (cpx_round_weights each: the
 *   weight to the network dtype, the bias through it and back to float32), as NetWeights builds them at load.
 *   cpx_unet_head_backward: feat [nS*1024][256] of `dtype` (tensor 0), the forward's workspace, dlogits [nS*1024][ncls*64] float32
 *   (cpx_class_loss) -> grads (flat, float32).  Ops are walked in reverse; per op dW = dY^T im2col(X) and db = column sums of dY on
 *   the exact float32 matrix instruction v_mfma_f32_32x32x2_f32 over slabs of cpx_unet_wgrad_slab_rows rows of an im2col operand
 *   that is gathered from the stored tensors, never materialised (per-slab partials added in slab order in float64, rounded once),
 *   and dX = col2im(dY W) with the rounded operand in float32 (the float32 GEMM of cpx_gemm on the transposed operand, then a gather
 *   that adds the taps in tap order, splits the a|b concat, adds a second consumer's contribution to the first's and lets the
 *   last one apply the producer's ReLU mask, stored output > 0).  Rounding to the network dtype is the identity in the backward
 *   (straight-through); the neck output gets no gradient.  No atomics: bitwise reproducible.  Padded channels and the Npad / Kpad
 *   padding get exact zeros.  The workspace holds, at cpx_unet_grad_layout's byte offsets, the gradient [rows_pad][ld] float32
 *   with respect to every op's output but the last (whose gradient is dlogits), after the ReLU mask of that op.              */
int cpx_unet_wgrad_slab_rows(void);
long long cpx_unet_param_layout(const cpx_conv_op *ops_host, int n_ops, long long *w_off, long long *b_off, int *n_pad, int *k_pad);
int cpx_unet_refresh_operands(const cpx_conv_op *ops_host, int n_ops, const float *params, int dtype, void *stream);
size_t cpx_unet_backward_workspace_bytes(const cpx_conv_op *ops_host, int n_ops, int n_subtiles, int dtype);
int cpx_unet_grad_layout(const cpx_conv_op *ops_host, int n_ops, int n_subtiles, int dtype, size_t *g_off, int *g_ld);
int cpx_unet_head_backward(const cpx_conv_op *ops_host, int n_ops, const void *feat, int n_subtiles, int dtype,
                           const void *fwd_workspace, size_t fwd_workspace_bytes, const float *dlogits, float *grads,
                           void *workspace, size_t workspace_bytes, void *stream);

/* Training the neck (csrc/cpx_train_neck.hip; additive, no ABI bump): the reference's `--freeze backbone` (with the flow head) and
 * `--freeze backbone segmentation_head` (vit_sam.py:216-249, run_training.py:92-98).  The neck is the tail of cpx_net_forward:
 *   y0 = x W0^T -> a1 = LayerNorm2d(y0) -> y2 = conv3x3(a1, W2) -> feat = LayerNorm2d(y2) -> head = feat Wh^T + bh.
 * Every entry takes a stream and allocates nothing; no floating-point atomics: bitwise reproducible.  Not with a UNet head
 * (n_unet_ops > 0 is refused: that head's backward gives the neck output no gradient).
 *   cpx_net_backbone_offset: byte offset, inside the workspace of cpx_net_forward for the same (n_subtiles, dtype), of the last
 *   block's output x [n_subtiles * 1024][1024] (network dtype), valid after a forward until the next one (the tail only reads it).
 *   (size_t)-1 = invalid argument (the offset itself is 0).
 *   cpx_neck_forward_train: exactly the launches of that tail on a given x (16-byte aligned), in its order, writing y0 (before
 *   LayerNorm 1), a1 (after it), y2 (before LayerNorm 2) and feat (the neck output), [n_subtiles * 1024][256] of the network dtype
 *   each, at the four byte offsets of cpx_neck_train_layout in `workspace` (256-byte aligned): nothing is overwritten.  head and feat
 *   are bitwise what cpx_net_forward produces for the same n_subtiles.
 *   cpx_layernorm_backward: y [rows][C] as stored (dtype, widened exactly), gamma [C], dout [rows][C] float32, C = 256 (or 1024, below).  Per row, in
 *   float64 from y: mean, biased var, rstd = 1 / sqrt(var + (double)eps), xhat = (y - mean) rstd, g = dout gamma,
 *   dy = rstd (g - mean(g) - xhat mean(g xhat)); dgamma = sum over rows of dout xhat, dbeta = sum over rows of dout.  Row sums:
 *   a fixed butterfly in one wave; column sums: per-workgroup partials over blocks of 64 rows, then one workgroup adds them in block
 *   order.  Every output is rounded to float32 once.  Pointers 16-byte aligned.
 *   cpx_neck_backward: x and the workspace cpx_neck_forward_train ran this batch in, dhead [rows][ld_head] float32 = d loss / d head
 *   (flow columns 0..191 from cpx_seg_loss or zeros, class columns from cpx_class_loss, padding columns 0) -> grads, one flat float32
 *   buffer W0 [256][1024] | gamma1 | beta1 | W2 [256][2304] (k = tap * 256 + c, the operand's layout) | gamma2 | beta2 at the element
 *   offsets of cpx_neck_grad_layout (which returns the element count; off may be NULL).  Steps: dfeat = dhead Wh (the rounded
 *   operand widened, float32 GEMM), LayerNorm 2 backward, dW2 and da1 = col2im(dy2 W2) by the kernels of cpx_unet_head_backward (slabs
 *   of cpx_unet_wgrad_slab_rows rows), LayerNorm 1 backward, dW0 = dy0^T x.  Rounding to the network dtype is the identity
 *   (straight-through); nothing flows to the backbone.  cpx_neck_backward_workspace_bytes also returns, where off is not NULL, the
 *   byte offsets of dfeat, dy2, da1 and dy0 ([rows][256] float32 each) in that workspace.                                        */
size_t cpx_net_backbone_offset(int n_subtiles, int dtype);
size_t cpx_neck_train_workspace_bytes(int n_subtiles, int dtype);
int cpx_neck_train_layout(int n_subtiles, int dtype, size_t *off /* [4]: y0, a1, y2, feat */);
int cpx_neck_forward_train(const cpx_net_weights *w, const void *x, int n_subtiles, float *head, void *workspace,
                           size_t workspace_bytes, void *stream);
size_t cpx_layernorm_backward_workspace_bytes(int rows, int C);
int cpx_layernorm_backward(int dtype, const void *y, const float *gamma, const float *dout, int rows, int C, float eps,
                           float *dy, float *dgamma, float *dbeta, void *workspace, size_t workspace_bytes, void *stream);
long long cpx_neck_grad_layout(long long *off /* [6] or NULL */);
size_t cpx_neck_backward_workspace_bytes(int n_subtiles, int dtype, int ld_head, size_t *off /* [4] or NULL: dfeat, dy2, da1, dy0 */);
int cpx_neck_backward(const cpx_net_weights *w, const void *x, int n_subtiles, const void *fwd_workspace, size_t fwd_workspace_bytes,
                      const float *dhead, float *grads, void *workspace, size_t workspace_bytes, void *stream);

/* Training the transformer blocks: the backward kernels (csrc/cpx_train_blocks.hip; additive, no ABI bump).  Every entry takes a stream
 * and allocates nothing; no floating-point atomics: bitwise reproducible.  All gradients are float32.
 *   cpx_layernorm_backward also takes C = 1024 (a block's norm1 / norm2: 16 channels per lane of the one wave per row); its workspace
 *   for either width is cpx_layernorm_backward_bytes(rows, C) (cpx_layernorm_backward_workspace_bytes keeps answering for C = 256
 *   alone).  For C = 256 every output is bitwise what it was.
 *   cpx_attention_backward: the derivative of the function cpx_attention(CPX_DT_F32, ...) computes, for the architecture's shape (1024
 *   tokens = 32 x 32 per crop, 16 heads of 64), in float32 on v_mfma_f32_32x32x2_f32.  qkv [rows][3072] as stored in `dtype`, widened
 *   exactly (O [rows][1024], the stored attention output, is accepted and not read: delta_i = dO_i . O_i is formed from the recomputed
 *   P, since an O rounded to the network dtype would put its 2^-9 into every dS; it may be NULL); rel_h / rel_w [64][64] of `dtype` in the operand convention of
 *   cpx_block_weights: rel_pos / scale, row 63 zero; dO [rows][1024] float32.  Outputs: dqkv [rows][3072] (dq | dk | dv), drel_h and
 *   drel_w [64][64] float32: the gradients with respect to the OPERAND tables (the caller undoes the 1 / scale), summed over all heads
 *   and crops in a fixed order with float64 partials and rounded once; row 63 is written as zero.  P is recomputed from row maxima and
 *   sums found in a first pass.  Workspace: 8.44 MiB per crop (67.5 MiB for 8 crops, 270 MiB for 32).  Pointers 16-byte aligned, the
 *   workspace 256-byte aligned.
 *   cpx_gelu_backward: dpre = dh * (Phi(pre) + pre phi(pre)), the derivative of the erf GELU of the mlp.lin1 epilogue, n float32
 *   elements (a multiple of 4).
 * The two drivers below (forward, backward) each have ONE body and ONE contract, stated for the widest entry; every older entry is that
 * entry with some arguments fixed (the tables), bit for bit and launch for launch.  keep, in both: NULL, or [n_blocks][n_subtiles] uint8 on
 * the HOST, read before the call returns -- layer drop (stochastic depth, vit_sam.py:165-173): block first_block + j runs on crop n where
 * keep[j][n] != 0,
 *   x_{j+1}[n] = keep[j][n] ? block_j(x_j[n]) : x_j[n]     (the second branch bit for bit)
 * which is the reference's x * mask + blk(x) * (1 - mask) with mask = 1 - keep.  Nothing inside a block crosses a crop, so a block runs on
 * its kept crops alone, compacted in crop order; a dropped (block, crop) pair costs neither a forward nor a backward.  keep NULL or all
 * non-zero is no mask: the launches of the entries without the argument.
 *
 * cpx_blocks_forward_train_drop(w, x, n_subtiles, first_block, keep, head, workspace, workspace_bytes, stream) -- the training forward.
 *   Without a mask: the launches of cpx_net_forward for blocks first_block .. depth - 1 (K = depth - first_block of them), in
 *   their order and with their MLP row parts (cpx_net_mlp_parts), on x [n_subtiles * 1024][1024] (network dtype), the input of block
 *   first_block -- what cpx_net_forward leaves at cpx_net_backbone_offset when run with a host copy of the weights whose depth is
 *   first_block -- then cpx_neck_forward_train.  Kept per trained block, in the network dtype, at the 4 K + 2 byte offsets of
 *   cpx_blocks_train_layout (per block x_in, qkv, ao, x_mid; then x_out, the last block's output, and the neck's training workspace):
 *   the block input, the qkv rows (for the half types with their V third copied back from the transposed V^T the qkv GEMM writes
 *   instead), the attention output and the rows after the attention residual.  Nothing kept is overwritten.  The
 *   backward recomputes both LayerNorm outputs, the lin1 pre-activation, the hidden activations and the softmax in float32.  head, the
 *   neck's tensors and x_out are bitwise cpx_net_forward's for the same n_subtiles for float32, for unfused weights, and for the fused
 *   half types below 16 crops; from 16 crops up cpx_net_forward takes a block's row statistics from the GEMM before it, and the first
 *   trained block takes them from cpx_row_stats instead (same sums, another order).  Not with a UNet head.
 *   Under a mask: the running full-batch rows live in the x_out record; per block the kept crops are gathered into the block's x_in
 *   record (with their statistics where the weights fold LayerNorm), the block runs on n_keep crops exactly as it runs without a mask on a
 *   batch of n_keep, and its output is scattered back.  The x_in, qkv, ao and x_mid records of block j hold n_keep_j * 1024 valid rows at
 *   their front; a block that keeps nothing launches nothing; x_out and the neck cover all crops.
 *   workspace: cpx_blocks_train_workspace_bytes_drop (the layout of cpx_blocks_train_layout, then one staging tensor of the batch's
 *   rows); without a mask the size of cpx_blocks_train_workspace_bytes, which ends before the staging tensor, suffices.
 *     cpx_blocks_forward_train(w, x, n, first_block, head, ...)   = cpx_blocks_forward_train_drop with keep NULL
 *
 * cpx_blocks_backward_drop(w, params, n_subtiles, first_block, keep, fwd_workspace, fwd_workspace_bytes, dy0, grad_dtype, attn_grad_dtype,
 * grads, dx_all, dx_in, workspace, workspace_bytes, stream) -- the backward of that forward.
 *   Walks the trained blocks in reverse from dy0 [rows][256] float32 = d loss / d (x_out W0^T), which
 *   cpx_neck_backward leaves at off[3] of its workspace (d x_out = dy0 W0 is formed here).  Per block: lin2 (dW, db, dh), GELU backward,
 *   lin1, LayerNorm 2 backward, the residual add; proj, attention backward, qkv, LayerNorm 1 backward, the residual add.
 *   params: K records of cpx_block_grad_layout holding
 *   the UNFOLDED parameters as the forward reads them (each rounded through the network dtype, float32; the rel slots are not read);
 *   grads: K records of the same layout, ln1 gamma, beta | qkv W, b | rel_h, rel_w [64][64] | proj W, b | ln2 gamma, beta | fc1 W, b |
 *   fc2 W, b: with respect to the unfolded gamma, beta, W, b (not the folded operands of fuse_ln) and to the operand tables.  Where the
 *   forward folds LayerNorm into qkv / lin1, the data gradient and the recomputed pre-activation use the folded operand the forward
 *   multiplied by, and dW, dgamma, dbeta follow from dWf = dpre^T xhat by the chain rule through the fold after the last slab.  Rounding
 *   to the network dtype is the identity (straight-through).
 *   keep: the mask the forward ran with.  The slabs of two adjacent crops and their order stay; per block the body runs on the slab's
 *   kept crops -- two (adjacent in the compact records), one (1024 rows, on that crop's half of the slab's dx) or none (skipped) -- from
 *   the compact row offset 1024 * (kept crops of that block before the slab).  A dropped crop's dx rows pass down untouched, bitwise,
 *   into dx_all and dx_in as well; a block with no kept crop has an all-zero gradient record.
 *   grad_dtype: CPX_DT_F32 -- every dX = dY W and dW = dY^T X is the exact-float32 GEMM behind a transposing copy.  CPX_DT_BF16 (mixed-
 *   precision gradients; additive, no ABI bump) is accepted for a CPX_DT_BF16 network only (fp16 gradients would need loss scaling, a float32 network has
 *   no half operands: both are CPX_EINVAL).  In that mode every matrix product of the backward takes both operands rounded to bf16 (round
 *   to nearest even, each value once), accumulates in float32 on the bf16 MFMA and writes float32:
 *     dW += bf16(dy)^T bf16(a)   da = bf16(dy) W   pre = bf16(xhat or xn) W1^T + b1   d x_out = bf16(dy0) W0
 *   with W the operand the forward multiplied by (exact in bf16, folded where the forward folds) and db += the column sums of the UNROUNDED
 *   float32 dy in float64.  Activation gradients stay float32 between the products; LayerNorm, GELU and attention backward, the unfolding
 *   of the folded gradients, the slabs and their order are those of the float32 mode.
 *   attn_grad_dtype: the precision of the attention backward, a third switch.  CPX_DT_F32 is cpx_attention_backward; CPX_DT_BF16 runs
 *   cpx_attention_backward_bf16 in its place and needs grad_dtype CPX_DT_BF16 (hence a bf16 network); every other combination is
 *   CPX_EINVAL (workspace bytes 0) before anything is launched.
 *   dx_all: NULL, or [K + 1][rows][1024] float32 receiving the gradient of every trained block's input (record j) and of x_out (record K).
 *   dx_in (additive, no ABI bump): NULL, or [rows][1024] float32 receiving the gradient of block first_block's input alone -- record 0 of dx_all without the K
 *   records after it (128 MB at 32 crops where dx_all for K = 24 is 3.3 GB), copied per slab from the same buffer.  16-byte aligned like
 *   its neighbours.  What cpx_embed_backward takes when first_block is 0.
 *   workspaces: fwd_workspace is what the forward filled; workspace has cpx_blocks_backward_workspace_bytes_mp(n_subtiles, dtype,
 *   grad_dtype, attn_grad_dtype) bytes, whatever keep and attn_grad_dtype are (the two attention backwards share one layout).  It is
 *   smaller in the bf16 mode (190 MiB against 241 MiB): it holds no transposed float32 operands.
 *   slabs: the crops go through all blocks in slabs of cpx_blocks_backward_slab_crops() = 2 and the slabs' gradients are added in slab
 *   order, so the workspace does not grow with the batch: 241 MiB for 8 and for 32 crops.
 *   No atomics in any mode or under any mask: two runs are bitwise equal.
 *   CPX_EINVAL, before anything is launched: a null w, params, fwd_workspace, dy0, grads or workspace; workspace or fwd_workspace too
 *   short or not 256-byte aligned; params, dy0, grads, dx_all or dx_in not 16-byte aligned; first_block outside 0 .. depth - 1 or more
 *   than 4096 trained blocks; weights with a UNet head, with a null neck0_w or float32 ones with fuse_ln; n_subtiles * 1024 beyond
 *   2^31 - 2 rows; the precision combinations named above.
 *     cpx_blocks_backward_in(.., dy0, grad_dtype, attn_grad_dtype, grads, dx_all, dx_in, ..)  = cpx_blocks_backward_drop with keep NULL
 *     cpx_blocks_backward_mp(.., dy0, grad_dtype, attn_grad_dtype, grads, dx_all, ..)         = ... and dx_in NULL
 *     cpx_blocks_backward_ex(.., dy0, grad_dtype, grads, dx_all, ..)                          = ... and attn_grad_dtype CPX_DT_F32
 *     cpx_blocks_backward(.., dy0, grads, dx_all, ..)                                         = ... and grad_dtype CPX_DT_F32
 *     cpx_blocks_backward_workspace_bytes_ex(n, dtype, grad_dtype)  = cpx_blocks_backward_workspace_bytes_mp with attn_grad_dtype CPX_DT_F32
 *     cpx_blocks_backward_workspace_bytes(n, dtype)                 = ... and grad_dtype CPX_DT_F32                                       */
size_t cpx_blocks_train_workspace_bytes(int n_subtiles, int dtype, int n_blocks);
size_t cpx_blocks_train_workspace_bytes_drop(int n_subtiles, int dtype, int n_blocks);
int cpx_blocks_train_layout(int n_subtiles, int dtype, int n_blocks, size_t *off /* [4 * n_blocks + 2] */);
int cpx_blocks_forward_train_drop(const cpx_net_weights *w, const void *x, int n_subtiles, int first_block, const unsigned char *keep,
                                  float *head, void *workspace, size_t workspace_bytes, void *stream);
int cpx_blocks_forward_train(const cpx_net_weights *w, const void *x, int n_subtiles, int first_block, float *head, void *workspace,
                             size_t workspace_bytes, void *stream);
long long cpx_block_grad_layout(long long *off /* [14] or NULL */);
int cpx_blocks_backward_slab_crops(void);
size_t cpx_blocks_backward_workspace_bytes_mp(int n_subtiles, int dtype, int grad_dtype, int attn_grad_dtype);
size_t cpx_blocks_backward_workspace_bytes_ex(int n_subtiles, int dtype, int grad_dtype);
size_t cpx_blocks_backward_workspace_bytes(int n_subtiles, int dtype);
int cpx_blocks_backward_drop(const cpx_net_weights *w, const float *params, int n_subtiles, int first_block, const unsigned char *keep,
                             const void *fwd_workspace, size_t fwd_workspace_bytes, const float *dy0, int grad_dtype, int attn_grad_dtype,
                             float *grads, float *dx_all, float *dx_in, void *workspace, size_t workspace_bytes, void *stream);
int cpx_blocks_backward_in(const cpx_net_weights *w, const float *params, int n_subtiles, int first_block, const void *fwd_workspace,
                           size_t fwd_workspace_bytes, const float *dy0, int grad_dtype, int attn_grad_dtype, float *grads, float *dx_all,
                           float *dx_in, void *workspace, size_t workspace_bytes, void *stream);
int cpx_blocks_backward_mp(const cpx_net_weights *w, const float *params, int n_subtiles, int first_block, const void *fwd_workspace,
                           size_t fwd_workspace_bytes, const float *dy0, int grad_dtype, int attn_grad_dtype, float *grads, float *dx_all,
                           void *workspace, size_t workspace_bytes, void *stream);
int cpx_blocks_backward_ex(const cpx_net_weights *w, const float *params, int n_subtiles, int first_block, const void *fwd_workspace,
                           size_t fwd_workspace_bytes, const float *dy0, int grad_dtype, float *grads, float *dx_all, void *workspace,
                           size_t workspace_bytes, void *stream);
int cpx_blocks_backward(const cpx_net_weights *w, const float *params, int n_subtiles, int first_block, const void *fwd_workspace,
                        size_t fwd_workspace_bytes, const float *dy0, float *grads, float *dx_all, void *workspace,
                        size_t workspace_bytes, void *stream);
/* The weight-gradient product of the bf16 gradient mode (csrc/cpx_gemm_tn.hip): out[n][k] (+)= sum_m A[m][n] B[m][k], A [M][N] and B [M][K] bf16 row-major
 * (both operands are read transposed, by ds_read_b64_tr_b16: no transposing copy), out [N][ld_out] float32; add = 1 adds to what out
 * holds, add = 0 overwrites.  Each element is one float32 accumulation over m in order.  Requires M % 64 == 0, N % 128 == 0, K % 128 == 0
 * (all > 0), ld_out >= K, add 0 or 1, and A, B, out 16-byte aligned; anything else returns CPX_EINVAL and launches nothing.          */
int cpx_gemm_tn_bf16(const void *A, const void *B, int M, int N, int K, int add, float *out, int ld_out, void *stream);
/* db[c] += sum over rows of dy[row][c], dy [rows][N] float32: float64 partial sums in a fixed tree per column (chains over rows 4 apart,
 * four chains per 64 rows, the 64-row partials in order), added to db and rounded once.  rows % 64 == 0, N % 64 == 0; workspace of
 * cpx_colsum_workspace_bytes(rows, N) bytes (0 for an invalid shape), 8-byte aligned.                                                 */
size_t cpx_colsum_workspace_bytes(int rows, int N);
int cpx_colsum_add(const float *dy, int rows, int N, float *db, void *workspace, size_t workspace_bytes, void *stream);
size_t cpx_layernorm_backward_bytes(int rows, int C);
size_t cpx_attention_backward_workspace_bytes(int n_subtiles);
int cpx_attention_backward(int dtype, const void *qkv, const void *rel_h, const void *rel_w, const void *O, const float *dO,
                           int n_subtiles, float *dqkv, float *drel_h, float *drel_w, void *workspace, size_t workspace_bytes,
                           void *stream);
int cpx_gelu_backward(const float *pre, const float *dh, size_t n, float *dpre, void *stream);
/* The attention backward of a bf16 network on bf16 operands (csrc/cpx_attn_bwd16.hip; additive, no ABI bump).  qkv [rows][3072], rel_h,
 * rel_w [64][64] are bf16 (CPX_DT_BF16 is the only element type: there is no dtype argument), dO [rows][1024] float32; outputs float32
 * dqkv [rows][3072], drel_h, drel_w [64][64].  With q, k, v, Rh, Rw as stored (exact) and r(.) = round to nearest even to bf16, each
 * value once:
 *   S'    = q . (k + Rh[qy - ky + 31] + Rw[qx - kx + 31])    bf16 MFMA, float32 accumulation, nothing rounded
 *   P     = softmax_j(scale S')                              float32, exponent (S' - m) * scale, times 1 / l before any rounding
 *   dP    = r(dO) v^T                                        r(dO) is the only form in which dO enters anything
 *   delta = sum_j P dP                                       float32, from the unrounded P and dP (not from the stored O)
 *   dS'   = scale P (dP - delta)                             float32
 *   dv    = r(P)^T r(dO)      dk = r(dS')^T q
 *   dq    = r(dS') k + sum_ky r(G_h) Rh[..] + sum_kx r(G_w) Rw[..],   G_h, G_w = the row-group sums of the unrounded float32 dS'
 *   dRh, dRw = cpx_attention_backward's table gradients on the float32 G_h, G_w and q (float64 partials, crop order, row 63 zero)
 * Every product accumulates in float32 on v_mfma_f32_32x32x16_bf16; no floating-point atomics, no workgroup waits for another, every sum
 * in a fixed order: two runs are bitwise equal.  The workspace has cpx_attention_backward's size.  Null pointers, qkv / rel_h / rel_w /
 * dO / dqkv not 16-byte aligned, a workspace not 256-byte aligned or too short, n_subtiles outside 1 .. 16383: CPX_EINVAL, nothing is
 * launched.  The blocks' backward runs it where attn_grad_dtype is CPX_DT_BF16.                                                       */
size_t cpx_attention_backward_bf16_workspace_bytes(int n_subtiles);
int cpx_attention_backward_bf16(const void *qkv, const void *rel_h, const void *rel_w, const float *dO, int n_subtiles, float *dqkv,
                                float *drel_h, float *drel_w, void *workspace, size_t workspace_bytes, void *stream);
/* Training the patch embedding and the position table (csrc/cpx_train_embed.hip; additive, no ABI bump): with first_block 0 the last stage
 * of full fine-tuning, from the dx_in of the blocks' backward.
 * cpx_embed_grad_layout: the element count of one flat float32 record W [1024][192] | b [1024] | pos [1024][1024] (off: the three element
 * offsets); k of W in the order of pe_w / cpx_patchify_f32.
 * cpx_embed_backward: the gradients of x = round(p W^T + b + pos[row % 1024]) (the cpx_gemm(..., CPX_EPI_POS_BF16, ...) launch that opens
 * cpx_net_forward), rounding passed straight through, from patches [rows][192] in `dtype` as that GEMM read them and dx_in [rows][1024]
 * float32 (rows = n_subtiles * 1024).  The record is overwritten.
 *   dpos[t][c] = sum over the crops n, in order, of dx[n * 1024 + t][c]: one float64 chain, rounded once
 *   db[c]      = sum over the rows of the unrounded float32 dx[row][c] in float64 (the unrounded sums of dpos, tokens in order within groups
 *                of four, the groups in order), rounded once
 *   dW[c][k]   = sum over the rows of dx[row][c] p[row][k]:
 *     grad_dtype CPX_DT_F32   on the exact-float32 MFMA, p widened exactly, in slabs of two crops added in slab order (the float32 route of
 *                             the blocks' backward)
 *     grad_dtype CPX_DT_BF16  (a bf16 network only, as in cpx_blocks_backward_ex) r(dx)^T p on v_mfma_f32_32x32x16_bf16: dx rounded to bf16
 *                             once, nearest even, p exact, float32 accumulation.  The rows are split over S = 8 min(n_subtiles, 4)
 *                             workgroups per 128-channel tile (128 rows per split up to 4 crops, 32 n_subtiles beyond: 256 workgroups), each
 *                             split one accumulation chain over its rows in order; the float32 partial tiles are added in split order by a
 *                             second launch.  Both operands are read transposed from row-major LDS tiles by ds_read_b64_tr_b16.
 * Takes a stream, allocates nothing, no floating-point atomics, no workgroup waits for another; every sum runs in an order fixed by
 * n_subtiles alone: two runs are bitwise equal.  Workspace: cpx_embed_backward_workspace_bytes (2 MiB + 768 KiB per split in bf16 mode,
 * 13 MiB in float32 mode; 0 for invalid arguments).  Null pointers, patches / dx_in / grads not 16-byte aligned, a workspace not 256-byte
 * aligned or too short, n_subtiles outside the range of cpx_blocks_backward, an unknown dtype, grad_dtype CPX_DT_BF16 with a CPX_DT_F16 or
 * CPX_DT_F32 network: CPX_EINVAL, nothing is launched.                                                                                  */
long long cpx_embed_grad_layout(long long *off /* [3] or NULL */);
size_t cpx_embed_backward_workspace_bytes(int n_subtiles, int dtype, int grad_dtype);
int cpx_embed_backward(int dtype, const void *patches, const float *dx_in, int n_subtiles, int grad_dtype, float *grads, void *workspace,
                       size_t workspace_bytes, void *stream);
/* The crop moves of layer drop (csrc/cpx_train_blocks.hip; additive, no ABI bump), which the training forward runs under a mask.
 * cpx_gather_crops / cpx_scatter_crops: the 1024 rows of each crop of `crops` (HOST, n entries, strictly increasing, each < n_subtiles)
 * from a full [n_subtiles * 1024][1024] buffer of `dtype` into a compact [n * 1024][1024] one in list order, and back (the full buffer's
 * other crops untouched).  One wave per row, 16-byte accesses; the list travels by value in the kernel arguments, 64 crops per launch: no
 * device table, no allocation, nothing read after the call returns.  stats: NULL, or (half types) [n * 1024][4][2] float32 receiving the
 * row statistics of the compact rows in the same pass, bitwise cpx_row_stats of them (the same code sums both).  n = 0 launches nothing
 * and returns CPX_OK; a list that is unordered, repeats a crop or names a crop >= n_subtiles, a null or not 16-byte aligned buffer,
 * stats with CPX_DT_F32: CPX_EINVAL, nothing is launched.  src and dst are distinct buffers.                                            */
int cpx_gather_crops(int dtype, const void *src, int n_subtiles, const int *crops, int n, void *dst, float *stats, void *stream);
int cpx_scatter_crops(int dtype, const void *src, int n_subtiles, const int *crops, int n, void *dst, void *stream);

/* ------------------------------------------------------------------------
 * t2  training-time augmentation of class-head crops (csrc/cpx_augment.hip)
 * replaces augment_single_image, /root/reference/src/classpose/dataset.py:23-56: the stain jitter, cellpose's
 * random_rotate_and_resize and the normalize_img that follows them.  Every entry runs on `stream` and allocates nothing.
 * ---------------------------------------------------------------------- */
/* cpx_hed_jitter_u8: HEDTransform.transform on uint8 patches (transforms/hed.py:237-298 with separate_stains /
 *   combine_stains, :48-110).  img, out [n][H][W][3] uint8 (distinct buffers), sigma / bias [n][3] float32 (the draws of
 *   sample_sigma / sample_bias), applied [n] int32.  Image i is transformed when cutoff_lo <= (sum of its bytes / count) / 255.0
 *   <= cutoff_hi in double (the sum is an exact integer, as np.mean of uint8 is in float64), else copied unchanged.
 *   Complex mode (simple_mode 0; shift = 1 for uint8): float32(p / 255.0) + 1, -log, times float32 HED_FROM_RGB, * (1 + sigma) +
 *   bias per stain, times -RGB_FROM_HED, exp, - 1, clip to [-1, 1], the affine round trip of rescale_intensity(in_range=(-1, 1)),
 *   clip to [0, 1], (x * 255) truncated.  simple_mode 1: the input clipped to [1e-6, 1], no shift, the result clipped to [0, 1].
 *   float32 throughout with full-precision logf / expf.                                                                      */
int cpx_hed_jitter_u8(const uint8_t *img, int n, int H, int W, const float *sigma, const float *bias, double cutoff_lo,
                      double cutoff_hi, int simple_mode, uint8_t *out, int32_t *applied, void *stream);

/* cpx_warp_affine_u8 / cpx_warp_affine_f32: the cv2.warpAffine calls of cellpose's random_rotate_and_resize as called at
 *   dataset.py:42-48 (INTER_LINEAR for the image, INTER_NEAREST for the labels, constant border).  src [n][sh][sw][3] uint8 or
 *   [n][3][sh][sw] float32; labels [n][sh][sw] int16 or NULL (then labels_out is NULL too); inv [n][6] double, the INVERSE map:
 *   source (sx, sy) = (inv[0] x + inv[1] y + inv[2], inv[3] x + inv[4] y + inv[5]) of output pixel (x, y), evaluated in double
 *   left to right without fused operations.  out [n][3][dh][dw] float32 (what cpx_patchify_f32 reads), labels_out [n][dh][dw].
 *   Image: x0 = floor(sx), weight float(sx - x0), four taps, a tap outside the source counts as 0 on its own; two horizontal
 *   lerps and one vertical in float32, each a + (b - a) * w.  Labels: the source pixel (floor(sx + 0.5), floor(sy + 0.5)), or
 *   label_fill outside the source.  NOT OpenCV's scheme, which quantises source coordinates to 1/32 pixel.               */
int cpx_warp_affine_u8(const uint8_t *src, const int16_t *labels, int n, int sh, int sw, const double *inv, int dh, int dw,
                       int label_fill, float *out, int16_t *labels_out, void *stream);
int cpx_warp_affine_f32(const float *src, const int16_t *labels, int n, int sh, int sw, const double *inv, int dh, int dw,
                        int label_fill, float *out, int16_t *labels_out, void *stream);

/* cpx_normalize_stats_f32 / cpx_normalize_apply_f32: cellpose normalize_img -> normalize99 (dataset.py:55) on float32 planes
 *   img [n][3][H][W], the twins of cpx_normalize_stats_u8 / cpx_normalize_apply_u8.  Per plane the order statistics at ranks
 *   lo_prev, lo_prev + 1, hi_prev, hi_prev + 1 are found EXACTLY (radix select on order-preserving 32-bit keys, one workgroup
 *   per plane, four histogram passes through LDS, no workspace), then numpy's float32 'linear' quantile arithmetic with the
 *   host's gammas; stats [n][3][4] = {x01, x99 - x01, mode, x99}, mode 0 = constant plane (left untouched), 1 = (x - x01) /
 *   (x99 - x01), 2 = range <= 1e-3 (zeros).  NaN is out of contract; -0.0 and 0.0 compare equal.  out may be img.        */
int cpx_normalize_stats_f32(const float *img, int n, int H, int W, int lo_prev, float lo_gamma, int hi_prev, float hi_gamma,
                            float *stats, void *stream);
int cpx_normalize_apply_f32(const float *img, const float *stats, int n, int H, int W, float *out, void *stream);

/* ------------------------------------------------------------------------
 * t3  dataset statistics of (instance, class) training maps (csrc/cpx_labelstats.hip)
 * replaces the host passes behind class weights, oversampling and the rescale by cell diameter: get_class_counts and
 * get_instance_counts (classpose/train_utils.py:387-436 of the reference) and the `unique(masks, return_counts=True)` of
 * cellpose.utils.diameters (train_utils.py:256-268).  Runs on `stream`, allocates nothing, integer atomics only: every output
 * is an exact integer that does not depend on scheduling.
 * ---------------------------------------------------------------------- */
/* cpx_label_stats: inst [nI][H][W] int32 instance ids (any non-negative values, neither contiguous nor small; up to H * W
 *   distinct ones per image), cls [nI][H][W] int16 class maps, 1 <= ncls <= 64, nI <= 65535, H * W <= 2^28.
 *   class_px [nI][ncls] int64        pixels with cls == j: np.bincount of the non-negative classes (the reference drops EVERY
 *                                    negative class, not only -100, train_utils.py:401);
 *   inst_per_class [nI][ncls]        np.unique(inst[cls == j]).size (train_utils.py:435): the background id 0 counts as an id when
 *                                    it carries class j, an id that carries two classes counts in both, and pixels of a negative
 *                                    class take no part;
 *   n_masks [nI]                     m = (distinct ids of the image) - 1: cellpose.utils.diameters takes `counts[1:]` of a sorted
 *                                    unique, which drops the SMALLEST id present -- the background when there is one, else the
 *                                    smallest real cell;
 *   mid_area [nI][2]                 with the m remaining areas (pixels of an id over the whole image, whatever the class) sorted
 *                                    ascending and ranked from 0: {a[(m - 1) / 2], a[m / 2]}, {0, 0} when m == 0.  The host forms
 *                                    median(sqrt(area)) = (sqrt(a0) + sqrt(a1)) / 2 and divides by sqrt(pi) / 2 in float64;
 *   status [nI]                      bit 0: a negative id, bit 1: a class >= ncls; the image's other outputs are then void.
 *   The tables are open-addressing hash tables of a power of two >= 2 * H * W slots per image in the workspace, which therefore
 *   never fill up.  cpx_label_stats_workspace_bytes is host only and returns 0 for arguments the entry would refuse.            */
size_t cpx_label_stats_workspace_bytes(int nI, int H, int W, int ncls);
int cpx_label_stats(const int32_t *inst, const int16_t *cls, int nI, int H, int W, int ncls, int64_t *class_px,
                    int32_t *inst_per_class, int32_t *n_masks, int32_t *mid_area, int32_t *status,
                    void *workspace, size_t workspace_bytes, void *stream);

/* ------------------------------------------------------------------------
 * t4  training windows from a device-resident pool of whole annotated images of any size (csrc/cpx_augment.hip)
 * replaces what ClassposeDataset.__getitem__ -> augment_single_image (classpose/dataset.py:23-56 of the reference) does to the
 * WHOLE image of a draw: the HEDTransform call with its cut-off test on the whole image's mean (:41) and the
 * random_rotate_and_resize window (:42-48), without an upload per step or a launch per source shape.
 * Pool layout: pool_u8 holds the images back to back as [h_i][w_i][3] uint8 without padding, pool_lab int16 class maps at the same
 * pixel offsets, px_off [nI] int64 the pixel offset of image i (its bytes start at 3 * px_off[i], an odd address for many
 * sizes: nothing assumes alignment), hw [nI][2] int32 {h_i, w_i}, pool_px the pixels of the whole pool.  A table entry that does
 * not lie inside [0, pool_px) is never dereferenced: status bit 1 is set instead.  status is ONE int32 word that the entry clears
 * first.  Both entries run on `stream` and allocate nothing.
 * ---------------------------------------------------------------------- */
/* cpx_pool_byte_sums: sums [nI] uint64, the exact integer sum of the bytes of each image -- the numerator of the stain jitter's
 *   cut-off test lo <= (sum / count) / 255.0 <= hi (cpx_hed_jitter_u8), which the reference applies to the whole image.  A
 *   per-image constant: computed once per pool.  0 and status bit 1 for an entry outside the pool.                          */
int cpx_pool_byte_sums(const uint8_t *pool_u8, const int64_t *px_off, const int32_t *hw, int nI, long long pool_px,
                       uint64_t *sums, int32_t *status, void *stream);

/* cpx_warp_affine_pool_u8: crop t is cpx_warp_affine_u8 of image image_of[t] of the pool by the inverse map inv[t][6] -- the
 *   coordinates, the four taps, the three lerps and the nearest-label rule are those of cpx_warp_affine_u8, operation for
 *   operation.  out [n][3][dh][dw] float32, labels_out [n][dh][dw] int16 (NULL exactly when pool_lab is NULL).
 *   sigma / bias [n][3] float32 and applied [n] int32 (all three or none; NULL = no stain jitter) are per CROP: where
 *   applied[t] != 0 every tap INSIDE the source goes through the per-pixel function of cpx_hed_jitter_u8 (simple_mode as
 *   there) before the interpolation; a tap outside the source is 0, not jitter(0).  That is bitwise cpx_hed_jitter_u8 of the
 *   whole image followed by cpx_warp_affine_u8, at four jitter evaluations per output pixel instead of one per source pixel.
 *   An image_of[t] outside [0, nI) is never dereferenced: the crop is zeros / label_fill and status bit 0 is set.          */
int cpx_warp_affine_pool_u8(const uint8_t *pool_u8, const int16_t *pool_lab, const int64_t *px_off, const int32_t *hw, int nI,
                            long long pool_px, const int32_t *image_of, const double *inv, int n, const float *sigma,
                            const float *bias, const int32_t *applied, int simple_mode, int dh, int dw, int label_fill,
                            float *out, int16_t *labels_out, int32_t *status, void *stream);

/* ------------------------------------------------------------------------
 * t5  H&E stain-matrix perturbation (csrc/cpx_augment.hip)
 * replaces HEStainingTransform.transform -> augment_stains (classpose/transforms/he_staining.py:110-164, :195-266 of the
 * reference) as wired by StarDistAugmentation._build_color_transform (transforms/stardist_augmentation.py:48-81): the colour
 * half of the `enhanced` strategy.  The reference refits the image's two-stain basis (extract_stains, :47-107: NMF on optical
 * density) at every draw; here it is a per-image constant that the host fits once on the samples of cpx_stain_samples, and the
 * device only re-renders.  float64, unfused, left to right.  Every entry runs on `stream` and allocates nothing.
 * ---------------------------------------------------------------------- */
/* cpx_stain_samples: the rows that extract_stains hands to NMF.fit (he_staining.py:74-93), as the RGB bytes of the selected
 *   pixels (density is a function of the byte, rgb_to_density :23-27).  Pool layout as in t4.  Per image i, in raster order: the
 *   tissue pixels are those with (0.212671 * lin[R] + 0.715160 * lin[G]) + 0.072169 * lin[B] < y_t in double -- lin [256] double
 *   and y_t from the host: one threshold on linear luminance that restates `cv2.cvtColor(x, COLOR_RGB2LAB)[..., 0] < 200` (:78);
 *   k[i] int64 is their count; the values are the tissue pixels, or ALL pixels when k[i] == 0 (:83-85); with N values, N > 128
 *   keeps the values of rank 0, 128, 256, ... (`values[::128]`, :90-91), else all N.  They are written as byte triples from
 *   samples + 3 * out_off[i] on; image i needs room for max(128, ceil(h_i w_i / 128)) triples inside the out_triples of the
 *   buffer, nothing beyond what was selected is written.  status (ONE int32 word, cleared first): bit 1 a table entry outside
 *   the pool, bit 2 an output range outside the buffer; such an image is neither read nor written and its k is 0.
 *   Three launches (counts per 1024-pixel chunk by ballot, a scan per image, ranks and stores): integers only, no atomics on
 *   data, the result does not depend on the launch geometry.  workspace: cpx_stain_samples_workspace_bytes (host only; 0 for
 *   arguments the entry refuses), 8-byte aligned.                                                                            */
size_t cpx_stain_samples_workspace_bytes(int nI, long long pool_px);
int cpx_stain_samples(const uint8_t *pool_u8, const int64_t *px_off, const int32_t *hw, int nI, long long pool_px,
                      const double *lin, double y_t, const int64_t *out_off, long long out_triples, int64_t *k,
                      uint8_t *samples, int32_t *status, void *workspace, size_t workspace_bytes, void *stream);

/* cpx_he_stain_u8: augment_stains + stains_to_rgb (he_staining.py:110-164) on uint8 images of one shape, the twin of
 *   cpx_hed_jitter_u8.  img, out [n][H][W][3] uint8 (distinct buffers); params [n][14] double = Hinv [3][2] (pinv of the stain
 *   basis), M [2][3] = max(H + amount_matrix * U, 0), and the two factors 1 + amount_stains * u_j; mode [n] int32: image t is
 *   transformed where mode[t] == 2, else copied; density [256] double = max(-log(max(b, 1) / 255), 1e-6) from the host.
 *   Per pixel: d_c = density[byte_c]; s_j = max((d_0 Hinv[0][j] + d_1 Hinv[1][j] + d_2 Hinv[2][j]) * factor_j, 0);
 *   x_c = s_0 M[0][c] + s_1 M[1][c]; byte = trunc(clip(255 * exp(-x_c), 0, 255)).                                          */
int cpx_he_stain_u8(const uint8_t *img, int n, int H, int W, const double *params, const int32_t *mode, const double *density,
                    uint8_t *out, void *stream);

/* cpx_warp_affine_pool_stain_u8: cpx_warp_affine_pool_u8 with a colour transform per CROP, mode [n] int32: 0 none, 1 the
 *   stain jitter of cpx_hed_jitter_u8 with sigma / bias [n][3] (the host has already applied the cut-off), 2 the per-pixel
 *   function of cpx_he_stain_u8 with stain_params [n][14].  The transform runs on the four in-source taps of every output
 *   pixel before the interpolation; the geometry code is the one cpx_warp_affine_pool_u8 runs.  Mode 2 is bitwise
 *   cpx_he_stain_u8 of the whole image followed by cpx_warp_affine_u8; mode 1 bitwise cpx_warp_affine_pool_u8 with applied = 1,
 *   mode 0 bitwise cpx_warp_affine_pool_u8 without jitter.  status as there.  No pointer but pool_lab / labels_out is NULL. */
int cpx_warp_affine_pool_stain_u8(const uint8_t *pool_u8, const int16_t *pool_lab, const int64_t *px_off, const int32_t *hw,
                                  int nI, long long pool_px, const int32_t *image_of, const double *inv, int n,
                                  const float *sigma, const float *bias, int simple_mode, const double *stain_params,
                                  const double *density, const int32_t *mode, int dh, int dw, int label_fill, float *out,
                                  int16_t *labels_out, int32_t *status, void *stream);

/* ------------------------------------------------------------------------
 * t6  image quality: Gaussian blur and hue / brightness / saturation jitter (csrc/cpx_augment.hip)
 * replaces GaussianBlurTransform.transform (classpose/transforms/image_quality.py:41-75 of the reference) and
 * HueBrightnessSaturationTransform.transform -> _hbs_adjust (image_quality.py:173-217, :239-276), the image-quality half of the
 * `enhanced` strategy (transforms/augmentation_configs.py:28-61) as StarDistAugmentation applies it after the colour stage.
 * The host draws sigma and the three HBS values and forms the Gaussian weights; the device does everything per pixel.
 * The layout is always [H][W][3]: the reference's guess that an image with H <= 4 (blur) or H == 3 (HBS) is channel-first
 * is not reproduced.  Every entry runs on `stream` and allocates nothing.
 * ---------------------------------------------------------------------- */
/* cpx_hbs_u8: _hbs_adjust (image_quality.py:173-217) on uint8 images of one shape.  img, out [n][H][W][3] (distinct buffers);
 *   hbs [n][4] float32 = {hue, brightness, saturation, 1 - saturation (formed in double, then rounded)}; apply [n] int32: image t
 *   is transformed where apply[t] != 0, else copied; unit [256] float32 = arange(256, float32) / float32(255) from the host.
 *   float32, one rounding per operation: the hue shift (RGB -> HSV, remainder(h + hue, 1), HSV -> RGB) is skipped where
 *   hue == 0, brightness is clamp(x * brightness, 0, 1), the saturation blend clamp(fma(gray, 1 - sat, x * sat), 0, 1) with
 *   gray = fma(b, 0.114f, fma(g, 0.587f, r * 0.2989f)) is skipped where sat == 1 (torchvision's add_(other, alpha=) is a fused
 *   multiply-add in ATen), byte = trunc(clip(x * 255, 0, 255)).                                                             */
int cpx_hbs_u8(const uint8_t *img, int n, int H, int W, const float *hbs, const int32_t *apply, const float *unit,
               uint8_t *out, void *stream);

/* cpx_blur_pool_rects_u8: scipy.ndimage.gaussian_filter(plane, sigma) per channel (image_quality.py:57-73) of the
 *   colour-transformed image, restricted to a rectangle.  Pool layout as in t4.  Request j of k: image image_of[j], rectangle
 *   rects[j] = {y0, x0, h, w} inside that image (h <= max_h, w <= max_w: the launch covers max_h x max_w), radius[j] in
 *   0 .. 8 = int(4 sigma + 0.5), weights[j][17] double = phi / sum(phi), phi = exp(-0.5 / sigma^2 * x^2) for
 *   x = -radius .. radius in [0 .. 2 radius], formed on the host.  The colour stage is the one of cpx_warp_affine_pool_stain_u8
 *   with the same per-request sigma / bias [k][3], stain_params [k][14], density [256], mode [k] (0 none, 1 jitter, 2 stain
 *   perturbation).  Written: the h x w x 3 bytes of the rectangle, row-major, from scratch + scratch_off[j] on; the ranges of
 *   two requests must not overlap.  Arithmetic, exactly scipy's: rows (axis 0) first, then columns; border `reflect` about the
 *   IMAGE's borders, never the rectangle's (index m = p mod 2n, m < n ? m : 2n - 1 - m); per pass in double
 *   acc = x[c] w[r], then acc += (x[c - k] + x[c + k]) w[r - k] for k = r .. 1; the value between the passes and the result
 *   are uint8 by truncation.  One launch, a 32 x 32 tile plus halo per workgroup through LDS; no global intermediate.
 *   status (ONE int32 word, cleared first): bit 0 an image_of outside [0, nI), bit 1 a table entry outside the pool, bit 2 a
 *   rectangle that is empty, larger than max_h x max_w or not inside its image, or a radius outside 0 .. 8, bit 3 a scratch
 *   range outside [0, scratch_bytes); such a request reads and writes nothing.  No pointer is NULL.                          */
int cpx_blur_pool_rects_u8(const uint8_t *pool_u8, const int64_t *px_off, const int32_t *hw, int nI, long long pool_px,
                           const int32_t *image_of, const int32_t *rects, const int32_t *radius, const double *weights,
                           const int64_t *scratch_off, int k, int max_h, int max_w, const float *sigma, const float *bias,
                           int simple_mode, const double *stain_params, const double *density, const int32_t *mode,
                           uint8_t *scratch, long long scratch_bytes, int32_t *status, void *stream);

/* cpx_warp_affine_pool_quality_u8: cpx_warp_affine_pool_stain_u8 with two more inputs per CROP.  hbs [n][4], hbs_apply [n],
 *   unit [256] as in cpx_hbs_u8: where hbs_apply[t] != 0 every in-image tap goes through the per-pixel function of cpx_hbs_u8
 *   after the colour stage.  override_off [n] int64, override_rect [n][4] int32 {y0, x0, h, w}: where override_off[t] >= 0 the
 *   in-image taps of crop t are the bytes scratch[override_off[t] + ((y - y0) w + (x - x0)) 3 + c] (what
 *   cpx_blur_pool_rects_u8 wrote: colour stage and blur already applied) and the colour stage is skipped; a tap inside the image
 *   but outside the rectangle is 0, reads nothing and sets status bit 4; a range outside [0, scratch_bytes) sets bit 3 and the
 *   crop's image is zeros.  Taps outside the image are 0 and the labels come from the pool, as in every pool entry.  Bitwise the
 *   colour stage, the blur of the whole image, cpx_hbs_u8 of the whole image and cpx_warp_affine_u8, in that order; with no
 *   flag and no override bitwise cpx_warp_affine_pool_stain_u8.  scratch may be NULL when scratch_bytes == 0.                */
int cpx_warp_affine_pool_quality_u8(const uint8_t *pool_u8, const int16_t *pool_lab, const int64_t *px_off, const int32_t *hw,
                                    int nI, long long pool_px, const int32_t *image_of, const double *inv, int n,
                                    const float *sigma, const float *bias, int simple_mode, const double *stain_params,
                                    const double *density, const int32_t *mode, const float *hbs, const int32_t *hbs_apply,
                                    const float *unit, const uint8_t *scratch, long long scratch_bytes,
                                    const int64_t *override_off, const int32_t *override_rect, int dh, int dw, int label_fill,
                                    float *out, int16_t *labels_out, int32_t *status, void *stream);

/* ------------------------------------------------------------------------
 * t8  training the flow head `out` = nn.Conv2d(256, 192, 1) next to the class head (additive, no ABI bump)
 * The reference's `--freeze backbone neck` (paper_experiments/run_training.py:92-98, classpose/vit_sam.py:232-249): seg_trainable
 * is then true (classpose/train.py:482-489) and the total loss is seg + CE + Tversky, multiplier 1 each.  The flow head is the
 * first 192 columns of the head GEMM; cpx_head_wgrad, cpx_adamw_step and cpx_round_weights serve it unchanged.  The three entry
 * points below take a stream, allocate nothing and use no floating-point atomics.
 * cellpose.dynamics.labels_to_flows / masks_to_flows_gpu, the flow branch of cellpose.transforms.random_rotate_and_resize and
 * cellpose.train._loss_fn_seg are RESTATED here from cellpose 4.0.x and not pinned against the installed wheel (cellpose is not
 * a build dependency), as classpose_amd.augment.sample_affine already is.
 * ---------------------------------------------------------------------- */
/* cpx_masks_to_flows: masks [nT][H][W] int32 instance ids, compact in 1..n, 0 = background -> flows [nT][2][H][W] float32
 *   (dY, dX): the fp64 in-mask heat diffusion of cpx_remove_bad_flow_masks (same label statistics, centre pick, n_iter =
 *   2 * the largest extent of the tile, same launches), then the central differences mu of the result, mu / (1e-60 + |mu|),
 *   0 on the background, rounded once to float32.  workspace: cpx_postproc_workspace_bytes(nT, H, W).
 *   status is ONE int32 word that the entry clears first: an id < 0 sets CPX_MTF_BAD_ID, an id >= cpx_postproc_max_labels(H, W)
 *   sets CPX_MTF_TOO_MANY_LABELS; such pixels count as background and nothing is read or written through the id.            */
#define CPX_MTF_TOO_MANY_LABELS 1
#define CPX_MTF_BAD_ID 2
int cpx_masks_to_flows(const int32_t *masks, int nT, int H, int W, float *flows, int32_t *status, void *workspace,
                       void *stream);

/* cpx_warp_affine_pool_flow_f32: the training targets under the crop's geometry.  pool_tgt holds, for image i of the pool table
 *   (px_off, hw, pool_px as in section t4), three float32 planes [3][h_i][w_i] = (mask, flow Y, flow X) starting at float
 *   3 * px_off[i].  Crop t samples image image_of[t] by inv[t][6] with the coordinates, the four taps (0 outside the source)
 *   and the three lerps of cpx_warp_affine_f32 on all three planes; then, in float32 with every product and the sum rounded on
 *   their own (no fused multiply-add), v = (float)vec[t][.]:
 *     fy' = v[0] * fy + v[1] * fx,   fx' = v[2] * fy + v[3] * fx.
 *   The host forms vec = [cos th, f sin th, -sin th, f cos th] with f = -1 for a flipped source, +1 otherwise: cellpose negates
 *   the X flow of a flipped image and then rotates, Y' = X sin th + Y cos th, X' = X cos th - Y sin th.  The scale does not
 *   rescale the vectors and they are not renormalised.  out [n][3][dh][dw] float32 (mask, flow Y, flow X): channel 0 stays the
 *   interpolated mask.  status as cpx_warp_affine_pool_u8 (bit 0: image_of outside [0, nI); bit 1: table entry outside the pool). */
int cpx_warp_affine_pool_flow_f32(const float *pool_tgt, const int64_t *px_off, const int32_t *hw, int nI, long long pool_px,
                                  const int32_t *image_of, const double *inv, const double *vec, int n, int dh, int dw,
                                  float *out, int32_t *status, void *stream);

/* cpx_seg_loss: cellpose.train._loss_fn_seg and its gradient at the flow head's output.  head as cpx_class_loss reads it:
 *   column k*64 + i*8 + j of token (ph, pw) is channel k of pixel (8 ph + i, 8 pw + j), k = 0 dY, 1 dX, 2 cellprob (the first
 *   192 columns; later columns are not read).  targets [nI][3][H][W] float32 = (mask, flow Y, flow X).
 *     flow = mean over (b, 2, H, W) of (z - 5 t)^2 / 2
 *     cp   = mean over (b, H, W) of max(z, 0) - z y + log1p(exp(-|z|)),   y = [mask > 0.5]
 *   Every pixel counts.  Out: flow [1], cp [1] float32 and dlogits [rows][192] float32 = w_seg * d(flow + cp) / d head:
 *   w_seg (z - 5 t) / (2 nI H W) on the flow columns, w_seg (sigmoid(z) - y) / (nI H W) on the cellprob columns.
 *   One pass over the logits and a one-workgroup kernel; sums are float64, added in a fixed order.                          */
size_t cpx_seg_loss_workspace_bytes(int nI, int H, int W);
int cpx_seg_loss(const float *head, int ld_head, const float *targets, int nI, int H, int W, float w_seg, float *flow,
                 float *cp, float *dlogits, void *workspace, size_t workspace_bytes, void *stream);

/* ------------------------------------------------------------------------
 * a17  polygonisation (HOST function: all pointers are host pointers)
 * replaces, per instance, cv2.findContours(cell_mask, RETR_EXTERNAL,
 * CHAIN_APPROX_SIMPLE)[0] + shapely.Polygon(...).is_valid/.centroid/.area/.length
 * of PostProcessor.__call__, /root/reference/src/classpose/entrypoints/predict_wsi.py:601-652.
 * ---------------------------------------------------------------------- */
typedef struct cpx_cell {
    double area, perimeter, cx, cy;  /* in level-0 slide pixels (after scale + offset)   */
    int32_t n_pts, offset;           /* vertices xy_pool[offset .. offset+n_pts) (ring not closed) */
    int32_t valid;                   /* >= 4 vertices and a simple (OGC-valid) ring       */
    int32_t cls;
} cpx_cell;
/* masks_host [H][W] uint16 of ONE tile; recs_host[n] its records; vertex i of a cell is
 * (x_px * scale + off_x, y_px * scale + off_y).  Returns #vertices written (>= 0) or < 0. */
int cpx_polygonize_host(const uint16_t *masks_host, int H, int W, const cpx_record *recs_host, int n,
                        double scale, double off_x, double off_y, double *xy_pool, int max_pts,
                        cpx_cell *cells);

/* f1: the same polygonisation on the DEVICE (one thread per instance, post-processing stream), so
 * that only vertex lists and cpx_cell rows leave the GPU instead of the 2 B/pixel id maps.
 * masks_u16 [nT][H][W]; records [nT][max_rec] + rec_counts [nT] as cpx_instance_records wrote them;
 * origins [nT][2] double (level-0 x, y of each tile); cells [nT][max_rec] (rows >= rec_counts[t]
 * untouched); vertex i of a cell = (x_px * scale + origin_x, y_px * scale + origin_y) at
 * xy_pool[2 * (offset + i)], offsets are an exclusive scan in (tile, record) order; n_pts_total [1]
 * receives the pool use (cells whose vertices would pass max_pts come back with n_pts = 0).  A contour visits a
 * pixel at most twice, so max_pts = nT * 2 * H * W can never overflow (what classpose_amd.engine allocates: 16 B per
 * vertex, 16.8 MB for 8 tiles of 256 px); only n_pts_total vertices need to leave the device.
 * Precondition: hole-free instances (what cpx_fill_holes_and_remove_small_masks produces); then the
 * outputs are bit-identical to cpx_polygonize_host.                                            */
size_t cpx_polygonize_workspace_bytes(int nT, int H, int W, int max_rec);
int cpx_polygonize_device(const uint16_t *masks_u16, const cpx_record *records, const int32_t *rec_counts,
                          int nT, int H, int W, int max_rec, double scale, const double *origins,
                          double *xy_pool, int max_pts, cpx_cell *cells, int32_t *n_pts_total,
                          void *workspace, void *stream);

/* ------------------------------------------------------------------------
 * f2  cross-tile de-duplication: the fixed-radius pair search
 * replaces KDTree(centers).query_pairs(max_dist) of deduplicate,
 * /root/reference/src/classpose/entrypoints/predict_wsi.py:923-927 (scipy.spatial.KDTree, p = 2)
 * ---------------------------------------------------------------------- */
/* centers_xy [n][2] double (x, y) = the rounded centroids of every cell of the slide.  The pair set
 * {(i, j), i < j : (xi-xj)^2 + (yi-yj)^2 <= max_dist^2} (double arithmetic, products and sum unfused: exactly
 * scipy's test) via a uniform grid of edge `cell` covering [x0, x0 + grid_w*cell) x [y0, y0 + grid_h*cell).  `cell` must be
 * a power of two with cell * (1 - 2^-20) >= max_dist (anything else is refused): the bucketing is then exact enough that
 * no two points within max_dist of each other land more than one cell apart, whatever max_dist and the coordinates are.
 * Two calls on the same workspace: pairs == NULL buckets + counts (-> *n_pairs, device int64); then with
 * pairs [max_pairs][2] int32 writes them sorted by i (deterministic).  The greedy grouping of :929-960 follows
 * the iteration order of a Python set and stays on the host (classpose_amd.geojson.dedup_from_pairs).   */
size_t cpx_dedup_pairs_workspace_bytes(int n_points, int grid_w, int grid_h);
int cpx_dedup_pairs(const double *centers_xy, int n, double x0, double y0, double cell, int grid_w, int grid_h,
                    double max_dist, int32_t *pairs, long long max_pairs, long long *n_pairs,
                    void *workspace, size_t workspace_bytes, void *stream);

/* ------------------------------------------------------------------------
 * f3 / a19  the two GeoJSON FeatureCollections of a slide, streamed (host code, no HIP calls)
 * replaces json.dump({"type": "FeatureCollection", "features": [...]}) over the features of
 * to_geojson_polygon / apply_bounds_offset_to_feature / polygons_to_centroids,
 * /root/reference/src/classpose/entrypoints/predict_wsi.py:813-893,1336-1374,1772-1785.
 * Byte-identical to CPython's json encoder (", " and ": " separators, float.__repr__ numbers) except for the
 * random uuid4 ids.  cells [n_cells] rows of {double area, perimeter, cx, cy; int64 n_pts, cls} (48 B);
 * centroids_xy [n_cells][2] the centroids rounded to 2 decimals; ring i = xy_pool[2*offsets[i] .. 2*offsets[i+1])
 * (not closed; the writer repeats the first vertex); keep [n_keep] indices of the cells to write, in order;
 * class_json [n_class_json] the serialised {"name": ..., "color": [...]} object per value of cls;
 * bounds are subtracted from every coordinate when non-zero; n_threads <= 0 = one per core (max 16). */
int cpx_write_geojson(const char *contours_path, const char *centroids_path, const void *cells,
                      int64_t n_cells, const double *centroids_xy, const double *xy_pool,
                      const int64_t *offsets, const int64_t *keep, int64_t n_keep,
                      const char *const *class_json, int n_class_json, double bounds_x, double bounds_y,
                      int n_threads);
/* cpx_write_geojson plus n_extra further measurements per cell (the reference has none): after centroidY the contours
 * file's measurements list gains {"name": extra_names[e], "value": extra[i * n_extra + e]} for e = 0 .. n_extra-1, in order,
 * i the cell's index in `cells` (extra is [n_cells][n_extra]); extra_names are already JSON-encoded strings (quotes and
 * escapes included), values are written as float.__repr__.  The centroids file is the one cpx_write_geojson writes.
 * n_extra == 0 (names / extra may be NULL) is cpx_write_geojson, which forwards here.                                  */
int cpx_write_geojson_ex(const char *contours_path, const char *centroids_path, const void *cells,
                         int64_t n_cells, const double *centroids_xy, const double *xy_pool,
                         const int64_t *offsets, const int64_t *keep, int64_t n_keep,
                         const char *const *class_json, int n_class_json, double bounds_x, double bounds_y,
                         int n_threads, const char *const *extra_names, int n_extra, const double *extra);

/* cv2.findContours(mask, RETR_CCOMP, CHAIN_APPROX_SIMPLE) of the GrandQC class maps
 * (/root/reference/src/classpose/grandqc/wsi_tissue_detection.py:209-213,
 * wsi_artefact_detection.py:262-265), host code.  mask [H][W] uint8, non-zero = foreground.
 * Contour c = xy_pool[2*offsets[c] .. 2*(offsets[c]+n_pts[c])) as (x, y) int32 pairs;
 * parent[c] = -1 for outer borders, else the index of the enclosing component's outer border
 * (hierarchy[0, c, 3] of RETR_CCOMP).  Discovery (raster) order.  Returns #contours or < 0. */
int cpx_find_contours_ccomp_host(const uint8_t *mask_host, int H, int W, int32_t *xy_pool, int max_pts,
                                 int32_t *offsets, int32_t *n_pts, int32_t *parent, int max_contours);

/* ------------------------------------------------------------------------
 * r1  polygon rings -> instance-id maps: the inverse of the polygoniser (csrc/cpx_rasterize.hip)
 * replaces the host painting of annotations in paper_experiments/scripts/organise-datasets.py:626-652 of the reference
 * (`mask[..., 0][draw.polygon(g[:, 1], g[:, 0])] = i` per ring of every feature, in file order; `mask[..., 1][...] = idx_class`).
 * Runs on `stream`, allocates nothing, integer atomics only: the maps are bitwise reproducible.
 * ---------------------------------------------------------------------- */
/* cpx_rasterize_polygons: ring k = xy[ring_off[k] .. ring_off[k + 1]) as (x, y) float64 pairs in image-local pixels, painted
 *   into image ring_image[k] (NULL = image 0) of inst [n_images][H][W] int32 as inst[p] = max(inst[p], ring_value[k]) by an
 *   integer atomic max: with values that rise in feature order "the later feature wins" (the reference's painter's order) needs
 *   no ordering between workgroups.  inst is read-modify-write: clear it first, or paint onto an earlier call's map.
 *   THE RULE.  Pixel (r, c) has its centre at x = c, y = r.  A ring paints the pixel when the centre lies ON the ring (an edge or
 *   a vertex) or has an odd crossing number: even-odd rule, half-open edge test min(y0, y1) <= y < max(y0, y1).  This is the
 *   documented behaviour of skimage.draw.polygon with the boundary included, restated (not pinned against scikit-image).  A
 *   closing vertex equal to the first changes nothing; a ring with fewer than three vertices (after that) paints nothing; a ring
 *   partly or wholly outside the image is clipped to it; every ring paints, holes included, as the reference's `for g in
 *   geometry` does, so a feature is the union of its rings.  A ring with ring_value <= 0 or an image outside 0..n_images-1 is
 *   skipped.
 *   ARITHMETIC.  One orientation predicate, d = (x1 - x0) * (py - y0) - (y1 - y0) * (px - x0), in float64 without contraction
 *   and in this operand order; on the edge: d == 0 inside the edge's closed box; crossing: (y0 <= py < y1 and d > 0) or
 *   (y1 <= py < y0 and d < 0).  EXACT for vertices that are multiples of 1/16 with |coordinate| <= 32768 and H, W <= 32768: the
 *   differences are at most 2^20 sixteenths and each product stays below 2^53.  For other float64 coordinates a centre can be
 *   misclassified only where d rounds through zero.  The bounding box is clamped to the image in double before any conversion
 *   to int.  ring_off must be non-decreasing and inside xy (the caller's duty: the entry does not know the length of xy).
 *   Rings of at most 256 vertices and 4096 box pixels take one wave each, any other ring one workgroup per band of 8 rows.
 *   H, W <= 32768.  n_rings == 0 returns without a launch.  cpx_rasterize_workspace_bytes is host only and returns 0 for
 *   arguments the entry would refuse.
 * cpx_ids_to_classes: cls[p] = class_of[inst[p]] for inst[p] in 0..n_ids (class_of has n_ids + 1 entries; an id outside that
 *   range gives 0): the second channel of the reference's mask from the first.                                               */
size_t cpx_rasterize_workspace_bytes(long long n_rings, long long n_vertices, int n_images, int H, int W);
int cpx_rasterize_polygons(const double *xy, const long long *ring_off, const int *ring_value, const int *ring_image,
                           long long n_rings, int n_images, int H, int W, int *inst, void *workspace, size_t workspace_bytes,
                           void *stream);
int cpx_ids_to_classes(const int *inst, long long n_px, const unsigned char *class_of, int n_ids, unsigned char *cls,
                       void *stream);

/* ------------------------------------------------------------------------
 * r2  class or value maps -> instance maps by connected-component labelling (csrc/cpx_components.hip)
 * replaces the host labelling of semantic-only annotations: `ndimage.label` per class in
 * paper_experiments/run_cellpose_semantic.py:89-100 of the reference and `skimage.measure.label` behind
 * get_instance_counts(label_instances=True) (classpose/train_utils.py:407-436).  Runs on `stream`, allocates nothing, integer
 * atomics only: every output is an exact integer that does not depend on scheduling, so it is bitwise reproducible.
 * ---------------------------------------------------------------------- */
/* cpx_label_components: map [n][H][W] int32; 0 is background, EVERY other value is foreground, negatives included (the rule of
 *   skimage.measure.label with background 0, restated here and not pinned against scikit-image).
 *   THE RULE.  Two pixels are connected when they are neighbours and carry the same non-zero value.  connectivity 4: the edge
 *   neighbours; connectivity 8: the corner neighbours too; any other connectivity is refused.  A component is a maximal set of
 *   pixels connected through such steps.
 *   labels [n][H][W]   0 on background; on foreground the component's 1-based rank among the components of ITS image, ordered
 *                      by the raster index r * W + c of each component's first pixel -- the numbering of skimage.measure.label
 *                      and scipy.ndimage.label.  labels may not alias map.
 *   n_components [n]   the count per image (the largest label of the image).
 *   1 <= n <= 65535, H, W >= 1, H * W <= 2^28; image offsets are 64-bit.  Anything else returns non-zero and the workspace query
 *   returns 0, except that n == 0 is a successful no-op of the entry without a launch (its query still answers 0).
 *   Six launches, each a phase the next one needs complete; no workgroup ever waits for another.  Tiles of 64 x 64 pixels are
 *   labelled in LDS, the tile seams are merged by union-find on global parents with agent-scope integer atomic minima (the
 *   smaller index always becomes the parent, so a component's root is its raster-first pixel whatever the order of the unions),
 *   the roots are counted and ranked by a per-image scan in raster order.  The workspace holds one int32 parent per pixel and one
 *   count per 4096 pixels; every word read is written first, so it need not be cleared.  cpx_label_components_workspace_bytes
 *   is host only and returns 0 for arguments the entry would refuse.                                                          */
size_t cpx_label_components_workspace_bytes(int n, int H, int W);
int cpx_label_components(const int32_t *map, int n, int H, int W, int connectivity, int32_t *labels, int32_t *n_components,
                         void *workspace, size_t workspace_bytes, void *stream);

/* ------------------------------------------------------------------------
 * r3  touching cells of one class -> separate instances: distance peaks (csrc/cpx_split.hip)
 * The connected regions that r2 makes of a class map merge cells that touch.  These entries split them by a rule stated in
 * integers alone (restated on the CPU by tests/split_reference.py; NOT pinned against scikit-image's peak_local_max or
 * watershed, which is not a dependency).  They run on `stream`, allocate nothing, use integer arithmetic and integer atomics
 * only, and no workgroup ever waits for another: every output is a function of the map alone, bitwise reproducible.
 * Shapes: 1 <= n <= 65535, H, W >= 1, H * W <= 2^28 as r2, and H * H + W * W <= 2^30 so that every squared distance and every
 * sum of two of them is an int32.  Anything else returns non-zero, and the query returns 0; n == 0 is a successful no-op.
 * ---------------------------------------------------------------------- */
/* cpx_distance_sq: map [n][H][W] int32 -> d2 [n][H][W] int32 (may not alias map).  For a pixel p of value v != 0, d2[p] is the
 *   exact squared Euclidean distance to the nearest pixel of the same image whose value differs from v; 0 is a value like any
 *   other here.  The image border is not a site: a pixel whose image holds no other value gets H * H + W * W.  Pixels of value
 *   0 get 0.  workspace: n * H * W * 4 bytes (one int32 per pixel, the vertical distances g; no query of its own).
 *   Two launches.  A column sweep gives g[p], the vertical distance to the nearest other value in p's column.  Inside the
 *   horizontal run of equal value that holds p = (x, y), d2[p] = min((x - x')^2 + g(x', y)^2) over the run, capped by the squared
 *   distance to the first pixel past either run end; the scan walks outwards from x and stops once (x - x')^2 reaches the best. */
int cpx_distance_sq(const int32_t *map, int n, int H, int W, int32_t *d2, void *workspace, size_t workspace_bytes, void *stream);
/* cpx_split_touching: inst [n][H][W] int32 instance maps, 0 = background, ids 1 .. H * W (what r2 writes).
 *   SEEDS.  A pixel p of instance v is a seed when d2[p] >= min_radius^2 and no pixel q of the same instance with
 *   max(|dy|, |dx|) <= min_distance beats it; q beats p when d2[q] > d2[p], or d2[q] == d2[p] and q is earlier in raster order.
 *   The order is total, so a plateau has exactly one seed.  1 <= min_distance <= 64, 1 <= min_radius <= 32768.
 *   seeds [n][seed_cap] the raster indices y * W + x of an image's seeds, grouped by instance id in ascending order and in
 *                       raster order inside an instance; n_seeds [n] how many there are, also when they do not fit.
 *   status [n]          0, or bit 0: n_seeds > seed_cap, bit 1: an id outside 0 .. H * W.  An image with a non-zero status is
 *                       VOID: its labels are 0, its count is 0, its seed list is not written -- repeat it with seed_cap >=
 *                       n_seeds (H * W always suffices).  1 <= seed_cap <= H * W.
 *   ASSIGNMENT.  An instance with 0 or 1 seed keeps its pixels together.  Otherwise a pixel goes to the seed of its own instance
 *   with the smallest squared Euclidean distance, of equals to the one earlier in raster order: a straight bisector between two
 *   seeds, not a geodesic flood.
 *   labels [n][H][W], n_instances [n]: cpx_label_components with `connectivity` over that assignment, so the pieces of a seed's
 *   cell that are not connected become instances of their own, and the ids are the ranks of the first raster pixels.  labels
 *   may not alias inst, which is only read.
 *   Nine launches and two clears before the six of cpx_label_components.  cpx_split_workspace_bytes is host only and returns 0
 *   for arguments the entry would refuse: two int32 planes, two id tables of H * W + 1 entries, one seed list and the
 *   labeller's workspace per image.                                                                                          */
size_t cpx_split_workspace_bytes(int n, int H, int W, int seed_cap);
int cpx_split_touching(const int32_t *inst, int n, int H, int W, int min_distance, int min_radius, int connectivity,
                       int seed_cap, int32_t *labels, int32_t *n_instances, int32_t *seeds, int32_t *n_seeds, int32_t *status,
                       void *workspace, size_t workspace_bytes, void *stream);


#ifdef __cplusplus
}
#endif
#endif
