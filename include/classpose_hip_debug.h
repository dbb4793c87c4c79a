/*
 * classpose_hip_debug.h -- A/B, ablation and diagnostic switches.
 *
 * NOT part of the product ABI (include/classpose_hip.h) and NOT in the product library: these symbols -- and the
 * non-production kernel variants they select -- exist only in libclasspose_hip_debug.so, the same sources built with
 * -DCPX_DEBUG (csrc/Makefile).  libclasspose_hip.so exports none of them; there each switch is a compile-time constant
 * at its production value.  They are process-global test hooks used by tools/*.py and a few tests to compare kernel
 * variants in one process (classpose_amd._lib.use_debug_library() / CLASSPOSE_HIP_DEBUG=1); not thread-safe.
 */
#ifndef CLASSPOSE_HIP_DEBUG_H
#define CLASSPOSE_HIP_DEBUG_H
#ifdef __cplusplus
extern "C" {
#endif
void cpx_gemm_set_variant(int glds);        /* 128^2 GEMM: 1 LDS-DMA staging (default), 0 register staging */
void cpx_gemm_set_big(int on);              /* 1 (default): 256^2 kernel when the shape allows          */
void cpx_gemm_set_persistent(int on);       /* 1 (default): persistent 256^2 kernel with next-tile prefetch under the epilogue */
void cpx_gemm_set_persistent_qkv(int on);   /* qkv projection on the persistent kernel with a balanced q|k / V^T tile list */
void cpx_gemm_set_l2_block(int on);         /* 1 (default): 8 x 4 super-tile order per XCD, N-sweep; 2: M-sweep; 0: row-major */
void cpx_gemm_set_reverse(int on);          /* 0 (default): mlp.lin2 walks M backwards when 1            */
void cpx_gemm_set_direct(int mode);         /* 1 (default): direct-store epilogue of the persistent 256^2 kernel (accumulators -> v_permlane16_swap -> 16-byte buffer stores, no LDS staging) for the GELU epilogue; 2: also for the plain and ReLU epilogues (qkv keeps the staged rows); 0: staged rows */
void cpx_gemm_set_balanced(int on);         /* 1 (default): balanced fragment-read schedule of the persistent 256^2 main loop for the bf16 residual + row-statistics epilogue (proj, mlp.lin2); 0: plain schedule */
int cpx_gemm4w(const void *A, const void *W, int M, int N, int K, const float *bias, void *out, int ld_out, void *stream);   /* the 256^2 GEMM tile with ONE wave per SIMD (4 waves x 128 x 128, AGPR accumulators), persistent, bias epilogue, bf16 (csrc/cpx_gemm4w.hip) */
void cpx_gemm_set_4w(int on);               /* 1 (default): mlp.lin1 (bf16, folded LayerNorm + GELU) on the one-wave-per-SIMD kernel; 0: on the 8-wave persistent kernel (same bits) */
void cpx_gemm4w_set_variant(int v);         /* mlp.lin1's output stores on the one-wave-per-SIMD kernel: 0 (default) at agent scope (sc1, written through), 4096: ordinary stores (same bits); every other value acts as 0 (the timing-only ablations and abandoned store scopes that other values once selected are removed) */
void cpx_net_set_mlp_parts(int on);         /* 1 (default): the MLP of a layer in row parts of 16 384 tokens (hidden activations stay in the Infinity Cache); 0: one launch pair */
void cpx_attention_set_xcd_order(int on);   /* 1 (default): (sub-tile, head) pairs pinned to one XCD     */
void cpx_attention_set_variant(int v);      /* 2 (default): two query rows per wave, two workgroups per CU (production); 7: 4-wave, LDS-DMA ring + pipelined S (rounds 2-5, the bitwise reference); any other value: the attention entries fail with CPX_EINVAL */
void cpx_postproc_set_fused(int on);        /* 1 (default): the 23-launch fused chain of cpx_compute_masks / cpx_compute_masks_records; 0: the stage-wise sequence (39 launches) */
void cpx_gemm_set_nt(int on);               /* bits 0 / 1 / 2: non-temporal stores for the q / k / V^T thirds of the qkv projection's output (7 = default); 0: ordinary stores */
void cpx_follow_set_early_exit(int on);     /* 1 (default): Euler loop leaves when its orbit closes      */
void cpx_follow_set_lds_window(int on);     /* 1 (default): 32 x 32-cell foreground segments, the Euler loop's taps from an LDS copy of the segment's neighbourhood; 0: round 4 */
void cpx_blur_set_tile(int tile);            /* 32 (default): the product's tile of cpx_blur_pool_rects_u8; 64: the same kernel at 64 x 64 (tools/bench_train_quality.py) */
void cpx_confidence_set_footprint(int foot); /* 0 (default): a workgroup of cpx_instance_confidence covers 256 consecutive pixels; 1: a 16 x 16 block (same bits; tools/bench_cell_confidence.py) */
/* the product's bf16-only cpx_row_stats, with the half type as its first argument: CPX_DT_BF16 or CPX_DT_F16 */
int cpx_row_stats_dt(int dtype, const void *x, int rows, float *stats, void *stream);
/* the product's bf16-only cpx_gemm_ln, with the half type as its first argument: CPX_DT_BF16 or CPX_DT_F16 */
int cpx_gemm_ln_dt(int dtype, const void *A, const void *Wt, int M, int N, int K, int epilogue,
                   const float *bias, const void *aux, void *out, int ld_out,
                   const float *ln_stats, const float *ln_colsum, float *stats_out, void *stream);
/* the fp32 neck's im2col (k_im2col3_f32) on its own: x [n_subtiles*1024][256] -> out [n_subtiles*1024][9*256], k = tap*256 + c */
int cpx_im2col3_f32_debug(const float *x, int n_subtiles, float *out, void *stream);
/* where cpx_unet_head_forward leaves each op's output in its workspace (the layout helper the run itself uses): byte offset
 * and row stride in elements.  Ops 0 .. n_ops-2: the output tensor [rows_pad][ld].  The last op (the convT into the head): its
 * GEMM output before depth-to-space, [rows_in_pad][ld] with column tap*cout + co.                                            */
struct cpx_conv_op;
int cpx_unet_head_layout(const struct cpx_conv_op *ops, int n_ops, int n_subtiles, int dtype, size_t *dst_off, int *ld);
#ifdef __cplusplus
}
#endif
#endif
