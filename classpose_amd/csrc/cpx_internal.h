// Internal (non-ABI) interfaces between the translation units of libclasspose_hip.
// Every function takes the element type explicitly: there is no process-global compute dtype,
// so engines of different precision can run from different host threads (include/classpose_hip.h,
// "thread-safe for distinct streams + distinct workspaces").
#pragma once
#include "cpx_common.h"
#include <atomic>

// hipFuncSetAttribute(MaxDynamicSharedMemorySize) once per (kernel instantiation, device), race-free
struct CpxOncePerDevice {
    std::atomic<unsigned long long> done{0};
    template <class F>
    void operator()(F &&f) {
        int dev = 0;
        (void)hipGetDevice(&dev);
        const unsigned long long bit = 1ull << (dev & 63);
        if (!(done.load(std::memory_order_acquire) & bit)) {
            f();                                            // idempotent: two racing threads set the same value
            done.fetch_or(bit, std::memory_order_release);
        }
    }
};

// optional per-launch timing (bench.py's roofline lines): HIP events on the launch stream
// around the kernels of the selected kinds.  Created by cpx_prof_create, carried in
// cpx_net_weights.prof, owned by the caller; one handle per engine / host thread.
enum { CPX_PROF_FC1 = 0, CPX_PROF_ATTN = 1, CPX_PROF_QKV = 2, CPX_PROF_PROJ = 3, CPX_PROF_FC2 = 4,
       CPX_PROF_PE = 5,        // the patch embedding (one launch per forward)
       CPX_PROF_TAIL = 6,      // neck (1x1 conv, LayerNorm2d, 3x3 conv, LayerNorm2d) + head GEMM [+ UNet head]: ONE span per forward
       CPX_PROF_KINDS = 7 };
struct CpxProf {
    hipEvent_t *ev = nullptr;      // 2 per timed launch
    int *kind = nullptr;
    int cap = 0, n = 0, stride = 1;
    int phase = 0;                 // advanced once per forward: layer l is timed when (l + phase) % stride == 0, so a
                                   // stride > 1 rotates through every layer instead of always sampling the same ones
    unsigned kinds_mask = 1;       // bit k: time kernels of kind k
};
// returns true and records the start event when this launch is to be timed
static inline bool cpx_prof_begin(CpxProf *p, int kind, int layer, hipStream_t s) {
    if (!p || !p->ev || p->n >= p->cap || !((p->kinds_mask >> kind) & 1)) return false;
    if (kind < CPX_PROF_PE && ((layer + p->phase) % p->stride) != 0) return false;      // (the once-per-forward kinds ignore the layer stride)
    p->kind[p->n] = kind;
    return hipEventRecord(p->ev[2 * p->n], s) == hipSuccess;
}
static inline void cpx_prof_end(CpxProf *p, hipStream_t s) {
    (void)hipEventRecord(p->ev[2 * p->n + 1], s);
    ++p->n;
}

// half-precision (bf16 / fp16) kernels: cpx_gemm.hip, cpx_net.hip
int cpx_gemm_half(int dtype, const void *A, const void *Wt, int M, int N, int K, int epilogue, const float *bias,
                  const void *aux, void *out, int ld_out, const float *ln_stats, const float *ln_colsum,
                  float *stats_out, void *stream);
int cpx_conv3_half(int dtype, const void *x, const void *Wt, int M, int N, int C, int epilogue, const float *bias,
                   void *out, int ld_out, void *stream);
int cpx_row_stats_half(int dtype, const void *x, int rows, float *stats, void *stream);
int cpx_gemm_half_uses_big_tile(int M, int N, int K, int epilogue);
// Crop compaction (cpx_gemm.hip, next to the row statistics it shares its sums with): up to CPX_CROP_LIST crops per launch, the list by
// value in the kernel arguments -- no device table, nothing that outlives the call.  crop[i]: the crop of the full buffer that is crop
// first + i of the compact one.  scatter 0: full src -> compact dst, with the compact rows' statistics [rows][4][2] where stats is not
// null (half types); scatter 1: compact src -> full dst.  The caller has checked every crop against the full buffer's crop count
#define CPX_CROP_LIST 64
struct CpxCropList { int n, first; int crop[CPX_CROP_LIST]; };
int cpx_move_crop_rows_run(int dtype, const void *src, void *dst, const CpxCropList &list, int scatter, float *stats, hipStream_t s);
// one-wave-per-SIMD 256^2 kernel (cpx_gemm4w.hip), bf16 / fp16: gelu(folded-LayerNorm(A) W^T + bias); 1 = launched, 0 = not this kernel's shape
int cpx_gemm4w_gelu_ln(int f16, const void *A, const void *W, int M, int N, int K, const float *bias, const float *ln_stats, const float *ln_colsum,
                       void *out, int ld_out, hipStream_t s);
int cpx_layernorm_half(int dtype, const void *x, const float *w, const float *b, int rows, int C, float eps,
                       void *out, void *stream);
int cpx_attention_half(int dtype, const void *qkv, const void *rel_h, const void *rel_w, int n_subtiles, void *vT_ws,
                       void *out, void *stream, bool transpose_v);
// production attention kernel (cpx_attn2w.hip): two query rows per wave, two workgroups per CU; vT holds V^T already
int cpx_attention2w_launch(int dtype, const void *qkv, const void *vT, const void *rel_h, const void *rel_w,
                           int n_subtiles, void *out, int xcd_order, hipStream_t s);

// float32 kernels (exact-f32 MFMA): cpx_net_f32.hip
int cpx_gemm_f32(const float *A, const float *Wt, int M, int N, int K, int epilogue, const float *bias,
                 const float *aux, float *out, int ld_out, void *stream);
int cpx_layernorm_f32(const float *x, const float *w, const float *b, int rows, int C, float eps, float *out,
                      void *stream);
int cpx_attention_f32(const float *qkv, const float *rel_h, const float *rel_w, int n_subtiles, float *out,
                      void *stream);
// the neck's im2col: x [n_subtiles * 1024][256] -> out [n_subtiles * 1024][2304], k = tap * 256 + c
int cpx_im2col3_f32(const float *x, int n_subtiles, float *out, void *stream);

// XCD-aware remap of the GEMM kernels: workgroup ids with equal (id % 8) share an XCD, so id v of nblk gets the position
// that gives each XCD one contiguous range of tiles (the first nblk % 8 XCDs one tile more)
__device__ __forceinline__ int xcd_contiguous_id(int v, int nblk) {
    const int nxcd = 8, q = nblk / nxcd, r = nblk % nxcd, x = v % nxcd;
    return (x < r ? x * (q + 1) : r * (q + 1) + (x - r) * q) + v / nxcd;
}

// returns the first non-zero status of a chain of launches from the enclosing function (or lambda)
#define CPX_RUN(call) do { const int rc_ = (call); if (rc_) return rc_; } while (0)

// the forward workspace in any dtype (cpx_net.hip): vt and st have size 0 for float32, col for the half types
struct NetWs { size_t off_x, off_xn, off_qkv, off_vt, off_ao, off_h, off_neck, off_neck2, off_st, off_col, total; };
NetWs cpx_net_ws(int nS, int dtype);
// One transformer block in w->dtype (cpx_net.hip), for cpx_net_forward and the training forward (cpx_train_blocks.hip): [LayerNorm or
// its folded form ->] qkv GEMM -> attention -> x_mid = x_in + proj -> x_out = x_mid + MLP, the MLP in row parts (cpx_net_mlp_parts).
// x_in / x_mid / x_out may be one buffer.  xn: the LayerNorm output (unfolded only); vt: V^T (half types); hb: the hidden activations;
// st: the row statistics of x_in on entry and of x_out on return (folded only), emitted by the residual GEMMs themselves when
// big_stats.  prof: the timing handle, or null
struct CpxBlockBufs { const void *x_in; void *x_mid, *x_out, *xn, *qkv, *vt, *ao, *hb; float *st; };
int cpx_net_block(const cpx_net_weights *w, int layer, int nS, const CpxBlockBufs &t, bool big_stats, CpxProf *prof, void *stream);
// do the residual GEMMs of a folded half-precision forward over nS crops emit the row statistics themselves (the 256^2 kernel)?
bool cpx_net_big_stats(const cpx_net_weights *w, int nS);
// the network tail in w->dtype (cpx_net.hip): y0 = x W0^T -> a1 = LayerNorm2d(y0) -> y2 = conv3x3(a1) -> feat = LayerNorm2d(y2) ->
// head = feat Wh^T + bh [-> UNet head over feat, in unet_ws].  y0 / y2 and a1 / feat may alias; col: float32 only, the im2col staging
int cpx_net_tail(const cpx_net_weights *w, const void *x, int nS, void *y0, void *a1, void *y2, void *feat, void *col, float *head,
                 void *unet_ws, size_t unet_ws_bytes, void *stream);

// UNet semantic head over token-major tensors of any element type (cpx_net.hip)
int cpx_unet_head_run(int dtype, const cpx_conv_op *ops, int n_ops, const void *feat, int nS, float *head, int ld_head,
                      int col0, void *workspace, size_t ws_bytes, void *stream);
size_t cpx_unet_ws_bytes(int dtype, const cpx_conv_op *ops, int n_ops, int nS);
void cpx_unet_act_layout(int dtype, const cpx_conv_op *ops, int n_ops, int nS, size_t *off, int *ld);   // n_ops <= 64

static inline size_t es_of(int dtype) { return dtype == CPX_DT_F32 ? 4 : 2; }
static inline bool dtype_ok(int dtype) { return dtype == CPX_DT_BF16 || dtype == CPX_DT_F16 || dtype == CPX_DT_F32; }
// the two predicates of the blocks' backward that the embedding's backward shares: the crop count (rows = nS * 1024 fit an int) and the
// gradient GEMMs' precision (float32 for every network, bf16 for a bf16 network alone)
static inline bool cpx_crops_ok(int nS) { return nS > 0 && (size_t)nS * 1024 < 0x7fffffffull; }
static inline bool cpx_grad_dtype_ok(int dtype, int grad_dtype) {
    return grad_dtype == CPX_DT_F32 || (grad_dtype == CPX_DT_BF16 && dtype == CPX_DT_BF16);
}
static inline int up128(long long x) { return (int)((x + 127) / 128 * 128); }
static inline int up64(int x) { return (x + 63) / 64 * 64; }
// GEMM view of a cpx_conv_op, forward and backward: out [rows_pad][Npad] = im2col(X) [rows_pad][Kpad] W^T, W [Npad][Kpad].  rows runs over
// the op's output grid ho x wo; kind 2 (convT): over its INPUT grid, Npad covers the 4 taps and depth-to-space makes 4 rows of each.
// The op's stored output (and its gradient) is [rows_out_pad][ld]
struct OpDims { int taps, ctot, Npad, Kpad, Kp128, ho, wo, ld, rows_pad, rows_out_pad; size_t rows; };
static inline OpDims op_dims(const cpx_conv_op &o, int nS) {
    OpDims d;
    d.taps = o.kind == 0 ? 9 : (o.kind == 1 ? 4 : 1);
    d.ctot = o.cin_a + o.cin_b;
    d.Npad = up128(o.kind == 2 ? 4 * o.cout : o.cout);
    d.Kpad = up64(d.taps * d.ctot);
    d.Kp128 = up128(d.Kpad);
    d.ho = o.kind == 0 ? o.h : (o.kind == 1 ? o.h / 2 : o.h * 2);
    d.wo = o.kind == 0 ? o.w : (o.kind == 1 ? o.w / 2 : o.w * 2);
    d.rows = o.kind == 2 ? (size_t)nS * o.h * o.w : (size_t)nS * d.ho * d.wo;
    d.ld = up128(o.cout);
    d.rows_pad = up128((long long)d.rows);
    d.rows_out_pad = up128((long long)nS * d.ho * d.wo);
    return d;
}
struct CpxTensor { const char *p; int ld, c, h, w; };     // a token-major tensor [nS * h * w][ld], channels 0 .. c - 1 valid

// what the training translation units (cpx_train*.hip) share
// runs the statement(s) with `DT` a compile-time constant equal to `dtype` (which the caller has checked with dtype_ok)
#define CPX_DT_DISPATCH(dtype, DT, ...)                                                   \
    do {                                                                                  \
        if ((dtype) == CPX_DT_BF16) { constexpr int DT = CPX_DT_BF16; __VA_ARGS__; }      \
        else if ((dtype) == CPX_DT_F16) { constexpr int DT = CPX_DT_F16; __VA_ARGS__; }   \
        else { constexpr int DT = CPX_DT_F32; __VA_ARGS__; }                              \
    } while (0)
// element idx of a tensor of element type DT, widened exactly to float32
template <int DT>
__device__ __forceinline__ float load_f32(const void *p, size_t idx) {
    if constexpr (DT == CPX_DT_F32) return ((const float *)p)[idx];
    else if constexpr (DT == CPX_DT_F16) return (float)((const _Float16 *)p)[idx];
    else return bf16_to_f32(((const unsigned short *)p)[idx]);
}
template <int DT>
__device__ __forceinline__ float half_bits_to_f32(unsigned u) {
    if constexpr (DT == CPX_DT_F16) { const unsigned short h = (unsigned short)u; return (float)*reinterpret_cast<const _Float16 *>(&h); }
    else return bf16_to_f32((unsigned short)u);
}
// four consecutive elements (idx a multiple of 4) of a tensor of element type DT, widened exactly
template <int DT>
__device__ __forceinline__ float4 ld4(const void *p, size_t idx) {
    if constexpr (DT == CPX_DT_F32) return *reinterpret_cast<const float4 *>((const float *)p + idx);
    else {
        const uint2 a = *reinterpret_cast<const uint2 *>((const unsigned short *)p + idx);
        return make_float4(half_bits_to_f32<DT>(a.x & 0xFFFF), half_bits_to_f32<DT>(a.x >> 16), half_bits_to_f32<DT>(a.y & 0xFFFF),
                           half_bits_to_f32<DT>(a.y >> 16));
    }
}
// the exact-float32 matrix instruction: a 32 x 32 accumulator tile, two k per issue
typedef __attribute__((ext_vector_type(16))) float f32x16;
#define MFMA_F32(a, b, c) __builtin_amdgcn_mfma_f32_32x32x2f32((a), (b), (c), 0, 0, 0)
static inline dim3 grid1(size_t n) { return dim3((unsigned)((n + 255) / 256)); }      // one thread per item, 256 per workgroup
__device__ __forceinline__ double wave_sum(double x) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) x += __shfl_xor(x, o, 64);
    return x;               // every lane holds the same bits: a + b and b + a round alike
}

// the attention backward (cpx_train_blocks.hip float32, cpx_attn_bwd16.hip bf16 operands) -- one workspace layout for both:
// m | 1 / l | delta [crops * 16 * 1024] float32, Bh | Bw | Gh | Gw [crops * 16 * 1024][32] float32, part float64
struct AttnBwdLayout { size_t off_st[3], off_b[4], off_part, total; };
static inline AttnBwdLayout cpx_attn_bwd_layout(int nS) {
    AttnBwdLayout L; CpxArena a; const size_t n = (size_t)nS * 16 * 1024;
    for (int i = 0; i < 3; ++i) L.off_st[i] = a.take(n * sizeof(float));
    for (int i = 0; i < 4; ++i) L.off_b[i] = a.take(n * 32 * sizeof(float));
    L.off_part = a.take((size_t)nS * 4 * 2 * 4096 * sizeof(double));
    L.total = a.o;
    return L;
}
// the table gradients from the row-group sums Gh, Gw of dS' (k_rel_grad, k_rel_finish); `add_rel`: on top of what drel_h / drel_w hold
int cpx_attn_rel_grad_run(int dtype, const void *qkv, const float *Gh, const float *Gw, double *part, int nS, int add_rel, float *drel_h,
                          float *drel_w, void *stream);
// cpx_attention_backward_bf16 with `add_rel` (the blocks' backward runs a batch in slabs of crops, in order)
int cpx_attention_backward_bf16_run(const void *qkv, const void *rel_h, const void *rel_w, const float *dO, int nS, float *dqkv, float *drel_h,
                                    float *drel_w, int add_rel, void *workspace, size_t workspace_bytes, void *stream);

#define UW_SLAB 512                   // rows per slab of the weight gradients (k_wgrad, k_uwgrad) = longest serial accumulation chain L

// kernels of the UNet head's backward (cpx_train_unet.hip) that the neck's backward (cpx_train_neck.hip) runs too
struct UwArgs {
    const float *dy;                   // [rows][Npad], zero beyond the valid columns
    const void *xa, *xb;               // the op's source tensors in the network dtype
    int lda, ca, ldb, cb;
    int lh, lw;                        // log2 of the INPUT height / width
    int rows, Npad, Kpad, k_valid;     // k_valid = taps * (ca + cb)
    float *part_w; double *part_b;     // [slab][Npad][Kpad], [slab][Npad]
};
struct DxArgs {
    const float *dcol; int ldc;        // [rows of the op's GEMM][Kp128]
    int kind, ctot, coff, C;           // the source's channels are columns tap * ctot + coff + [0, C) of dcol
    int lh, lw;                        // log2 of the source's (= the op's input) height / width
    size_t rows_src;
    float *gx; int ld_gx;              // the source's gradient tensor: holds the contributions of the consumers run before
    const void *y; int ld_y; int mask; // mask: this is the source's last contribution and its producer has a ReLU
};
size_t cpx_uwgrad_part_w_bytes(size_t rows, int Npad, int Kpad);       // the float32 partials; the float64 bias partials follow them
size_t cpx_uwgrad_workspace_bytes(size_t rows, int Npad, int Kpad);    // both
// dW [Npad][Kpad] = dY^T im2col(X) of a conv of `kind` (cpx_conv_op.kind) and db [Npad]: k_uwgrad over the first n_valid (rounded up to 32)
// columns of dY, then k_uwgrad_reduce
int cpx_uwgrad_run(int dtype, int kind, const UwArgs &u, int n_valid, int bias_taps, int cout, float *dW, float *db, hipStream_t s);
// W [Npad][Kpad] of `dtype` -> float32 [Kp128][Npad], rows Kpad.. zero
int cpx_wt_run(int dtype, const void *w, int Npad, int Kpad, int Kp128, float *wt, hipStream_t s);
int cpx_dx_gather_run(int dtype, const DxArgs &g, hipStream_t s);      // col2im, added to g.gx
// in [R][Cc] of `dtype` -> out [Cc][R] float32, widened exactly (cpx_train_blocks.hip); R and Cc multiples of 32
int cpx_transpose_f32_run(int dtype, const void *in, int R, int Cc, float *out, hipStream_t s);
