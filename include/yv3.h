/*
 * yv3.h -- C-ABI of libyv3.so: the MI355X (gfx950) YOLOv3 inference hot path.
 *
 * The reference (ydixon/yolo_v3) has no FFI: its boundary is the Python module surface
 * (darknet.py / yololayer.py / utils.py).  The Python package yolo_v3_amd mirrors that
 * surface and calls ONLY the functions below (via ctypes, see yolo_v3_amd/_ffi.py).  Each
 * entry point names the reference call site it replaces (file:line in /root/reference).
 *
 * Conventions
 *   - every function returns 0 on success, a negative YV3_E* code on a bad argument, or a
 *     positive hipError_t when a launch fails;
 *   - all pointers are DEVICE pointers owned by the caller (PyTorch caching allocator) unless
 *     the name says host; nothing here allocates, frees or synchronises;
 *   - `stream` is a hipStream_t passed as void*; work is enqueued on it and nothing else;
 *   - activations are NHWC ("channels last"), fp32 (dtype 0) or bf16 (dtype 1); accumulation,
 *     BN scale/shift, decode and post-processing are always fp32;
 *   - no global mutable state: concurrent calls on distinct streams/workspaces are safe.
 */
#ifndef YV3_H
#define YV3_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define YV3_VERSION 100          /* 0.1.0 */

#define YV3_EINVAL   (-1)        /* null pointer / non-positive dimension                  */
#define YV3_ESHAPE   (-2)        /* shape not supported by the kernel family (see function) */
#define YV3_EWORKSPACE (-3)      /* workspace too small                                     */
#define YV3_EDTYPE   (-4)        /* unknown dtype code                                      */
#define YV3_ERCCL    (-5)        /* yv3_gather_boxes: librccl not found, or ncclAllGather failed */
#define YV3_ELIMIT   (-6)        /* input beyond a documented kernel limit (yv3_cocoeval)   */

/* Tensor / math modes.  "Plane" tensors are NP 16-bit planes [NP][B,H,W,C] (plane stride B*H*W*C): bf16 for NP = 1 (YV3_BF16) and
   3, fp16 for NP = 2 and for the one plane of YV3_F16.                                                                            */
#define YV3_F32  0               /* fp32 NHWC tensors, exact fp32 MFMA (v_mfma_f32_32x32x2_f32)          */
#define YV3_BF16 1               /* 1 bf16 plane, bf16 MFMA, fp32 accumulate                             */
#define YV3_F32_BF16X3 2         /* 3 bf16 planes = exact split v = p0+p1+p2 of an fp32 value; every fp32
                                    product is evaluated as its 6 leading bf16 partial products with fp32
                                    accumulation: fp32-class error at ~2.7x the fp32-MFMA rate            */
#define YV3_F32_F16X2 3          /* 2 fp16 planes hi+lo (11+11(+1 sign-carried) mantissa bits; values are
                                    saturated to +-65504, and magnitudes below 2^-14 keep an ABSOLUTE error
                                    floor of 2^-25 instead of a relative one); every fp32 product = 3 fp16
                                    MFMAs (hi*hi, hi*lo, lo*hi; the dropped lo*lo is <= 2^-22 |a*b|), fp32
                                    accumulation: ~4x fp32 epsilon per product at half the MFMA work of
                                    YV3_F32_BF16X3.  Callers should scale weights by a power of two so that
                                    max|w| is O(1) and fold the inverse into alpha (yolo_v3_amd.engine does) */

/* (code 4 is the Python side's BF16_ACT training mode: not a tensor format, YV3_EDTYPE at every entry point here) */
#define YV3_F16 5                /* 1 fp16 plane (11 significant bits, subnormals kept), v_mfma_f32_32x32x16_f16, fp32 accumulate: the
                                    kernels, tiles and selection rules of YV3_BF16 (same bytes, same matrix rate) at 1/8 of its rounding
                                    error.  Stored values are saturated to +-65504, which ORs bit 0 into *flags as for YV3_F32_F16X2;
                                    callers scale each output channel's weights to max|w| in [1,2) by a power of two and fold the
                                    inverse into alpha, as for YV3_F32_F16X2.  NOT in this mode: the Winograd forms (w_wino is ignored:
                                    a transformed operand rounded to 11 bits is another precision class), stream-K (workspace is
                                    ignored) and the four-wave 192x128 tile -- those are rules for two fp16 planes.                    */

#define YV3_I8 6                 /* int8 NHWC tensors with one fp32 scale per tensor (x ~ s * q, q in [-127, 127]; -128 is never produced),
                                    v_mfma_i32_32x32x32_i8, exact int32 accumulation (csrc/conv_planes_i8.hip).  One "plane"
                                    [1][B,H,W,C] of bytes.  Weights are int8 per output channel with the input scale(s) folded in; the
                                    epilogue is  t = fmaf((float)acc, alpha[co], beta[co]); v = max(t, 0.1 t) (YV3_ACT_LEAKY);
                                    v = fmaf((float)q_res, s_res, v) with a residual; q = clip(rint(v * inv_s_out), -127, 127).
                                    cin, cin_up and cin - cin_up must be multiples of 64, cout of 8.  out_dtype: YV3_I8, or YV3_BF16 --
                                    the same integers q written as one bf16 plane (exact), what a YV3_BF16 head conv reads.  Tiles, main
                                    loops and selection rules are YV3_BF16's, applied to the layer's BYTES (an int8 layer of C input
                                    channels is a bf16 layer of C/2); no Winograd form, no stream-K, no k3s1 / w4 variants (those
                                    options are ignored).  Batch slices (x / x2 / y_plane_stride) are YV3_ESHAPE.                        */

#define YV3_ACT_LINEAR 0
#define YV3_ACT_LEAKY  1         /* LeakyReLU(0.1), reference darknet.py:41 */

int yv3_version(void);
const char* yv3_error_string(int code);

/* ------------------------------------------------------------------------------------------
 * Weight preparation (one-off, at load time).  Replaces nothing on the reference's forward
 * path; it turns the parameters WeightManager loads (darknet.py:279-290) into kernel layout.
 * ------------------------------------------------------------------------------------------ */

/* OIHW fp32 [cout][cin][k][k]  ->  kernel layout for `dtype`; rows >= cout are 0.
 * YV3_F32: K-major [cout_pad][k][k][cin] fp32.  YV3_BF16 / YV3_F32_BF16X3: NP = 1 / 3 bf16 planes
 * pre-arranged tile by tile in the kernel's LDS image order; needs NP * cout_pad*k*k*cin * 2 bytes.  YV3_F32_F16X2 / YV3_F16: the same
 * image in 2 / 1 fp16 planes (round to nearest even).
 * YV3_I8: w_oihw holds ALREADY QUANTISED integers in [-127, 127] as fp32 (the caller quantises); they are arranged as
 * int8 in the same LDS image (64-byte rows = 64 K elements; cin a multiple of 64); needs cout_pad*k*k*cin bytes; k = 1 or 3.
 * k = 1 or 3; k = 4 (plane dtypes except YV3_F16, which has no Winograd form: YV3_ESHAPE): the 4x4 Winograd-domain filters U = G g G^T
 * of a 3x3 layer (yv3_conv_desc.w_wino). */
int yv3_pack_conv_weight(const float* w_oihw, void* w_packed, int cout, int cin, int k,
                         int cout_pad, int dtype, void* stream);

/* Eval-mode BatchNorm2d (darknet.py:39, eps=1e-5) as per-channel scale/shift:
 * alpha = gamma / sqrt(var + eps), beta = bias - mean * alpha. */
int yv3_fold_bn(const float* gamma, const float* bias, const float* mean, const float* var,
                float eps, float* alpha, float* beta, int channels, void* stream);

/* fp32 [n] <-> NP planes [NP][n] (np = 1 or 3: bf16, 3 is an exact, loss-free split; np = 2: fp16 hi+lo). Layout
 * conversion helpers for callers that hold fp32 tensors; not used inside the fused network plan. */
int yv3_split_planes(const float* in, void* out, long long n, int np, void* stream);
int yv3_merge_planes(const void* in, float* out, long long n, int np, void* stream);
/* The same for the one fp16 plane of YV3_F16 (np = 1 above is bf16): out[i] = fp16(in[i]), round to nearest even, subnormals kept,
 * saturated to +-65504 (infinities too; not reported: layout helper), NaN stays NaN; and back, exactly. */
/* YV3_I8 boundary: one bf16 plane [n] -> int8 [n], q = clip(rint(x * inv_s), -127, 127) (ties to even; NaN -> 0), inv_s = 1.0f / s
 * computed by the caller.  n a multiple of 8, both pointers 16- / 8-byte aligned. */
int yv3_quantize_bf16_i8(const void* in, void* out, long long n, float inv_s, void* stream);
int yv3_split_plane_f16(const float* in, void* out, long long n, void* stream);
int yv3_merge_plane_f16(const void* in, float* out, long long n, void* stream);

/* ------------------------------------------------------------------------------------------
 * Convolutions.  Replace conv_bn_relu.forward (darknet.py:43-44), res_layer.forward
 * (darknet.py:52-53), the plain head Conv2d (darknet.py:118) and UpsampleGroup's
 * interpolate+cat (darknet.py:161-162).
 * ------------------------------------------------------------------------------------------ */

/* First layer, feature.mlist.0: 3 -> 32 channels, 3x3, stride 1, pad 1, + BN + leaky.
 * x is the caller's NCHW fp32 image batch [B,3,H,W] (values in [0,1]); y is NHWC [B,H,W,32] in
 * out_dtype (fp32, 1 / 3 bf16 planes, 2 fp16 planes, or the one fp16 plane of YV3_F16).
 * w_tap_major is the OIHW weight permuted to [cin][kh][kw][cout] = [27][32] fp32;
 * alpha/beta from yv3_fold_bn.
 * flags (device pointer, may be NULL): YV3_F32_F16X2 runs this layer on the fp16 matrix cores with
 * inputs scaled by 2^4 and weights by 2^8; |x| > 4094 or |w| > 255 cannot be represented and OR bit 0
 * into *flags (the same sticky status word as yv3_conv_desc.flags).  YV3_BF16 and YV3_F16 compute the layer the same way and round
 * the result to one bf16 / one fp16 plane (YV3_F16: saturated to +-65504, which sets bit 0 too). */
int yv3_conv0(const float* x_nchw, const float* w_tap_major, const float* alpha, const float* beta,
              void* y_nhwc, int B, int H, int W, int out_dtype, int* flags, void* stream);

/* The first TWO layers in one launch (YV3_F32_F16X2 only): feature.mlist.0 = conv_bn_relu(3,32,3) (darknet.py:76) followed
 * by feature.mlist.1 = conv_bn_relu(32,64,3,s=2) (darknet.py:68-70), the first layer's [B,H,W,32] activation kept on chip.
 * Bit-identical to yv3_conv0(..., YV3_F32_F16X2) followed by yv3_conv2d on its output.  x_nchw as for yv3_conv0; w0 /
 * alpha0 / beta0 = the first layer's parameters as for yv3_conv0; w1_packed = the second layer's weights from
 * yv3_pack_conv_weight(cout 64, cin 32, k 3, cout_pad 64, YV3_F32_F16X2); y = 2 fp16 planes [2][B,H/2,W/2,64].
 * H and W must be multiples of 32.  flags: as yv3_conv_desc.flags. */
int yv3_conv_front(const float* x_nchw, const float* w0_tap_major, const float* alpha0, const float* beta0,
                   const void* w1_packed, const float* alpha1, const float* beta1, void* y,
                   int B, int H, int W, int* flags, void* stream);
/* The same for YV3_BF16: the first layer exactly as yv3_conv0(..., YV3_BF16) computes it (fp16 hi+lo matrix-core arithmetic, rounded
 * to bf16), w1_packed from yv3_pack_conv_weight(..., YV3_BF16), y = one bf16 plane [B,H/2,W/2,64].  Bit-identical to yv3_conv0
 * followed by yv3_conv2d in YV3_BF16. */
int yv3_conv_front_bf16(const float* x_nchw, const float* w0_tap_major, const float* alpha0, const float* beta0,
                        const void* w1_packed, const float* alpha1, const float* beta1, void* y,
                        int B, int H, int W, int* flags, void* stream);
/* The same for YV3_F16: the first layer as yv3_conv0(..., YV3_F16) computes it, w1_packed from yv3_pack_conv_weight(..., YV3_F16),
 * y = one fp16 plane [B,H/2,W/2,64].  Bit-identical to yv3_conv0 followed by yv3_conv2d in YV3_F16. */
int yv3_conv_front_f16(const float* x_nchw, const float* w0_tap_major, const float* alpha0, const float* beta0,
                       const void* w1_packed, const float* alpha1, const float* beta1, void* y,
                       int B, int H, int W, int* flags, void* stream);
/* The same for YV3_F32 (exact fp32; csrc/conv_front_f32.hip): the first layer as yv3_conv0(..., YV3_F32) computes it (one fma chain
 * per output over (c, kh, kw) on the vector ALUs), w1_packed [64][3][3][32] fp32 from yv3_pack_conv_weight(..., YV3_F32),
 * y fp32 NHWC [B,H/2,W/2,64].  Bit-identical to yv3_conv0 followed by yv3_conv2d in YV3_F32.  H, W multiples of 16 / 32. */
int yv3_conv_front_f32(const float* x_nchw, const float* w0_tap_major, const float* alpha0, const float* beta0,
                       const float* w1_packed, const float* alpha1, const float* beta1, float* y,
                       int B, int H, int W, void* stream);

/* The first residual block in one launch (YV3_F32_F16X2 only): feature.mlist.2 = res_layer(64) (darknet.py:46-53),
 * y = x + conv_bn_relu(32,64,3)(conv_bn_relu(64,32,1)(x)), the 32-channel intermediate kept on chip.  Bit-identical to the two
 * yv3_conv2d launches.  x, y: 2 fp16 planes [2][B,H,W,64] (H, W = the block's resolution, multiples of 16);
 * w1_packed / w2_packed from yv3_pack_conv_weight (cout_pad 32 / 64, YV3_F32_F16X2); alpha / beta from yv3_fold_bn (with the
 * weight scaling folded in, as for yv3_conv2d).  flags: as yv3_conv_desc.flags. */
int yv3_res_block64(const void* x, const void* w1_packed, const float* alpha1, const float* beta1,
                    const void* w2_packed, const float* alpha2, const float* beta2, void* y,
                    int B, int H, int W, int* flags, void* stream);
/* The same for YV3_BF16 (x, y: one bf16 plane [B,H,W,64]; weights from yv3_pack_conv_weight(..., YV3_BF16)); bit-identical to
 * the two yv3_conv2d launches in YV3_BF16. */
int yv3_res_block64_bf16(const void* x, const void* w1_packed, const float* alpha1, const float* beta1,
                         const void* w2_packed, const float* alpha2, const float* beta2, void* y,
                         int B, int H, int W, int* flags, void* stream);
/* The same for YV3_F16 (x, y: one fp16 plane [B,H,W,64]; weights from yv3_pack_conv_weight(..., YV3_F16)); bit-identical to the two
 * yv3_conv2d launches in YV3_F16. */
int yv3_res_block64_f16(const void* x, const void* w1_packed, const float* alpha1, const float* beta1,
                        const void* w2_packed, const float* alpha2, const float* beta2, void* y,
                        int B, int H, int W, int* flags, void* stream);
/* The same for YV3_F32 (exact fp32; csrc/conv_res64_f32.hip): x, y fp32 NHWC [B,H,W,64], H a multiple of 8, W of 16 (else
 * YV3_ESHAPE: run the two launches); w1_packed [32][64], w2_packed [64][3][3][32] from yv3_pack_conv_weight(..., YV3_F32).  Same
 * products in the same order as the two yv3_conv2d launches in YV3_F32: bit-identical to them. */
int yv3_res_block64_f32(const float* x, const float* w1_packed, const float* alpha1, const float* beta1,
                        const float* w2_packed, const float* alpha2, const float* beta2, float* y,
                        int B, int H, int W, void* stream);

typedef struct yv3_conv_desc {
    const void*  x;         /* NHWC [B,H,W,cin] -- or, when cin_up > 0, the LOW-resolution map
                               [B,H/2,W/2,cin_up] that is nearest-x2 upsampled on the fly      */
    const void*  x2;        /* cin_up > 0 only: route tail NHWC [B,H,W,cin-cin_up]; else NULL  */
    const void*  w;         /* packed weights [cout_pad][k*k*cin] (yv3_pack_conv_weight)      */
    const float* alpha;     /* [cout] scale; NULL means 1.0 (plain conv)                       */
    const float* beta;      /* [cout] shift (BN) or bias (plain conv)                          */
    const void*  residual;  /* NHWC like y, added AFTER the activation (darknet.py:53); or NULL */
    void*        y;         /* NHWC [B,Ho,Wo,cout], Ho = (H + 2*pad - k)/stride + 1             */
    int B, H, W;            /* input spatial size (of the full-resolution operand)             */
    int cin;                /* total input channels (multiple of 32)                           */
    int cin_up;             /* 0, or channels taken from the upsampled `x` (they come FIRST,
                               as torch.cat((up, route_tail), 1) in darknet.py:162); k must be 1 */
    int cout, cout_pad;     /* real and padded (multiple of 32) output channels                */
    int k, stride;          /* k in {1,3}; pad = (k-1)/2 (darknet.py:34-35); stride in {1,2}   */
    int act;                /* YV3_ACT_*                                                       */
    int dtype;              /* YV3_F32 / YV3_BF16 / YV3_F32_BF16X3 / YV3_F32_F16X2 / YV3_F16 / YV3_I8: format of x, x2, residual, w */
    int out_dtype;          /* format of y: == dtype, or YV3_F32 (head convs write fp32 logits); YV3_I8: or YV3_BF16 */
    int* flags;             /* optional device int32: bit 0 is OR-ed in when a YV3_F32_F16X2 or YV3_F16 output had to be
                               saturated (|value| > 65504), i.e. fp16 cannot represent this
                               layer -- rerun in YV3_F32_BF16X3 or YV3_F32 (YV3_F16: YV3_BF16).  NULL: not reported.
                               Bit 1: internal scheduling error (stream-K hand-over timed out).           */
    void*  workspace;       /* optional device scratch of yv3_conv_workspace_bytes() bytes, ZERO-FILLED once by
                               the caller and then left alone: enables the persistent "stream-K" schedule of the
                               YV3_F32_F16X2 kernels (every CU gets the same number of K chunks; a tile split
                               between two workgroups is finished by the first with the accumulators the second
                               left here), used for launches of fewer than two rounds of tiles.  One workspace
                               per stream: launches that may overlap must not share it.  Opt-in because a
                               split tile is summed head + tail: results stay within the parity tolerance but
                               are no longer bit-identical for the same image at different batch positions.
                               NULL: one tile per workgroup (bitwise batch-independent).                    */
    size_t workspace_bytes;
    /* Fused YOLO decode (plane dtypes with out_dtype == YV3_F32 and cout == 3*(5+C) only): when dec_out is not
       NULL the epilogue applies yv3_decode's map to the logits and writes the result to
       dec_out + b*dec_out_batch_stride + (y*W+x)*cout + channel  (exactly what yv3_decode(logits = y, out = dec_out)
       would write, bit for bit); `y` is then optional (NULL: the logits are not materialised). */
    float*    dec_out;
    long long dec_out_batch_stride;   /* floats */
    float     dec_stride;             /* input pixels per grid cell (yololayer.py:36)            */
    float     dec_anchors[6];         /* the 3 (w,h) anchor pairs of this scale, in input pixels */
    /* Kernel-selection overrides (tuning / A-B measurements; 0 = the library's defaults).  They live in the
       descriptor -- not in environment variables or other process-global state -- so concurrent callers cannot
       affect each other. */
    unsigned  options;                /* OR of YV3_OPT_*                                          */
    int       big_tile_min;           /* plane kernels: minimum number of 256x128 tiles for which that tile is
                                         used instead of 128x128 (0: default 128 = half a round of the chip) */
    int       tune[4];                /* kernel-SELECTION experiments (0 = off; tune[0..2]: every setting gives valid results of the same
                                         arithmetic).  tune[3] is IGNORED by the shipped libyv3.so: the IO ablations it selects
                                         (invalid results) exist only in measurement builds compiled with -DYV3_MEASURE */
    /* Plane strides in ELEMENTS for plane dtypes, 0 = the packed default B*H*W*C of that tensor.  They let one launch work
       on a batch SLICE of [NP][B_total,H,W,C] tensors (x / x2 / y + residual: base pointers offset by b0*H*W*C, B = slice
       size, strides = those of the full tensors): the engine runs a layer whose tiles fill between one and two rounds of the
       chip as "exactly one round" + "the rest" (bit-identical results: the K order does not depend on the tiling). */
    long long x_plane_stride, x2_plane_stride, y_plane_stride;
    /* Winograd F(2x2,3x3) path of the YV3_F32_F16X2 kernels (k = 3, stride 1, cin_up = 0, out_dtype == dtype; csrc/winograd.hip):
       when w_wino is not NULL the layer runs as  V = B^T d B (one streaming launch: 4x4 input tiles at stride 2, transformed in
       fp32, x 1/4, split hi/lo, written to wino_ws as [2][16][T][cin] fp16 planes, T = B*ceil(H/2)*ceil(W/2))  ->  sixteen
       T x cout x cin GEMMs on the matrix cores, folded on the fly into the four outputs of every tile (Y = A^T M A), same
       epilogue as the direct kernel: 2.25x fewer matrix instructions per output.  w_wino = the 4x4 transformed filters
       U = G g G^T packed with yv3_pack_conv_weight(k = 4); alpha_wino = alpha with U's per-row power-of-two scale and the
       x 4 of the input scaling folded in.  Results differ from the direct kernel by fp32 round-off only (per-layer error
       ~2x the direct scheme's, tools/winograd_numerics.py).  wino_ws: scratch of yv3_wino_workspace_bytes(B,H,W,cin) bytes,
       ZERO-FILLED once by the caller and then left alone (its tail holds the hand-over flags of the even schedule);
       launches that may overlap must not share it.  The library takes this path by the layer's count of 128x128 Winograd tiles
       (r = tiles / CUs: r >= 0.62 up to one round, r / ceil(r) >= 0.75 beyond -- measured crossovers; r >= 0.27 with
       YV3_OPT_TWO_LANES; YV3_OPT_WINO_ALWAYS: whenever w_wino is set) and the direct
       kernel otherwise -- the choice depends on B, so the same image may be computed by either form at different batch sizes
       (both within fp32 round-off of the exact result, not bit-identical to each other).  YV3_OPT_WINO_EVEN: stream-K schedule
       over transform positions (one persistent workgroup per CU; a split tile is summed head + tail). */
    const void*  w_wino;
    const float* alpha_wino;
    void*        wino_ws;
    size_t       wino_ws_bytes;
    /* Winograd F(4x4,3x3) path of the YV3_F32 kernels (k = 3, stride 1, cin_up = 0, cout % 64 == 0, cin == 64 or cin % 128 == 0; csrc/conv_wino4_f32.hip): when
       w_wino4 is not NULL the layer may run as  V = B^T d B over 6x6 input patches at stride 4 (points 0, 1, -1, 1/2, -2, inf; fp32;
       written to wino_ws as [36][T][cin], T = B*ceil(H/4)*ceil(W/4): yv3_wino4_workspace_bytes)  ->  thirty-six T x cout x cin GEMMs on
       v_mfma_f32_16x16x4_f32, folded on the fly into the sixteen outputs of every tile: 4x fewer matrix instructions than the direct
       form, 1.78x fewer than F(2x2,3x3).  w_wino4 = yv3_pack_wino4_weight_f32 of U = G g G^T; scale / shift = alpha / beta.  Results
       differ from the direct kernel by fp32 round-off (whole network: within 1.4x of the direct form's distance from an fp64
       evaluation on hostile data, equal on the headline data -- tools/winograd_f32_gate.py).  The library takes this form when its
       64-channel x 32-tile workgroups fill the chip (yv3_conv2d_form == YV3_FORM_WINOGRAD4), else F(2x2) by w_wino's rule, else the
       direct kernel.  Schedule: one (32 tiles x 64 channels) item per workgroup while the items fill whole rounds of the chip (two
       workgroups per CU); the items of a last, partial round are dealt out by patch row over all the slots -- an item split between
       workgroups of one XCD is summed part by part in workgroup order through the hand-over area at the END of wino_ws (the last
       yv3_wino4_workspace_bytes - V bytes: ZERO-FILLED once by the caller, then left alone; one wino_ws per stream).  Which items are
       split depends on B: the same image is then summed in a different (fixed per shape) order at different batch sizes / positions;
       YV3_OPT_WINO4_TILES keeps one item per workgroup.  A hand-over that times out sets bit 1 of *flags. */
    const void*  w_wino4;
    /* YV3_I8 only (ignored by every other dtype): the residual tensor's scale and 1.0f / (the output tensor's scale), computed once on the
       host; alpha / beta hold the layer's per-channel multiplier m = sw * alpha_bn and shift b. */
    float        s_res, inv_s_out;
} yv3_conv_desc;

#define YV3_OPT_NO_PINGPONG 1u    /* fp16-plane 8-wave tiles: single-phase main loop instead of the two-group ping-pong */
#define YV3_OPT_K3S1        2u    /* 3x3 stride-1 plane convs: the kw-tap-reuse kernel (conv_planes_k3s1.hip)          */
#define YV3_OPT_WINO_EVEN   4u    /* Winograd stage: even (stream-K over transform positions) schedule instead of one tile per workgroup */
#define YV3_OPT_WINO_ALWAYS 8u    /* Winograd stage whenever w_wino is set, whatever the tile count                                     */
#define YV3_OPT_TWO_LANES   16u   /* the caller runs an equal launch sequence on a second stream at the same time (two lanes of one batch):
                                     the Winograd rule's lower bound counts both lanes' tiles (0.27 instead of 0.55 rounds per launch)  */
#define YV3_OPT_WINO4_TILES 32u   /* F(4x4,3x3) stage: one item per workgroup only -- no even schedule (whose ranges wait for their partner
                                     workgroups: callers that share the GPU with other work; results then do not depend on the batch size) */
#define YV3_OPT_TILE_SHIFT  8     /* bits 8..15: force a tile configuration of the fp16-plane kernels (0 = automatic):
                                     1 = 256x128 / 8 waves, 2 = 128x128 / 8 waves, 3 = 128x128 / 4 waves, two workgroups per CU */

/* Size of yv3_conv_desc.workspace. */
size_t yv3_conv_workspace_bytes(void);

/* Size of yv3_conv_desc.wino_ws for a B x H x W x cin input (YV3_F32_F16X2). */
size_t yv3_wino_workspace_bytes(int B, int H, int W, int cin);

/* Size of yv3_conv_desc.wino_ws that the F(4x4,3x3) form of a YV3_F32 layer needs: V + the hand-over area (never more than
 * yv3_wino_workspace_bytes for H, W >= 4).  U [cout][cin][6][6] fp32 = G g G^T (points 0, 1, -1, 1/2, -2, inf; computed by the caller, in fp64 and rounded once)
 * -> the GEMM stage's packed image of cout*cin*36 floats; cout % 64 == 0, cin == 64 or a multiple of 128. */
size_t yv3_wino4_workspace_bytes(int B, int H, int W, int cin);
int yv3_pack_wino4_weight_f32(const float* u_oc66, float* packed, int cout, int cin, void* stream);

/* y = act(conv(x) * alpha + beta) (+ residual), implicit GEMM on the MFMA units. */
int yv3_conv2d(const yv3_conv_desc* desc, void* stream);

/* Which form would yv3_conv2d run for this descriptor ON THE CURRENT DEVICE (the per-launch rule depends on the CU count)?
 * YV3_FORM_DIRECT (0): the direct implicit-GEMM kernel (36 multiplications per 2x2 outputs and channel pair for a 3x3 layer);
 * YV3_FORM_WINOGRAD (1): input transform + 16-position GEMM (16 per 2x2 outputs: 2.25x fewer matrix instructions).
 * Negative: the YV3_E* code yv3_conv2d would return for it.  Launches nothing; used by tests (assert which plan ran) and by
 * bench.py (executed vs algorithmic FLOPs). */
#define YV3_FORM_DIRECT   0
#define YV3_FORM_WINOGRAD 1
#define YV3_FORM_WINOGRAD4 2     /* YV3_F32: F(4x4,3x3), 36 multiplications per 4x4 outputs and channel pair (4x fewer than direct) */
int yv3_conv2d_form(const yv3_conv_desc* desc);

/* How many kernels does yv3_conv2d launch for this descriptor on the current device?  1; 2 for the Winograd forms (input transform + GEMM
 * stage) and for a YV3_F32 1x1 layer whose whole rounds of tiles run on the persistent GEMM (csrc/conv_gemm_f32.hip) and the rest on the
 * small tiles.  Negative: the YV3_E* code yv3_conv2d would return.  Launches nothing; profiling tools use it to map a kernel trace to layers. */
int yv3_conv2d_launches(const yv3_conv_desc* desc);

/* Which kernel would yv3_conv2d run for this descriptor on the current device?  Writes one NUL-terminated line of at most 96 bytes into buf:
 * the kernel instantiation's name and every part of the library's choice that is not a function of the descriptor alone -- channel tiles;
 * plane modes: main loop, stream-K, persistent grid; YV3_F32: pin, the F(2x2) half tile, the F(4x4) schedule, the persistent GEMM's rows
 * and grid, the kernel and tiles of the rest.  Returns 0, the YV3_E* code yv3_conv2d would return, or YV3_EINVAL when buf_bytes is too
 * small.  Launches nothing; tests pin the selection rules with it.  The text is for people and tables, not a stable format. */
int yv3_conv2d_kernel(const yv3_conv_desc* desc, char* buf, size_t buf_bytes);

/* Run `n` convolutions back to back on `stream` (one host call for a whole network plan). */
int yv3_conv2d_sequence(const yv3_conv_desc* descs, int n, void* stream);

/* ------------------------------------------------------------------------------------------
 * YOLO head decode.  Replaces YoloLayer.forward, inference branch (yololayer.py:31-59,97-105).
 *   bx=(sigmoid(tx)+gx)*stride  by=(sigmoid(ty)+gy)*stride
 *   bw=exp(tw)*(aw/stride)*stride  bh likewise   conf=sigmoid(to)  cls_k=sigmoid(t_k)
 * out row = (y*W + x)*3 + a (yololayer.py:104); columns cx,cy,w,h,conf,cls0..
 * ------------------------------------------------------------------------------------------ */

/* logits NHWC [B,H,W,3*(5+C)] with row pitch `ld_logits` floats per pixel (>= 3*(5+C)).
 * out[b] starts at out + b*out_batch_stride (floats) and holds H*W*3 rows of (5+C) floats:
 * pass out = base + row_offset*(5+C) to write one scale into a concatenated [B,N,5+C] tensor.
 * anchors: 3 (w,h) pairs in input pixels (host pointer, copied by value). */
int yv3_decode(const float* logits, int ld_logits, const float* anchors_host, float stride,
               float* out, long long out_batch_stride, int B, int H, int W, int num_class,
               void* stream);

/* Same, reading the reference's NCHW layout [B,3*(5+C),H,W] (channel = a*(5+C)+attr,
 * yololayer.py:42) -- the drop-in YoloLayer.forward(x) entry. */
int yv3_decode_nchw(const float* logits_nchw, const float* anchors_host, float stride,
                    float* out, long long out_batch_stride, int B, int H, int W, int num_class,
                    void* stream);

/* dlogits (NCHW, as logits_nchw) = dL/dlogits of yv3_decode_nchw for dout = dL/dout ([B][H*W*3][5+C], contiguous): per element
 * dout times the decode map's derivative, recomputed from the logit -- stride s(1-s) for tx and ty, the decoded w and h for tw and
 * th, s(1-s) for conf and every class (s = sigmoid). */
int yv3_decode_bwd_nchw(const float* logits_nchw, const float* dout, const float* anchors_host, float stride,
                        float* dlogits_nchw, int B, int H, int W, int num_class, void* stream);

/* ------------------------------------------------------------------------------------------
 * Geometry helpers.  Replace boundingbox.py:25-29, utils.py:98-119, utils.py:122-146.
 * ------------------------------------------------------------------------------------------ */

/* boxes [n,4] cxcywh -> x1y1x2y2 (in place allowed: out may equal in). */
int yv3_cxcywh_to_xyxy(const float* in, float* out, long long n, void* stream);

/* out[n1,n2] = IOU(b1[i], b2[j]); boxes have `ld` floats per row (>= 4);
 * mode 0 = x1y1x2y2, 1 = cxcywh.  No +1, no epsilon: 0/0 gives NaN like the reference. */
int yv3_iou_matrix(const float* b1, int n1, int ld1, const float* b2, int n2, int ld2,
                   int mode, float* out, void* stream);

/* ------------------------------------------------------------------------------------------
 * Post-processing.  Replaces utils.postprocessing (utils.py:226-258) with
 * get_nms_detections (utils.py:148-202) / get_raw_detections (utils.py:204-224).
 *
 * Two calls so that the caller can size buffers from the candidate counts if it wants to:
 *   1. yv3_postproc_filter : score = cls*conf, confidence filter, candidate compaction
 *   2. yv3_postproc_nms    : order by (class asc, score desc, row asc), IOU bit masks,
 *                            greedy scan, compaction into [B,cap,7]
 * ------------------------------------------------------------------------------------------ */

/* Bytes of candidate storage for up to `max_cand` candidates per image. */
size_t yv3_postproc_cand_bytes(int B, int max_cand, int num_class);

/* Bytes of scratch yv3_postproc_nms needs for up to `max_n` candidates per image. */
size_t yv3_postproc_nms_workspace_bytes(int B, int max_n, int num_class);

#define YV3_PP_EVAL 1   /* is_eval=True: every (row,k) with cls_k*conf > thr (utils.py:238)          */
#define YV3_PP_PROB 2   /* caller guarantees 0 <= cls_k <= 1 (sigmoid outputs): rows with conf <= thr
                           cannot pass and are skipped unread.  Same result, ~5x less traffic.      */

/* dets: decoded detections [B,N,5+C] (cx,cy,w,h,conf,cls..), row pitch 5+C, NOT modified.
 * mode: OR of YV3_PP_*.  Without YV3_PP_EVAL: one candidate per row whose max_k(cls_k*conf) > thr,
 * class = first argmax (utils.py:242-246).
 * cand: opaque buffer of yv3_postproc_cand_bytes(B,max_cand,C); cand_counts [B] int32 receives
 * the number of candidates found per image (may exceed max_cand: then the excess was dropped
 * and the caller must retry with a larger buffer). */
int yv3_postproc_filter(const float* dets, int B, int N, int num_class, float conf_thr,
                        int mode, void* cand, int max_cand, int* cand_counts, void* stream);

/* max_n: upper bound on candidates per image that is actually processed (<= max_cand; images
 * with more candidates are truncated).  It sizes the workspace, so a caller that has read
 * cand_counts back can pass max(cand_counts); a sync-free caller passes max_cand.
 * out_boxes [B,cap,7] = x1,y1,x2,y2,conf,score,cls per kept box, ordered by class ascending then
 * score descending (utils.py:161-172,193-199); out_counts [B] = number kept (may exceed cap: rows
 * beyond cap are dropped).  use_nms = 0 reproduces get_raw_detections: every candidate, row order.
 * Zero-area / inverted boxes are dropped and never suppress (self-IOU not > thr, utils.py:182). */
int yv3_postproc_nms(const float* dets, int B, int N, int num_class, float nms_thr, int use_nms,
                     const void* cand, int max_cand, const int* cand_counts, int max_n,
                     float* out_boxes, int cap, int* out_counts,
                     void* workspace, size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------
 * Neighbours of the hot path: input preparation and box un-mapping.
 * ------------------------------------------------------------------------------------------ */

/* Replaces utils.letterbox_image + the /255, HWC->CHW of utils.load_image (utils.py:44-72):
 * img_hwc uint8 RGB [H,W,3] (device) -> out_chw fp32 [3,out_h,out_w] in [0,1]: cv2.resize(INTER_CUBIC) -- OpenCV's
 * fixed-point 8-bit path: A=-0.75 coefficients as 11-bit shorts, int32 horizontal pass, (sum + 2^21) >> 22 vertical
 * pass, no antialias -- to box = int(size*min(out_w/W,out_h/H)), centred (offset out/2 - box/2, utils.py:34-42) on
 * a 128-grey canvas.  Pass out_chw = batch + b*3*out_h*out_w.
 * PARITY WITH cv2 IS UNPINNED: cv2 is absent from the build image, so the kernel is checked bit for bit against a
 * restatement of OpenCV's scalar fixed-point path (oracle_cpu.cv_resize_cubic_u8), not against cv2 output.  SIMD builds
 * of OpenCV run the vertical cubic pass in float32 (VResizeCubicVec_32s8u) and can differ from the scalar formula by
 * 1 LSB on ~1e-4 of the pixels: expect agreement with a given cv2 build to within 1 LSB (1/255 of the input), unverified. */
int yv3_letterbox(const unsigned char* img_hwc, int H, int W, float* out_chw, int out_h, int out_w,
                  void* stream);

/* The same resampling with the box geometry GIVEN (box_w x box_h pixels of the resized image at (box_x, box_y) on the 128-grey
 * canvas): the evaluation pipeline's letterbox (transforms.py:144-209, IaaLetterbox: box at ((out_w-box_w)//2, (out_h-box_h)//2) --
 * one pixel off utils.letterbox_transforms' out//2 - box//2 when the parities differ) and its plain `iaa.Scale(dim)` (evaluate.py:213:
 * box == canvas, bicubic).  Same cv2 caveat as yv3_letterbox.  YV3_ESHAPE if the box does not fit the canvas. */
int yv3_letterbox_ex(const unsigned char* img_hwc, int H, int W, float* out_chw, int out_h, int out_w,
                     int box_w, int box_h, int box_x, int box_y, void* stream);

/* Replaces load_image(mode='resize') (utils.py:68-71): cv2.resize(img, (out_w,out_h)) with the default INTER_LINEAR
 * (OpenCV's fixed-point 8-bit path; an exact 2x2 shrink is INTER_AREA, as in cv::resize), /255, HWC -> CHW. */
int yv3_resize_linear(const unsigned char* img_hwc, int H, int W, float* out_chw, int out_h, int out_w,
                      void* stream);

/* Replaces boundingbox.correct_yolo_boxes (boundingbox.py:139-149) = letterbox_reverse (:95-116) or
 * rescale_bbox (:119-137) followed by x1y1x2y2 -> xywh.  boxes [B][cap][ld] with x1,y1,x2,y2 in the
 * first four columns (e.g. the [B,cap,7] output of yv3_postproc_nms, ld = 7); counts [B] valid rows per
 * image (NULL: all cap rows); org_wh [B][2] int32 original (width,height) per image (device).
 * out [B][cap][4] in original-image pixels, clipped to the image like the reference: x,y,w,h
 * (out_xyxy = 0, what correct_yolo_boxes returns) or the intermediate x1,y1,x2,y2 (out_xyxy = 1,
 * what letterbox_reverse / rescale_bbox return). */
int yv3_correct_boxes(const float* boxes, int B, int cap, int ld, const int* counts, const int* org_wh,
                      int img_w, int img_h, int is_letterbox, int out_xyxy, float* out, void* stream);

/* ------------------------------------------------------------------------------------------
 * Training augmentation (reference transforms.py + custom_data_train.ipynb getTransforms(aug=True), csrc/augment.hip):
 *   Compose([IaaAugmentations([iaa_hsv_aug(h, s, e), iaa_random_crop(j), iaa.Fliplr(0.5), IaaLetterbox(dim)]), ToTensor()])
 * for B images in one call.  params [B][8] float64 = dhue, dsat, dexp, top, right, bottom, left, flip: the colour draws (read as
 * float32 by the pixel pass), the signed CropAndPad side counts (positive pads with 128, negative crops; whole numbers) and the
 * flip (0 or 1).  hw [B][2] int32 = source (H, W).  Per image, the checks a host cannot make without a synchronisation are made
 * on the device, and each call writes status[b] for every image: 0, YV3_EINVAL (H or W <= 0, a source outside src_bytes, a
 * non-finite parameter, dsat or dexp < 0, a fractional side, flip not 0 / 1) or YV3_ESHAPE (a crop leaves H1 = H + top + bottom
 * or W1 = W + left + right below 1, or the letterboxed box has no pixel); such an image's outputs are zeros.  The return value
 * covers the host arguments (YV3_EINVAL: null pointer, non-positive size; YV3_EWORKSPACE).  Nothing allocates or synchronises.
 * Same cv2 caveat as yv3_letterbox (the resampling is the same fixed-point INTER_CUBIC).
 * ------------------------------------------------------------------------------------------ */

/* Bytes of workspace yv3_augment_images needs for src_bytes of packed sources (the colour-jittered copy; 0 if src_bytes <= 0). */
size_t yv3_augment_workspace_bytes(long long src_bytes);

/* Pixels, two launches.  src: packed uint8 RGB sources, image b = H*W*3 bytes at src + offsets[b] (int64, no alignment needed).
 * out: fp32 [B][3][out_h][out_w] in [0,1].  workspace: >= yv3_augment_workspace_bytes(src_bytes) device bytes. */
int yv3_augment_images(const unsigned char* src, long long src_bytes, const long long* offsets, const int* hw,
                       const double* params, int B, float* out, int out_h, int out_w,
                       void* workspace, size_t workspace_bytes, int* status, void* stream);

/* As yv3_augment_images, with the sources gathered from a larger allocation: image b is read at src + src_offsets[b] (checked
 * against src_bytes) and its colour copy lives at workspace + ws_offsets[b] (checked against ws_span <= workspace_bytes).  The
 * same source may occur more than once in a batch; the ws ranges of a batch must not overlap (the caller's duty).  src is not
 * written.  status[b] = YV3_EINVAL for either range out of bounds, outputs zeros, as today.  All offsets are int64 bytes and need
 * no alignment; the workspace a batch needs is its own images' bytes, whatever the size of the allocation they are read from. */
int yv3_augment_images_from(const unsigned char* src, long long src_bytes, const long long* src_offsets,
                            const long long* ws_offsets, long long ws_span, const int* hw, const double* params, int B,
                            float* out, int out_h, int out_w, void* workspace, size_t workspace_bytes, int* status, void* stream);

/* Labels, one launch, float64 arithmetic.  labels [B][T][5] float64 rows (cls, cx, cy, w, h) relative to the source (NULL when
 * T == 0); rows with w or h <= 0 (zero padding among them) are dropped, as label_np_to_bbs drops them.  target: fp32
 * [B][max_rows][5], the first max_rows kept rows (cls, cx, cy, w, h relative to out_w x out_h) in input order, zero-filled. */
int yv3_augment_labels(const double* labels, int B, int T, const int* hw, const double* params,
                       float* target, int max_rows, int out_h, int out_w, int* status, void* stream);

/* ------------------------------------------------------------------------------------------
 * The reference's ExtraAugmentations (transforms.py:292-329; csrc/extra_augment.hip) for B packed uint8 RGB images of any
 * sizes: one program of at most YV3_EXTRA_MAX_STEPS steps per image, every step on the whole output of the step before,
 * per channel, uint8 -> uint8.  The operations (tests/extra_aug_ref.py is their definition; v = the step's v[0..2]):
 *   YV3_EXTRA_GAUSS     scipy.ndimage.gaussian_filter(sigma = v[0]) on uint8: radius r = int(4 sigma + 0.5) <= 12, the program's
 *                       float64 gauss_w[0 .. 2r] (computed by the caller: exp(-0.5 / sigma^2 x^2), normalised), border reflect, rows
 *                       then columns, each pass truncated to uint8; r == 0 leaves the image as it is
 *   YV3_EXTRA_AVERAGE   cv2.blur, k in 2..7, anchor k / 2, border reflect-101, rint(float64(sum) * (1.0 / (k k)))
 *   YV3_EXTRA_MEDIAN    odd k in 3..11, the middle of the k x k window, border replicated
 *   YV3_EXTRA_SHARPEN   3x3 float32 kernel (1 - alpha) I + alpha [-1 .. 8 + lightness .. -1], alpha = v[0], lightness = v[1],
 *                       border reflect-101, float32 sums in row-major tap order, rint, clip
 *   YV3_EXTRA_NOISE     trunc(clip(p + v[0] * z)), z from Philox4x32-10 under `key` (counter = the pixel index y W + x, or that
 *                       times 3 plus the channel when per_channel is 1) and Box-Muller in float64
 *   YV3_EXTRA_ADD       clip(p + (int)v[c]), whole numbers in -255..255
 *   YV3_EXTRA_MUL       trunc(clip(float32(p) * float32(v[c])))
 *   YV3_EXTRA_CONTRAST  trunc(clip(float32(v[c]) * (float32(p) - 128) + 128))
 * A program holds one weight table, used by each of its GAUSS steps with r > 0 (which therefore share one sigma; the kernels can
 * only check r == gauss_radius).  The kernels check every
 * image themselves and write status[b]: 0, or YV3_EINVAL (H or W <= 0, a range outside its buffer, n_steps outside 0..6, an
 * unknown opcode, k out of range or even for the median, a non-finite value, a negative sigma or scale, r > 12, r != gauss_radius,
 * weights that are not finite or not symmetric, per_channel not 0 / 1, a fractional ADD value); such an image is copied through
 * unchanged (nothing is written for one whose ranges are out of bounds).  The return value covers the host arguments (YV3_EINVAL,
 * YV3_EWORKSPACE), checked before any launch.  No allocation, no synchronisation, no atomics: identical calls give identical bits.
 * ------------------------------------------------------------------------------------------ */
#define YV3_EXTRA_MAX_STEPS 6
#define YV3_EXTRA_MAX_RADIUS 12
enum { YV3_EXTRA_GAUSS = 1, YV3_EXTRA_AVERAGE = 2, YV3_EXTRA_MEDIAN = 3, YV3_EXTRA_SHARPEN = 4, YV3_EXTRA_NOISE = 5,
       YV3_EXTRA_ADD = 6, YV3_EXTRA_MUL = 7, YV3_EXTRA_CONTRAST = 8 };

typedef struct yv3_extra_step {
    int op;                      /* YV3_EXTRA_*                                                   */
    int k;                       /* AVERAGE, MEDIAN: the window's side                            */
    int per_channel;             /* NOISE: 0 = one draw per pixel, 1 = one per byte               */
    int reserved;
    double v[3];                 /* the operation's values (see above)                            */
    unsigned long long key;      /* NOISE: the Philox key                                         */
} yv3_extra_step;                /* 48 bytes */

typedef struct yv3_extra_program {
    int n_steps;                 /* 0 .. YV3_EXTRA_MAX_STEPS                                      */
    int gauss_radius;            /* the radius gauss_w was computed for (0: no table)             */
    yv3_extra_step steps[YV3_EXTRA_MAX_STEPS];
    double gauss_w[2 * YV3_EXTRA_MAX_RADIUS + 1];
} yv3_extra_program;             /* 496 bytes */

/* Bytes of workspace yv3_extra_augment needs for a batch whose packed outputs take out_bytes (0 if out_bytes <= 0). */
size_t yv3_extra_augment_workspace_bytes(long long out_bytes);

/* Six launches (one per program slot).  Image b = hw[2b] x hw[2b+1] x 3 bytes, read at src + src_offsets[b] (inside src_bytes:
 * src may be a packed batch or a larger allocation the images are gathered from; it is not written) and written at
 * out + out_offsets[b] (inside out_bytes); its intermediate results live at workspace + out_offsets[b].  The out ranges of a
 * batch must not overlap each other or the sources (the caller's duty).  All offsets are int64 bytes and need no alignment.
 * programs: yv3_extra_program[B] in device memory.  workspace: >= yv3_extra_augment_workspace_bytes(out_bytes). */
int yv3_extra_augment(const unsigned char* src, long long src_bytes, const long long* src_offsets, const int* hw,
                      const void* programs, int B, unsigned char* out, long long out_bytes, const long long* out_offsets,
                      void* workspace, size_t workspace_bytes, int* status, void* stream);

/* ------------------------------------------------------------------------------------------
 * Affine training augmentation: rotate, scale, shear, shift (csrc/affine_augment.hip) for B packed uint8 RGB images of any
 * sizes, one program per image; the output has the source's size.  tests/affine_aug_ref.py is the definition.  A program holds
 * two 2x3 float64 matrices in continuous pixel coordinates (pixel (x, y) covers [x, x+1) x [y, y+1)), both computed by the
 * caller: fwd maps source to output and moves the labels, inv (its inverse) maps output to source and fetches the pixels.
 *   pixels   Pillow's Image.transform(size, AFFINE, inv, BILINEAR, fillcolor 128) on RGB, float64 without fused multiply-add:
 *            xin = inv0 (x + 0.5) + inv1 (y + 0.5) + inv2 (yin from inv3..5); (128, 128, 128) unless 0 <= xin < W and
 *            0 <= yin < H; otherwise, after xin -= 0.5, yin -= 0.5: x0 = floor(xin), dx = xin - x0 (y likewise), columns x0 and
 *            x0 + 1 and row y0 clamped to the image, v1 = p[y0][x0] + (p[y0][x1] - p[y0][x0]) dx, v2 the same on row y0 + 1
 *            (v2 = v1 when that row is outside), the byte is trunc(v1 + (v2 - v1) dy)
 *   labels   rows (cls, cx, cy, w, h) relative to the source, float64: a row with w <= 0 or h <= 0 becomes zeros; otherwise its
 *            absolute corners through fwd, the axis-aligned hull of the four, clipped to [0, W - eps] x [0, H - eps] (eps =
 *            float32's), kept iff clipped area / hull area > 0.1 (bbs_remove_cut_out; a hull area <= 0 drops it) and written
 *            back relative, in place; a dropped row is zeros (yv3_augment_labels drops zero rows and keeps order)
 * active == 0 (the augmentation did not fire for this image): the image is copied, its rows are passed through untouched.
 * The kernels check every image themselves and write status[b]: 0, or YV3_EINVAL (H or W <= 0, a byte range outside its
 * buffer, a non-finite coefficient, active not 0 / 1); such an image is copied through and its rows are passed through (nothing
 * is written for an image whose ranges are out of bounds).  The return value covers the host arguments (YV3_EINVAL), checked
 * before the launch.  No workspace, no allocation, no synchronisation, no atomics: identical calls give identical bits.
 * ------------------------------------------------------------------------------------------ */
typedef struct yv3_affine_program {
    int active;                  /* 0: copy the image, pass its rows through; 1: transform        */
    int reserved;
    double fwd[6];               /* source -> output: x' = fwd0 x + fwd1 y + fwd2, y' from 3..5   */
    double inv[6];               /* output -> source, the inverse of fwd                          */
} yv3_affine_program;            /* 104 bytes */

/* Pixels, one launch.  Image b = hw[2b] x hw[2b+1] x 3 bytes, read at src + src_offsets[b] (inside src_bytes: src may be a
 * packed batch or a larger allocation the images are gathered from; it is not written; the same source may occur twice) and
 * written at out + out_offsets[b] (inside out_bytes).  The out ranges of a batch must not overlap each other or the sources (the
 * caller's duty).  All offsets are int64 bytes and need no alignment.  programs: yv3_affine_program[B] in device memory. */
int yv3_affine_augment(const unsigned char* src, long long src_bytes, const long long* src_offsets, const int* hw,
                       const void* programs, int B, unsigned char* out, long long out_bytes, const long long* out_offsets,
                       int* status, void* stream);

/* Labels, one launch.  labels, labels_out: [B][T][5] float64 (NULL when T == 0); labels_out may be labels. */
int yv3_affine_labels(const double* labels, int B, int T, const int* hw, const void* programs,
                      double* labels_out, int* status, void* stream);

/* Stand-alone UpsampleGroup tail (reference darknet.py:159-162: ``F.interpolate(out, scale_factor=2, mode='nearest')`` then
 * ``torch.cat((out, route_tail), 1)``), NCHW fp32:  out[b, c, y, x] = up[b, c, y/2, x/2] for c < c_up, tail[b, c - c_up, y, x] beyond.
 * up [B, c_up, h, w], tail [B, c_tail, 2h, 2w], out [B, c_up + c_tail, 2h, 2w].  Pure data movement (bit-exact).  Inside YoloNet
 * this never runs: the consumer convolution gathers both sources itself (yv3_conv_desc.x / x2 / cin_up). */
int yv3_upsample2x_concat(const float* up, const float* tail, float* out, int B, int c_up, int c_tail, int h, int w, void* stream);

/* ------------------------------------------------------------------------------------------
 * Multi-GPU ("yv3_gather_boxes(comm, ...)").  The reference is single-GPU; images are independent
 * (utils.py:152), so the sharded path has exactly ONE exchange: an all-gather of every rank's [b_local, rows, 7] fp32 payload --
 * rows = cap + 1: the [b_local, cap, 7] output of yv3_postproc_nms plus one row per image carrying its int32 candidate count,
 * kept count and the status word (yv3_conv_desc.flags), bit-cast; layout = yolo_v3_amd/dist.py:pack_payload / unpack_payload --
 * into gathered [world * b_local, rows, 7], rank order.
 *   rccl_comm: an ncclComm_t owned by the caller (ncclCommInitRank ...); stream: hipStream_t the collective is enqueued on.
 * One ncclAllGather over RCCL/xGMI, nothing else; no allocation, no synchronisation.  libyv3.so does not link librccl: the symbol is
 * resolved at the first call (from the process if RCCL is already loaded, else librccl.so.1 / librccl.so), YV3_ERCCL if absent.
 * The Python product (`detect_sharded`) issues the same collective through torch.distributed (backend "nccl" = RCCL), whose
 * communicator cannot be handed out; this entry point is for hosts that own their communicator.
 * ------------------------------------------------------------------------------------------ */
int yv3_gather_boxes(const float* payload, float* gathered, int b_local, int rows, void* rccl_comm, void* stream);

/* ------------------------------------------------------------------------------------------
 * COCO bbox evaluation.  Replaces pycocotools' COCOeval(gt, dt, 'bbox').evaluate() + accumulate() (useCats = 1), which
 * the reference notebook runs on the files evaluate.generate_annotations_file / generate_results_file write
 * (evaluate.ipynb cells 22-25, 48-51).  The caller parses the JSON and maps ids to dense indices: image index = position
 * in the sorted params.imgIds, category index = position in the sorted params.catIds, -1 = not evaluated (dropped).
 * Grouping, greedy matching, ordering and accumulation all run on the device; results are bit-identical to a float64
 * restatement of pycocotools (the file is compiled with -ffp-contract=off).
 *
 * Limits: len(iouThrs) * len(areaRng) <= 64, len(recThrs) <= 128, 1 <= n_maxdet <= YV3_COCO_MAX_MAXDETS, maxDets
 * ascending (COCOeval.evaluate sorts them) with maxDets[-1] <= 1024 -- checked here, YV3_ELIMIT / YV3_EINVAL.  At most
 * 256 GTs per (image, category) group -- found on the device, reported as YV3_ELIMIT in *status (0 = ok), which the
 * caller reads with the outputs; the outputs are then not valid.
 * ------------------------------------------------------------------------------------------ */
#define YV3_COCO_MAX_MAXDETS 8

typedef struct yv3_cocoeval_desc {
    int n_gt, n_det, n_img, n_cat;
    const int* gt_img;           /* [n_gt] dense image index, -1 = dropped                                  */
    const int* gt_cat;           /* [n_gt] dense category index, -1 = dropped                               */
    const double* gt_box;        /* [n_gt][4] x, y, w, h                                                    */
    const double* gt_area;       /* [n_gt] the annotation's 'area' field (area ranges)                      */
    const int* gt_crowd;         /* [n_gt] iscrowd (also the 'ignore' flag, as COCOeval._prepare sets it)   */
    const long long* gt_id;      /* [n_gt] annotation id; a det matched to id 0 counts as unmatched         */
    const int* det_img;          /* [n_det] dense image index, -1 = dropped                                 */
    const int* det_cat;          /* [n_det] dense category index, -1 = dropped                              */
    const double* det_box;       /* [n_det][4] x, y, w, h (area = w * h)                                    */
    const double* det_score;     /* [n_det] score; ties are broken by the position in this array            */
    int n_iou, n_rec, n_area, n_maxdet;
    const double* iou_thrs;      /* [n_iou] params.iouThrs                                                  */
    const double* rec_thrs;      /* [n_rec] params.recThrs                                                  */
    const double* area_rng;      /* [n_area][2] params.areaRng                                              */
    int max_dets[YV3_COCO_MAX_MAXDETS];   /* params.maxDets, ascending (host values)                        */
    double* precision;           /* [n_iou][n_rec][n_cat][n_area][n_maxdet] out                             */
    double* recall;              /* [n_iou][n_cat][n_area][n_maxdet] out                                    */
    double* scores;              /* [n_iou][n_rec][n_cat][n_area][n_maxdet] out                             */
    int* status;                 /* [1] out: 0, or YV3_ELIMIT when a group holds more than 256 GTs           */
} yv3_cocoeval_desc;

/* Bytes of device workspace yv3_cocoeval needs (0 on a bad argument). */
size_t yv3_cocoeval_workspace_bytes(int n_gt, int n_det, int n_img, int n_cat, int n_area);

/* Enqueues the whole evaluation on `stream`; ws: caller-owned device workspace of at least
 * yv3_cocoeval_workspace_bytes(...) bytes (no alignment beyond 256 bytes required). */
int yv3_cocoeval(const yv3_cocoeval_desc* desc, void* ws, size_t ws_bytes, void* stream);

/* ------------------------------------------------------------------------------------------
 * YOLO training loss of one head and dL/dlogits (reference yololayer.py:64-95 + build_target_tensor, yololayer.py:107-172,
 * which builds its targets on the CPU with a Python loop over images and GT rows).  One call = one head; YoloNet makes three.
 * Semantics are the reference's, quirks included: rows of an image are used up to the first all-zero row; the ignore mask
 * (IoU > 0.7 with ANY valid GT of the image) is not cleared at object cells; the best anchor is the first argmax over all
 * nine of the zero-centred IoU, in this head's grid units; two rows on one (image, anchor, cell): offsets and box_coord_mask
 * from the LAST row, classes united, both counted in nGT.  Sums are fp64 in a fixed order: identical calls, identical bits.
 *
 * Rows the reference cannot process -- a class outside [0, C), a negative or NaN value, a cell outside this head's grid,
 * w*h > 2 (math.sqrt of a negative number) -- are reported as YV3_EINVAL in *status; more than YV3_YOLO_LOSS_MAX_ROWS valid
 * rows in one image as YV3_ELIMIT.  Both are found on the device: the caller reads *status with the outputs, which are then
 * not valid.  Zero w / h are accepted, as the reference accepts them.
 * ------------------------------------------------------------------------------------------ */
#define YV3_YOLO_LOSS_MAX_ROWS 1024

typedef struct yv3_yolo_loss_desc {
    const float* logits;         /* raw head logits: element (b, p = gy*W + gx, c = anchor*(5+C) + attr) at
                                    b*stride_b + p*stride_p + c*stride_c (NCHW: H*W*3(5+C), 1, H*W; NHWC rows of ld: H*W*ld, ld, 1) */
    float* grad;                 /* optional out: dL/dlogits at the same offsets, every element written; NULL = skip        */
    long long stride_b, stride_p, stride_c;   /* element strides; they must address distinct elements                     */
    const float* target;         /* [B][T][5] rows (cls, cx, cy, w, h), relative, zero-padded; may be NULL when T == 0      */
    int B, H, W, T, num_class;
    float img_dim_h;             /* img_dim[1] of the reference: stride = img_dim_h / H                                      */
    float anchors[18];           /* all nine anchors (w, h), input pixels (host values)                                      */
    int mask[3];                 /* this head's anchor indices into anchors[]                                                */
    double* sums;                /* [6] out: loss_x, loss_y, loss_w, loss_h, loss_conf, loss_cls (the reference's sums)     */
    int* counts;                 /* [2] out: nCorrect, nGT                                                                   */
    int* status;                 /* [1] out: 0, YV3_EINVAL (a row the reference cannot process) or YV3_ELIMIT               */
} yv3_yolo_loss_desc;

/* Bytes of device workspace yv3_yolo_loss needs for B images of an H x W head and T target rows (0 on a bad argument). */
size_t yv3_yolo_loss_workspace_bytes(int B, int H, int W, int T);

/* Enqueues the loss (and the gradient when desc->grad is set) on `stream`: three launches, no allocation, no synchronisation.
 * ws: caller-owned device workspace of at least yv3_yolo_loss_workspace_bytes(B, H, W, T) bytes.  Pointers, sizes, anchors
 * and strides are checked here, before any launch (YV3_EINVAL / YV3_ESHAPE / YV3_EWORKSPACE). */
int yv3_yolo_loss(const yv3_yolo_loss_desc* desc, void* ws, size_t ws_bytes, void* stream);

/* ------------------------------------------------------------------------------------------
 * Training step (reference train.py: `loss = net(inp, labels); loss.backward()`, with darknet.py:27-53 in train mode), exact fp32
 * (csrc/train.hip; the bf16 counterparts of the convolution calls follow below).  Activations and gradients are fp32 NHWC [B][H][W][C] (P = B*H*W rows of C), except the first layer's
 * input, which is read in place as the caller's NCHW batch (x_nchw = 1).  Weights are torch's [cout][cin][k][k].  k is 1 or 3,
 * stride 1 or 2, padding (k-1)/2.  cin_up > 0: the input is cat(up2x(x2), x) along channels (reference darknet.py:161-162), read
 * in place: x2 is the low-resolution [B][H/2][W/2][cin_up] map, x the [B][H][W][cin-cin_up] route tail.  No call allocates or
 * synchronises; workspaces come from the caller.  Nothing uses float atomics and every sum runs in a fixed order, so identical
 * calls give identical bits.  YV3_EINVAL: null pointer / non-positive size; YV3_ESHAPE: k, stride, cin_up outside the above.
 * ------------------------------------------------------------------------------------------ */

/* wf (optional): [k*k*cin][cout], wd (optional): [k*k*cout][cin] -- the operand images of yv3_train_conv_fwd / _dgrad. */
int yv3_train_pack_weight(const float* w, float* wf, float* wd, int cout, int cin, int k, void* stream);

/* z = conv(x, w) [+ bias]: the pre-BatchNorm output of a conv_bn_relu (darknet.py:40, nn.Conv2d(bias=False)) or a head conv's
 * logits (darknet.py:115, bias given).  z: [B][Ho][Wo][cout]. */
int yv3_train_conv_fwd(const float* x, const float* x2, const float* wf, const float* bias, float* z,
                       int B, int H, int W, int cin, int cin_up, int cout, int k, int stride, int x_nchw, void* stream);

/* dx (+)= dL/dx of z = conv(x, w) for dz = dL/dz ([B][Ho][Wo][cout]); dx: [B][H][W][cin], added to when accumulate != 0. */
int yv3_train_conv_dgrad(const float* dz, const float* wd, float* dx, int B, int H, int W, int cin, int cout, int k, int stride,
                         int accumulate, void* stream);

/* dx = dL/dx of layer 0 (3x3, stride 1, pad 1, cin = 3): dz [B][H][W][cout] fp32, w the parameter itself [cout][3][3][3] fp32,
 * dx [B][3][H][W] fp32, overwritten -- the input gradient in the caller's NCHW layout (a direct memory-bound kernel, not the GEMM
 * tile).  cout must be a multiple of 4 (YV3_ESHAPE). */
int yv3_train_conv0_dgrad(const float* dz, const float* w, float* dx_nchw, int B, int H, int W, int cout, void* stream);

/* dw = dL/dw ([cout][cin][k][k], overwritten), a sum over all B*Ho*Wo output pixels split into chunks whose partials live in ws
 * and are added in chunk order.  The workspace size query takes the full cin (cin_up does not change it); 0 on a bad shape. */
size_t yv3_train_conv_wgrad_workspace_bytes(int B, int H, int W, int cin, int cout, int k, int stride);
int yv3_train_conv_wgrad(const float* x, const float* x2, const float* dz, float* dw, int B, int H, int W, int cin, int cin_up,
                         int cout, int k, int stride, int x_nchw, void* ws, size_t ws_bytes, void* stream);

/* Workspace of the per-channel reductions below over P rows of C channels (0 on a bad argument). */
size_t yv3_train_channel_workspace_bytes(long long P, int C);

/* Train-mode BatchNorm statistics of z (nn.BatchNorm2d, darknet.py:41): mean and 1/sqrt(biased var + eps) per channel.  With
 * run_*_out set, run_*_out = (1 - momentum) run_* + momentum (mean, unbiased var); they may alias run_*. */
int yv3_train_bn_stats(const float* z, long long P, int C, float eps, float momentum, const float* run_mean, const float* run_var,
                       float* run_mean_out, float* run_var_out, float* mean, float* invstd, void* ws, size_t ws_bytes, void* stream);

/* Eval-mode BatchNorm: mean = running_mean, invstd = 1/sqrt(running_var + eps). */
int yv3_train_bn_eval_stats(const float* run_mean, const float* run_var, float eps, float* mean, float* invstd, int C, void* stream);

/* y = LeakyReLU_0.1(gamma (z - mean) invstd + beta) [+ residual]  (darknet.py:41-44; the residual after the activation, :53). */
int yv3_train_bn_act_fwd(const float* z, const float* mean, const float* invstd, const float* gamma, const float* beta,
                         const float* residual, float* y, long long P, int C, void* stream);

/* Backward of yv3_train_bn_act_fwd for dy = dL/dy: with du = dy * act'(u), dbeta = sum du, dgamma = sum du * xhat, and
 * dz = gamma invstd (du - dbeta/P - xhat dgamma/P) when train != 0 (batch statistics), dz = gamma invstd du otherwise. */
int yv3_train_bn_act_bwd(const float* z, const float* dy, const float* mean, const float* invstd, const float* gamma, const float* beta,
                         float* dz, float* dgamma, float* dbeta, long long P, int C, int train, void* ws, size_t ws_bytes, void* stream);

/* Head conv bias (darknet.py:115): dout = dlogits * (*scale) (scale: device fp32 scalar, NULL = 1), dbias = sum over P of dout. */
int yv3_train_bias_bwd(const float* dlogits, const float* scale, float* dout, float* dbias, long long P, int C, void* ws, size_t ws_bytes,
                       void* stream);

/* dst += src (the gradient of an activation that fans out: residual skips, route tails, route heads). */
int yv3_train_add(const float* src, float* dst, long long n, void* stream);

/* Backward of cat(up2x(low), tail) (darknet.py:161-162): dlow (+)= the 2x2 sums of channels [0, cin_up) of dcat, dtail (+)= the
 * other ctail channels.  H, W: the full resolution; either output may be NULL. */
int yv3_train_upcat_bwd(const float* dcat, float* dlow, float* dtail, int B, int H, int W, int cin_up, int ctail,
                        int acc_low, int acc_tail, void* stream);

/* ------------------------------------------------------------------------------------------
 * BF16 training step (net.backprop_math = BF16, csrc/train_bf16.hip): the three convolution products above with both operands
 * rounded to bf16 (round to nearest even, as torch's fp32 -> bf16 conversion) and fp32 accumulation; z, dx and dw stay fp32.
 * bf16 tensors are passed as raw 16-bit images (void*).  coutp = cout rounded up to a multiple of 8: a bf16 dz has coutp
 * channels, the padding ones zero (yv3_train_to_bf16 with ld = coutp).  Except on the first layer (x_nchw = 1), cin and cin_up
 * must be multiples of 8 (YV3_ESHAPE otherwise).  Errors, determinism and the absence of allocation / synchronisation are as for
 * the fp32 calls.
 * ------------------------------------------------------------------------------------------ */

/* dst[r][c] = bf16(src[r][c]) for c < C, 0 for C <= c < ld (rows of C fp32 in, rows of ld bf16 out).  NaN -> 0x7fc0. */
int yv3_train_to_bf16(const float* src, void* dst, long long rows, int C, int ld, void* stream);

/* wf (optional): [coutp][k*k*cin] bf16 (K index tap*cin + ci), wd (optional): [cin][k*k*coutp] bf16 (K index tap*coutp + co);
 * padding channels zero -- the operand images of yv3_train_conv_fwd_bf16 / _dgrad_bf16. */
int yv3_train_pack_weight_bf16(const float* w, void* wf, void* wd, int cout, int cin, int k, void* stream);

/* z = conv(bf16 x, bf16 w) [+ bias], fp32 [B][Ho][Wo][cout]; x, x2 as yv3_train_conv_fwd's, in bf16. */
int yv3_train_conv_fwd_bf16(const void* x, const void* x2, const void* wf, const float* bias, float* z,
                            int B, int H, int W, int cin, int cin_up, int cout, int k, int stride, int x_nchw, void* stream);

/* dx (+)= dL/dx for the bf16 dz ([B][Ho][Wo][coutp]); dx fp32 [B][H][W][cin]. */
int yv3_train_conv_dgrad_bf16(const void* dz, const void* wd, float* dx, int B, int H, int W, int cin, int cout, int k, int stride,
                              int accumulate, void* stream);

/* The same for the bf16 dz copy ([B][H][W][coutp], coutp = cout rounded up to 8); w is rounded to bf16 inside, RNE as
 * yv3_train_to_bf16 rounds; products accumulate in fp32. */
int yv3_train_conv0_dgrad_bf16(const void* dz, const float* w, float* dx_nchw, int B, int H, int W, int cout, void* stream);

/* dw = dL/dw (fp32 [cout][cin][k][k]) from bf16 x and dz ([B][Ho][Wo][coutp]); fp32 split partials summed in split order in fp64. */
size_t yv3_train_conv_wgrad_bf16_workspace_bytes(int B, int H, int W, int cin, int cout, int k, int stride);
int yv3_train_conv_wgrad_bf16(const void* x, const void* x2, const void* dz, float* dw, int B, int H, int W, int cin, int cin_up,
                              int cout, int k, int stride, int x_nchw, void* ws, size_t ws_bytes, void* stream);

/* ------------------------------------------------------------------------------------------
 * BF16_ACT training step (net.backprop_math = BF16_ACT, csrc/train_bf16.hip and csrc/train_bf16_act.hip): the BF16 step with every
 * conv_bn_relu activation stored once, in bf16 -- the conv output zb = bf16(z32), the layer output bf16(leaky(bn(zb)) [+ res]) and
 * dz -- and no fp32 z, y or dz.  The arithmetic between two stores is fp32 (fp64 in the reductions), each store rounds as
 * yv3_train_to_bf16 does.  C (cout) must be a multiple of 8 except for yv3_train_bias_bwd_bf16 (YV3_ESHAPE otherwise).
 * ------------------------------------------------------------------------------------------ */

/* zb = bf16(conv(bf16 x, bf16 w)), [B][Ho][Wo][cout] bf16: yv3_train_conv_fwd_bf16's accumulators (same kernel, same order), no bias. */
int yv3_train_conv_fwd_bf16o(const void* x, const void* x2, const void* wf, void* zb, int B, int H, int W, int cin, int cin_up, int cout,
                             int k, int stride, int x_nchw, void* stream);

/* Workspace of the four calls below over P rows of C channels (0 on a bad argument). */
size_t yv3_train_channel_bf16_workspace_bytes(long long P, int C);

/* yv3_train_bn_stats of a bf16 z. */
int yv3_train_bn_stats_bf16(const void* z, long long P, int C, float eps, float momentum, const float* run_mean, const float* run_var,
                            float* run_mean_out, float* run_var_out, float* mean, float* invstd, void* ws, size_t ws_bytes, void* stream);

/* y = bf16(leaky(gamma (z - mean) invstd + beta) [+ residual]); z, residual and y bf16 [P][C]. */
int yv3_train_bn_act_fwd_bf16(const void* z, const float* mean, const float* invstd, const float* gamma, const float* beta,
                              const void* residual, void* y, long long P, int C, void* stream);

/* yv3_train_bn_act_bwd of a bf16 z and a fp32 dy; dz is written as bf16 [P][C], dgamma and dbeta as fp32. */
int yv3_train_bn_act_bwd_bf16(const void* z, const float* dy, const float* mean, const float* invstd, const float* gamma,
                              const float* beta, void* dz, float* dgamma, float* dbeta, long long P, int C, int train, void* ws,
                              size_t ws_bytes, void* stream);

/* yv3_train_bias_bwd with dout = bf16(dlogits * (*scale)) in rows of C rounded up to a multiple of 8, the padding channels zero;
 * dbias sums the fp32 products. */
int yv3_train_bias_bwd_bf16(const float* dlogits, const float* scale, void* dout, float* dbias, long long P, int C, void* ws,
                            size_t ws_bytes, void* stream);

/* ------------------------------------------------------------------------------------------
 * Baseline JPEG decode (csrc/jpeg_parse.cpp, csrc/jpeg_entropy.h, csrc/jpeg.hip): file bytes -> uint8 RGB [H][W][3], the bits
 * libjpeg(-turbo)'s defaults give (integer "islow" IDCT, "fancy" chroma upsampling, fixed-point YCbCr -> RGB), for a batch of
 * files in four launches.  The host parser accepts only what it positively recognises; every other file gets a reason and is
 * the caller's to decode elsewhere (yolo_v3_amd.jpeg falls back to PIL).  Errors in the entropy-coded data, and coefficients
 * no 8-bit encoder writes, are found on the device and reported per image in status[]; such an image's destination bytes are
 * unspecified (inside its own extent).  Status 0 means libjpeg's bytes.
 * ------------------------------------------------------------------------------------------ */

/* yv3_jpeg_info.reason: why yv3_jpeg_parse refuses a file (0 = accepted) */
#define YV3_JPEG_OK            0
#define YV3_JPEG_NOT_JPEG      1   /* no SOI                                                                   */
#define YV3_JPEG_MALFORMED     2   /* a header segment that is cut short or contradicts itself                 */
#define YV3_JPEG_PROGRESSIVE   3   /* SOF2                                                                     */
#define YV3_JPEG_SOF           4   /* arithmetic, lossless or hierarchical frames (SOF3, 5..7, 9..11, 13..15)  */
#define YV3_JPEG_PRECISION     5   /* samples or quantisation tables wider than 8 bits                         */
#define YV3_JPEG_COMPONENTS    6   /* neither 1 nor 3 components (CMYK / YCCK)                                 */
#define YV3_JPEG_COLORSPACE    7   /* 3 components not known to be YCbCr (Adobe APP14, or no JFIF and ids != 1,2,3) */
#define YV3_JPEG_SAMPLING      8   /* luma not 1x1 / 2x1 / 2x2, or chroma not 1x1 (4:4:0, 4:1:1, ...)          */
#define YV3_JPEG_MULTISCAN     9   /* the first scan does not hold all components, or something other than EOI follows it */
#define YV3_JPEG_TABLES        10  /* a table the scan names is missing or invalid when SOS is reached         */
#define YV3_JPEG_SIZE          11  /* a side of 0 or above 16384                                               */

/* status[b] of yv3_jpeg_decode_batch (0 = decoded) */
#define YV3_JPEG_S_INFO        1   /* the record is not one yv3_jpeg_parse accepts                              */
#define YV3_JPEG_S_BOUNDS      2   /* the scan, the destination or the workspace share lies outside its buffer */
#define YV3_JPEG_S_HUFFTABLE   3   /* a Huffman spec that is no prefix code                                     */
#define YV3_JPEG_S_CODE        4   /* a bit pattern that is no code of the table                                */
#define YV3_JPEG_S_OVERRUN     5   /* the data ended inside a unit                                              */
#define YV3_JPEG_S_COEF        6   /* a run past coefficient 63, or a block past the unit's last one            */
#define YV3_JPEG_S_MARKER      7   /* restart markers: wrong count or order, or a marker inside a unit          */
#define YV3_JPEG_S_EXTRA       8   /* whole bytes left over at the end of a unit                                */
#define YV3_JPEG_S_DC          9   /* a DC value outside 16 bits                                                */
#define YV3_JPEG_S_RANGE       10  /* a block outside the range in which every libjpeg IDCT gives the same bytes: a dequantised
                                      coefficient or a column-pass output outside +-16383, or a sample outside [-512, 511]
                                      before the +128 (no 8-bit encoder writes such a block; libjpeg's 16-bit SIMD words and its
                                      masked range-limit index then wrap, each build its own way)                 */

typedef struct yv3_jpeg_info {
    long long scan_offset;            /* first entropy-coded byte, from the start of the file                                  */
    long long scan_length;            /* bytes up to the marker that ends the scan (or to the end of a truncated file)         */
    int width, height, ncomp;
    int restart_interval;             /* MCUs per restart segment, 0 = none                                                    */
    int reason;                       /* YV3_JPEG_*: 0 = every field is valid and the file is one the decoder takes            */
    int has_exif;                     /* an APP1 "Exif" segment is present (the orientation is the caller's to read)           */
    unsigned char h[4], v[4];         /* sampling factors per component, as in SOF                                             */
    unsigned char tq[4], td[4], ta[4];/* quantiser index (SOF), DC and AC Huffman selector (SOS) per component                 */
    unsigned char quant_defined[4];
    unsigned char huff_defined[8];    /* tables 0..3: DC 0..3, tables 4..7: AC 0..3                                            */
    unsigned char quant[4][64];       /* natural (row-major) order                                                             */
    unsigned char huff_counts[8][16]; /* codes of length 1..16                                                                 */
    unsigned char huff_values[8][256];
} yv3_jpeg_info;

/* Host only, no GPU: walks the markers of data[0, n) and fills *out.  Returns YV3_EINVAL for a null pointer, else 0 with
 * out->reason set.  Accepted (reason 0): SOF0 / SOF1, 8-bit samples and tables, 1 component or 3 YCbCr components (a JFIF
 * marker, or ids 1,2,3; no Adobe APP14), one interleaved scan over all components, luma 1x1 / 2x1 / 2x2 with chroma 1x1,
 * sides <= 16384, every table defined before SOS.  No byte outside data[0, n) is read, whatever the bytes are. */
int yv3_jpeg_parse(const unsigned char* data, size_t n, yv3_jpeg_info* out);

typedef struct yv3_jpeg_batch_desc {
    const unsigned char* src;         /* device: the files' bytes                                                              */
    long long src_bytes;
    const long long* src_offsets;     /* device [B]: file b starts at src + src_offsets[b] (any alignment; files may repeat)   */
    const yv3_jpeg_info* infos;       /* device [B]: the parser's records -- what the kernels read and re-check                */
    const yv3_jpeg_info* infos_host;  /* host [B]: the same records, for the argument checks and the launch geometry           */
    unsigned char* dst;               /* device: image b = uint8 RGB [H][W][3] at dst + dst_offsets[b]                         */
    long long dst_bytes;
    const long long* dst_offsets;     /* device [B]: checked against dst_bytes on the device, in 64 bits                       */
    int* status;                      /* device [B] out: YV3_JPEG_S_*                                                          */
    int B;
} yv3_jpeg_batch_desc;

/* Host only: bytes of device workspace a batch of these (host) records needs -- per image the int16 coefficients, the uint8
 * component planes and the restart-segment offsets.  0 on a bad argument; a record with reason != 0 adds nothing. */
size_t yv3_jpeg_workspace_bytes(const yv3_jpeg_info* infos_host, int B);

/* Enqueues the decode of B files on `stream`: layout, entropy decode (one workgroup per image, one lane per restart segment),
 * IDCT, upsampling + colour.  ws must be 256-byte aligned (the kernels make 16-byte accesses at 256-aligned offsets from it).
 * YV3_EINVAL (null pointer, ws not 256-aligned, B outside 1..65535, non-positive sizes), YV3_ESHAPE (a host record
 * with reason != 0 or fields the parser cannot produce), YV3_EWORKSPACE -- all before any launch.  Integer arithmetic only:
 * identical calls give identical bits. */
int yv3_jpeg_decode_batch(const yv3_jpeg_batch_desc* desc, void* ws, size_t ws_bytes, void* stream);

/* The entropy stage of yv3_jpeg_decode_batch_ex (an enum, not status or reason codes).
 * SERIAL: one lane per unit (a whole scan, or a restart segment), as yv3_jpeg_decode_batch.
 * PARALLEL: the self-synchronising decoder (csrc/jpeg_sync.h).  A unit of 256 bytes or more is cut into subsequences of 64
 * bytes, one lane each; a lane decodes speculatively from its first bit, exit states are handed down the chain until each
 * subsequence's entry state is proven from the unit's first bit (windows of 256 subsequences, at most 16 proving passes each),
 * and only proven lanes write.  Shorter units take one lane each as before; one image may hold both kinds. */
enum { YV3_JPEG_ENTROPY_SERIAL = 0, YV3_JPEG_ENTROPY_PARALLEL = 1 };

/* yv3_jpeg_workspace_bytes for the given entropy stage.  The parallel stage keeps its per-subsequence records in LDS, so both
 * stages need the same bytes; 0 on a bad argument or an unknown `entropy`. */
size_t yv3_jpeg_workspace_bytes_ex(const yv3_jpeg_info* infos_host, int B, int entropy);

/* yv3_jpeg_decode_batch with the entropy stage chosen per call; SERIAL is yv3_jpeg_decode_batch itself, through the same code.
 * The status contract of PARALLEL: status[b] and, at status 0, every destination byte are exactly SERIAL's for the same input,
 * whatever the bytes are.  The parallel stage either establishes that the serial routine would return 0 for a unit and have
 * written exactly these coefficients, or it zeroes the unit's coefficients again and runs the serial routine on one lane in the
 * same launch (an FF that is no FF 00 pair, an error from a proven state, a wrong block count, a failed end check, a DC value
 * outside 16 bits); that routine's status stands.  handed_over: device [B] or null; with PARALLEL, handed_over[b] = the units of
 * image b that were handed to the serial routine -- 0 for every file an encoder can write (not written with SERIAL).  The same
 * argument checks before any launch, and YV3_EINVAL for an unknown `entropy`; no allocation, no synchronisation. */
int yv3_jpeg_decode_batch_ex(const yv3_jpeg_batch_desc* desc, int entropy, int* handed_over, void* ws, size_t ws_bytes, void* stream);

/* ---- Progressive files (SOF2; csrc/jpeg_prog.h), opt-in at every layer ----------------------------
 * yv3_jpeg_parse_ex with YV3_JPEGP_ACCEPT describes an accepted progressive file in a yv3_jpeg_prog record; its yv3_jpeg_info
 * keeps reason = YV3_JPEG_PROGRESSIVE, so every entry above still refuses the file.  yv3_jpeg_decode_batch_prog takes a batch
 * that mixes baseline and progressive images.  (These names carry the prefix YV3_JPEGP_: the YV3_JPEG_ codes above are a
 * closed list.) */
#define YV3_JPEGP_ACCEPT       1   /* the `accept` flag of yv3_jpeg_parse_ex: progressive files                  */
#define YV3_JPEGP_MAX_SCANS    64  /* a grey file with one scan per coefficient fits                             */
#define YV3_JPEGP_MAX_TABLES   66  /* every scan's tables fit: 63 AC scans, one table each, and three DC tables  */

/* further yv3_jpeg_info.reason codes, given by yv3_jpeg_parse_ex with YV3_JPEGP_ACCEPT alone */
#define YV3_JPEGP_SCAN         12  /* a scan header outside the accepted forms: Ss = 0 with Se != 0, an interleaved AC scan,
                                      Se < Ss or Se > 63, Al > 13, Ah neither 0 nor Al + 1, components repeated or out of order */
#define YV3_JPEGP_SCRIPT       13  /* the scans are no complete progression: a repeated first scan, a refinement whose Ah is not
                                      the Al before it, AC before DC, a band missing or not coded down to Al = 0 at EOI, or a
                                      segment between scans that is none of DHT, DRI, COM, APPn                               */
#define YV3_JPEGP_CAPACITY     14  /* more than YV3_JPEGP_MAX_SCANS scans                                         */
#define YV3_JPEGP_DQT          15  /* a quantisation table after the first SOS                                   */

/* further status[b] codes of yv3_jpeg_decode_batch_prog */
#define YV3_JPEGP_S_REFINE     11  /* a refinement scan's symbol whose size is neither 0 nor 1                    */
#define YV3_JPEGP_S_VALUE      12  /* an AC coefficient outside 16 bits after the shift or a correction           */

typedef struct yv3_jpegp_scan {
    long long offset, length;         /* the scan's entropy-coded bytes, from the start of the file                            */
    int restart_interval;             /* the DRI in force at this SOS: MCUs (interleaved) or the component's own blocks         */
    int pad0;
    unsigned char ns;                 /* components in the scan, 1..3                                                          */
    unsigned char ss, se, ah, al;
    unsigned char level;              /* 1..nlevels: yv3_jpegp_levels' (csrc/jpeg_prog.h), recomputed on the device            */
    unsigned char comp[3];            /* component indices, ascending                                                          */
    unsigned char tab[3];             /* per component: index into tables[] -- the DC table of a first DC scan, the AC table
                                         of an AC scan (tab[0]); unused entries are 255                                        */
    unsigned char pad1[4];
} yv3_jpegp_scan;

typedef struct yv3_jpegp_table { unsigned char counts[16], values[256]; } yv3_jpegp_table;

/* One image's progressive record, FIXED SIZE (a batch's records are an array; about 20 KB each, and only progressive images
 * carry one).  tables[] holds each Huffman specification some scan uses, as it was in force at that scan's SOS: a table that
 * is redefined between two scans takes two entries. */
typedef struct yv3_jpeg_prog {
    int accepted;                     /* 1: a progressive file the decoder takes; 0: none (every other field is then 0)        */
    int nscans, ntables, nlevels;
    yv3_jpegp_scan scans[YV3_JPEGP_MAX_SCANS];
    yv3_jpegp_table tables[YV3_JPEGP_MAX_TABLES];
} yv3_jpeg_prog;

/* yv3_jpeg_parse with an `accept` flag word and a progressive record (prog may be null when accept is 0).  accept = 0: *out is
 * yv3_jpeg_parse's, byte for byte, and *prog is zeroed.  With YV3_JPEGP_ACCEPT a SOF2 file is walked to its EOI: accepted
 * (prog->accepted = 1, out->reason stays YV3_JPEG_PROGRESSIVE) when the frame obeys the baseline frame rules and the scans are a
 * complete progression libjpeg decodes without a warning -- every scan of the forms in YV3_JPEGP_SCAN's comment with its tables
 * defined at its SOS, every coefficient of every component coded first with Ah = 0 and then down to Al = 0, no DQT after the
 * first SOS, nothing but EOI (or the end of a truncated file) after the last scan; otherwise out->reason says why.  out's
 * frame fields (size, components, sampling, quantisers, has_exif) are valid for an accepted file; its scan and Huffman fields
 * are not meaningful.  No byte outside data[0, n) is read.  For such a record yv3_jpeg_workspace_bytes and _ex answer as for
 * any refused record -- the image adds nothing, so the result is the slot table of the batch (256 for B = 1), not 0 -- and the
 * older decode entries answer YV3_ESHAPE. */
int yv3_jpeg_parse_ex(const unsigned char* data, size_t n, int accept, yv3_jpeg_info* out, yv3_jpeg_prog* prog);

/* yv3_jpeg_batch_desc plus the progressive records.  prog_of[b] = index of image b's record in progs, or -1 for a baseline
 * image (whose info record has reason 0). */
typedef struct yv3_jpeg_batch_desc_prog {
    yv3_jpeg_batch_desc base;
    const yv3_jpeg_prog* progs;       /* device [P]                                                                            */
    const yv3_jpeg_prog* progs_host;  /* host [P]: the same records                                                            */
    const int* prog_of;               /* device [B]                                                                            */
    const int* prog_of_host;          /* host [B]                                                                              */
    int P;                            /* 0: no progressive image; progs* may then be null                                      */
} yv3_jpeg_batch_desc_prog;

/* Host only: workspace bytes of yv3_jpeg_decode_batch_prog.  Without a progressive image it is yv3_jpeg_workspace_bytes_ex's;
 * with one, a device copy of every info record and the restart offsets of every scan are added.  0 on a bad argument. */
size_t yv3_jpeg_workspace_bytes_prog(const yv3_jpeg_info* infos_host, const int* prog_of_host, const yv3_jpeg_prog* progs_host, int P,
                                     int B, int entropy);

/* yv3_jpeg_decode_batch_ex for a batch that may hold progressive images.  Baseline images take the entropy stage `entropy`
 * names, exactly as there; progressive images take entropy_prog_kernel (one workgroup per image; scans that code different
 * coefficients run side by side, level by level), which is not launched when P is 0 -- the call is then
 * yv3_jpeg_decode_batch_ex itself.  The device records are re-checked before any kernel trusts them; the status contract is
 * the same: status 0 means libjpeg's bytes.  YV3_ESHAPE also for a prog_of_host entry outside [-1, P), a baseline record with
 * reason != 0 and a progressive record yv3_jpeg_parse_ex cannot have produced. */
int yv3_jpeg_decode_batch_prog(const yv3_jpeg_batch_desc_prog* desc, int entropy, int* handed_over, void* ws, size_t ws_bytes,
                               void* stream);

/* The kernels yv3_jpeg_decode_batch, _ex and _prog have launched in this process so far, counted where they are launched (for
 * tests and measurements: a batch without a progressive image adds four, one with a progressive image five). */
long long yv3_jpeg_launch_count(void);

/* ------------------------------------------------------------------------------------------
 * Baseline JPEG encode (csrc/jpeg_enc.h, csrc/jpeg_enc.hip): uint8 RGB or grey pixels on the device ->
 * the file libjpeg(-turbo) writes for them at the same quality and subsampling with its defaults -- Annex K tables scaled by
 * the quality, fixed-point RGB -> YCbCr, h2v1 / h2v2 downsampling, the "islow" forward DCT, the standard Huffman tables, no
 * restart markers, a JFIF APP0 -- byte for byte.  A batch of images of any sizes and modes takes nine launches; nothing
 * allocates, nothing synchronises, identical calls give identical bytes.
 * Limits: sides up to 16384 and at most 2 000 000 blocks in the scan, dummy blocks included (4096 x 4096 in 4:4:4 has 786 432),
 * so that every bit offset of an image fits 32 bits; beyond that YV3_ELIMIT.  (The encoder's names carry the prefix YV3_JPEGE_,
 * as the progressive decoder's carry YV3_JPEGP_: the YV3_JPEG_ codes are the baseline decoder's closed set.)
 * ------------------------------------------------------------------------------------------ */
enum { YV3_JPEGE_444 = 0, YV3_JPEGE_422 = 1, YV3_JPEGE_420 = 2 };      /* `subsampling` (PIL's numbers); ignored for grey */

/* status[b] of the encode call (0 = out holds the file, out_len[b] bytes) */
#define YV3_JPEGE_S_INFO    1   /* the device record is no image the encoder takes (sizes, pitch, null pointers)        */
#define YV3_JPEGE_S_BOUNDS  2   /* the device records need more workspace than the host records the call was sized by   */
#define YV3_JPEGE_S_SPACE   3   /* out_cap is smaller than the file: nothing is written, out_len[b] is the length needed */
#define YV3_JPEGE_S_RANGE   4   /* a DC difference above category 11 or an AC value above category 10 (no 8-bit image
                                      gives one): no code exists for it, nothing is written                                */

typedef struct yv3_jpeg_enc_image {
    const unsigned char* pixels;      /* device: [height] rows of width * ncomp bytes, `pitch` bytes apart (RGB or grey)        */
    long long pitch;                  /* >= width * ncomp                                                                      */
    unsigned char* out;               /* device: the file is written to out[0, out_len)                                        */
    long long out_cap;                /* bytes at out; no byte at or past out + out_cap is ever written                        */
    int width, height;
    int ncomp;                        /* 3: RGB -> YCbCr; 1: grey                                                              */
    int subsampling;                  /* YV3_JPEGE_*                                                                        */
    int quality;                      /* 1..100, libjpeg's scale                                                               */
    int reserved;
} yv3_jpeg_enc_image;

typedef struct yv3_jpeg_enc_desc {
    const yv3_jpeg_enc_image* images;       /* device [B]: what the kernels read and check                                     */
    const yv3_jpeg_enc_image* images_host;  /* host [B]: the same records, for the argument checks, the workspace and the grids */
    int* out_len;                     /* device [B] out: the file's length (also when status is YV3_JPEGE_S_SPACE)          */
    int* status;                      /* device [B] out: YV3_JPEGE_S_*                                                      */
    int B;                            /* 1..65535                                                                              */
} yv3_jpeg_enc_desc;

/* Host only: the bytes of the file up to and including the SOS segment, in libjpeg's order (SOI, APP0, one DQT per table, SOF0,
 * DHT DC0 AC0 [DC1 AC1], SOS).  Writes at most cap bytes and returns the header's length (out may be null when cap is 0), or
 * YV3_EINVAL / YV3_ELIMIT. */
long long yv3_jpeg_encode_header(int width, int height, int ncomp, int subsampling, int quality, unsigned char* out, long long cap);

/* Host only: a length no file of this size and mode exceeds -- the header, the scan at 11 + 11 bits for every DC and 16 + 10 for
 * every AC coefficient (the longest codes of the standard tables with the widest values), doubled for stuffing, and EOI.
 * YV3_EINVAL / YV3_ELIMIT (negative) otherwise. */
long long yv3_jpeg_encode_bound(int width, int height, int ncomp, int subsampling);

/* Host only: workspace bytes of the encode call for these records; 0 on a bad argument or a record the call refuses. */
size_t yv3_jpeg_encode_workspace_bytes(const yv3_jpeg_enc_image* images_host, int B);

/* Encodes the batch on `stream`.  ws: device, 256-aligned, its contents need not be cleared and may be reused by the next call.
 * YV3_EINVAL (null pointer, B outside 1..65535, sizes < 1, ncomp not 1 or 3, unknown subsampling, quality outside 1..100, pitch
 * too small), YV3_ELIMIT (see above), YV3_EWORKSPACE -- all from the host records, before any launch.  The device records are
 * checked again by the kernels (status). */
int yv3_jpeg_encode_batch(const yv3_jpeg_enc_desc* desc, void* ws, size_t ws_bytes, void* stream);

/* ------------------------------------------------------------------------------------------
 * Box outlines and label tags drawn into a batch of uint8 RGB images in place (csrc/draw.hip), one launch.
 * Every pixel decides its own colour by walking its image's boxes in order -- outline, then tag, the last writer wins -- so the
 * result needs no atomics and does not depend on scheduling.  Box j's outline: the pixels of [x1, x2] x [y1, y2] less than
 * `thickness` pixels from one of the four sides.  Its tag (tag >= 0; mask of mw x mh bits): left = max(min(max(x1, 0), W - mw), 0),
 * bottom = min(max(y1, mh), H), top = bottom - mh; the pixels of [left, left + mw) x [top, bottom) inside the image take the box
 * colour, and black where the mask bit is set.  A mask row is ceil(mw / 8) bytes, the leftmost pixel in bit 7.
 * ------------------------------------------------------------------------------------------ */
typedef struct yv3_draw_image {
    unsigned char* pixels;            /* device: [height][width][3] with rows `pitch` bytes apart                              */
    long long pitch;
    int width, height;
    int first_box, num_boxes;         /* this image's boxes: boxes[first_box, first_box + num_boxes), painted in that order    */
} yv3_draw_image;

typedef struct yv3_draw_box {
    int x1, y1, x2, y2;
    int tag;                          /* index into tags, or -1: no tag                                                        */
    unsigned char rgb[3], reserved;
} yv3_draw_box;

typedef struct yv3_draw_tag {
    long long offset;                 /* of the mask's first byte in the atlas                                                 */
    int width, height;
} yv3_draw_tag;

/* images, boxes, tags, atlas: device.  max_width / max_height: at least every image's (they size the grid; an image larger than
 * that is left untouched).  Images without boxes are not written.  The kernel bounds every box, tag and atlas access by num_boxes_total,
 * num_tags and atlas_bytes.  YV3_EINVAL: null pointer (boxes / tags / atlas may be null when their count is 0), B < 1,
 * thickness < 1, non-positive sizes. */
int yv3_draw_boxes(const yv3_draw_image* images, int B, const yv3_draw_box* boxes, int num_boxes_total, const yv3_draw_tag* tags,
                   int num_tags, const unsigned char* atlas, long long atlas_bytes, int thickness, int max_width, int max_height,
                   void* stream);

/* ------------------------------------------------------------------------------------------
 * The update step (csrc/optim.hip; yolo_v3_amd/optim.py): torch's clip_grad_norm_, torch.optim.SGD and torch.optim.Adam / AdamW
 * over a list of fp32 tensors, a few launches for the whole list.  The list arguments (g, p, buf, n, ...) are HOST arrays of `count` device pointers /
 * element counts; they are read during the call and travel in the kernel arguments, so the caller may reuse them at once.
 * Each workgroup owns YV3_OPTIM_CHUNK consecutive elements of one tensor.  Pointers need 4-byte alignment only (16-byte
 * aligned entries take 16-byte accesses); every access is bounded by the entry's n.  Entries must not overlap.  No allocation,
 * no synchronisation, no device-to-host read, no atomics: identical calls give identical bits.  YV3_EINVAL (a null pointer, a
 * count < 0, an n <= 0, unknown flags), YV3_EWORKSPACE, YV3_ELIMIT (a tensor of more than 2^30 chunks) -- all before any launch.
 * ------------------------------------------------------------------------------------------ */
#define YV3_OPTIM_CHUNK   16384
#define YV3_SGD_FIRST     1   /* the first step of these parameters: buf = d (buf is not read)   */
#define YV3_SGD_NESTEROV  2
#define YV3_SGD_MAXIMIZE  4

/* YV3_OPTIM_CHUNK, for callers that size the partials. */
int yv3_optim_chunk(void);

/* partials[k] = the fp64 sum of g^2 over chunk k, chunks numbered tensor by tensor (tensor i has ceil(n[i] / YV3_OPTIM_CHUNK)):
 * per thread in element order, then a fixed tree over the workgroup's threads.  YV3_EWORKSPACE if partials_cap (in doubles)
 * is smaller than the number of chunks. */
int yv3_grad_sumsq(const float* const* g, const long long* n, int count, double* partials, long long partials_cap, void* stream);

/* out[0] = total_norm = (float)sqrt(partials[0] + partials[1] + ..., in index order, fp64);
 * out[1] = coef = min(max_norm / (total_norm + 1e-6f), 1.0f) in fp32, NaN if the quotient is NaN.  count = 0 gives 0 and 1. */
int yv3_clip_coef(const double* partials, long long count, float max_norm, float* out, void* stream);

/* g = g * (*coef) for every tensor of the list; coef on the device. */
int yv3_grad_scale(float* const* g, const long long* n, int count, const float* coef, void* stream);

/* One SGD step on every (p, g, buf) of the list with one set of hyper-parameters; per element, each line one fp32 rounding:
 *   gs = coef ? g * (*coef) : g;  if MAXIMIZE: gs = -gs;         d = weight_decay != 0 ? gs + weight_decay * p : gs;
 *   if momentum != 0:  buf = FIRST ? d : momentum * buf + one_minus_dampening * d;   d = NESTEROV ? d + momentum * buf : buf;
 *   p = p + (-lr) * d.
 * g is not written.  buf may be NULL when momentum == 0; coef (device) may be NULL. */
int yv3_sgd_step(float* const* p, const float* const* g, float* const* buf, const long long* n, int count, const float* coef,
                 float lr, float momentum, float one_minus_dampening, float weight_decay, int flags, void* stream);

#define YV3_ADAM_FIRST     1  /* the first step of these parameters: exp_avg, exp_avg_sq, max_exp_avg_sq are +0 and not read */
#define YV3_ADAM_AMSGRAD   2
#define YV3_ADAM_MAXIMIZE  4
#define YV3_ADAM_DECOUPLED 8  /* AdamW: decay multiplies p; without it decay is the L2 coefficient added to g     */

/* One Adam / AdamW step (torch.optim.Adam, not capturable) on every (p, g, exp_avg m, exp_avg_sq v, max_exp_avg_sq vmax) of the
 * list with one set of scalars, which the caller reduces in double and rounds to fp32: w = 1 - beta1, beta2, one_minus_beta2,
 * sqrt_bc2 = sqrt(1 - beta2^step), eps, neg_step_size = -(lr / (1 - beta1^step)), and decay = 1 - lr * weight_decay with
 * DECOUPLED, weight_decay without (0: no decay).  Per element, each operation one fp32 rounding, no fused multiply-add, sqrt
 * and divide correctly rounded, denormals kept:
 *   gs = coef ? g * (*coef) : g;  if MAXIMIZE: gs = -gs;
 *   if DECOUPLED: p = p * decay;  else if decay != 0: gs = gs + decay * p;
 *   d = gs - m;   m = |w| < 0.5 ? m + w * d : gs - d * (1.0f - w);
 *   v = v * beta2;   v = v + (one_minus_beta2 * gs) * gs;
 *   s = v;  if AMSGRAD: s = vmax = vmax is NaN ? vmax : v is NaN ? v : vmax > v ? vmax : v;
 *   den = sqrt(s) / sqrt_bc2 + eps;   p = p + neg_step_size * (m / den).
 * g is not written.  max_exp_avg_sq may be NULL without AMSGRAD; coef (device) may be NULL.  The float4 path needs all of an
 * entry's pointers 16-byte aligned. */
int yv3_adam_step(float* const* p, const float* const* g, float* const* exp_avg, float* const* exp_avg_sq,
                  float* const* max_exp_avg_sq, const long long* n, int count, const float* coef, float w, float beta2,
                  float one_minus_beta2, float sqrt_bc2, float eps, float neg_step_size, float decay, int flags, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* YV3_H */
