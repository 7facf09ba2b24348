"""ctypes binding of libyv3.so (C-ABI declared in include/yv3.h).

The library is built in-tree by ``__graft_entry__.build()`` (``make -C yolo_v3_amd/csrc``).
There is deliberately no fallback: if the shared object is missing or a call fails, the
product path raises.  PyTorch is only used by callers for device memory and streams.
"""
import ctypes
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
# YV3_LIB (another build of the library: A/B variants, the -DYV3_MEASURE build) is honoured in measurement sessions only (YV3_MEASURE=1)
LIB_PATH = (os.environ.get("YV3_LIB") if os.environ.get("YV3_MEASURE") == "1" else None) or os.path.join(_HERE, "libyv3.so")

if os.environ.get("YV3_MEASURE") != "1":
    _stray = sorted(k for k in os.environ if k.startswith("YV3_") and k not in ("YV3_MEASURE", "YV3_DIST_BACKEND", "YV3_DUMP_PLAN"))
    if _stray:                      # (a user who points YV3_LIB at another build must learn that it is not loaded)
        import warnings
        warnings.warn("yolo_v3_amd: %s set but ignored -- library / kernel-selection overrides are honoured in measurement sessions only "
                      "(YV3_MEASURE=1); the bundled libyv3.so and the default plans are used" % ", ".join(_stray), RuntimeWarning)

F32, BF16, F32X3, F32H2 = 0, 1, 2, 3
BF16_ACT = 4          # net.backprop_math only: the BF16 training step with activations stored in bf16 only (backprop.py)
F16 = 5               # YV3_F16: one fp16 plane on the BF16 kernels (inference only)
I8 = 6                # YV3_I8: calibrated int8 activations and weights, int32 accumulation (inference only; needs net.int8_scales)
ACT_LINEAR, ACT_LEAKY = 0, 1
PP_EVAL, PP_PROB = 1, 2
OPT_NO_PINGPONG, OPT_K3S1, OPT_WINO_EVEN, OPT_WINO_ALWAYS, OPT_TWO_LANES, OPT_WINO4_TILES = 1, 2, 4, 8, 16, 32
OPT_TILE_SHIFT = 8
# The measurement codes of yv3_conv_desc (csrc/conv_select.h's enums without their YV3_ prefix; tests/test_host_logic.py compares name by name):
# forced tile (options bits 8..15), tune[0] and tune[1] of exact fp32, tune[1] of the plane kernels (a bit set)
(TILE_AUTO, TILE_256x128_W8, TILE_128x128_W8, TILE_128x128_W4, TILE_128x64, TILE_256x128_W4, TILE_256x256, TILE_256x128_W4_ROLL,
 TILE_256x256_ROLL, TILE_256x256_ROLL4) = range(10)
TILE_192x256_ROLL, TILE_W4_192x128, TILE_256x256_PP3, TILE_256x256_PP4, TILE_192x256_PP3, TILE_192x256_PP4 = 11, 12, 13, 14, 15, 16
T0_F32_TILE_64, T0_F32_TILE_128_W4, T0_F32_TILE_128_1X1, T0_WINO2_HALF, T0_WINO2_FULL = 2, 6, 7, 8, 9
T0_WINO4_NEVER, T0_WINO4_ALWAYS, T0_GEMM_NEVER, T0_GEMM_ALWAYS = 10, 11, 13, 14
T1_WINO4_NO_EVEN, T1_WINO4_NO_FULL, T1_GEMM_ALL_ROWS = 1, 2, 3
T1P_NO_SHORT_K, T1P_WINO_OTHER_LOOP, T1P_BF16_ROUND3, T1P_BF16_NO_192, T1P_NO_W4 = 1, 2, 8, 16, 32
T1P_NO_W4_1X1, T1P_NO_W4_3X3, T1P_W4_LANES_3X3, T1P_BF16_ROLL, T1P_BF16_PP3 = 64, 128, 256, 512, 1024
KERNEL_LINE_BYTES = 96


def conv2d_kernel(desc):
    """yv3_conv2d_kernel's line for a ConvDesc (raises on the YV3_E* code yv3_conv2d would return)."""
    buf = ctypes.create_string_buffer(KERNEL_LINE_BYTES)
    check(lib().yv3_conv2d_kernel(ctypes.byref(desc), buf, KERNEL_LINE_BYTES), "yv3_conv2d_kernel")
    return buf.value.decode()

c_void_p, c_int, c_float, c_size_t, c_longlong = (ctypes.c_void_p, ctypes.c_int, ctypes.c_float,
                                                  ctypes.c_size_t, ctypes.c_longlong)


class ConvDesc(ctypes.Structure):
    """struct yv3_conv_desc (include/yv3.h)."""
    _fields_ = [("x", c_void_p), ("x2", c_void_p), ("w", c_void_p), ("alpha", c_void_p), ("beta", c_void_p),
                ("residual", c_void_p), ("y", c_void_p),
                ("B", c_int), ("H", c_int), ("W", c_int), ("cin", c_int), ("cin_up", c_int),
                ("cout", c_int), ("cout_pad", c_int), ("k", c_int), ("stride", c_int), ("act", c_int),
                ("dtype", c_int), ("out_dtype", c_int), ("flags", c_void_p),
                ("workspace", c_void_p), ("workspace_bytes", ctypes.c_size_t),
                ("dec_out", c_void_p), ("dec_out_batch_stride", c_longlong), ("dec_stride", c_float),
                ("dec_anchors", c_float * 6), ("options", ctypes.c_uint), ("big_tile_min", c_int), ("tune", c_int * 4),
                ("x_plane_stride", c_longlong), ("x2_plane_stride", c_longlong), ("y_plane_stride", c_longlong),
                ("w_wino", c_void_p), ("alpha_wino", c_void_p), ("wino_ws", c_void_p), ("wino_ws_bytes", ctypes.c_size_t),
                ("w_wino4", c_void_p), ("s_res", c_float), ("inv_s_out", c_float)]


COCO_MAX_MAXDETS = 8
ELIMIT = -6


class CocoEvalDesc(ctypes.Structure):
    """struct yv3_cocoeval_desc (include/yv3.h)."""
    _fields_ = [("n_gt", c_int), ("n_det", c_int), ("n_img", c_int), ("n_cat", c_int),
                ("gt_img", c_void_p), ("gt_cat", c_void_p), ("gt_box", c_void_p), ("gt_area", c_void_p),
                ("gt_crowd", c_void_p), ("gt_id", c_void_p),
                ("det_img", c_void_p), ("det_cat", c_void_p), ("det_box", c_void_p), ("det_score", c_void_p),
                ("n_iou", c_int), ("n_rec", c_int), ("n_area", c_int), ("n_maxdet", c_int),
                ("iou_thrs", c_void_p), ("rec_thrs", c_void_p), ("area_rng", c_void_p),
                ("max_dets", c_int * COCO_MAX_MAXDETS),
                ("precision", c_void_p), ("recall", c_void_p), ("scores", c_void_p), ("status", c_void_p)]


YOLO_LOSS_MAX_ROWS = 1024
EINVAL, ESHAPE, EWORKSPACE = -1, -2, -3


class YoloLossDesc(ctypes.Structure):
    """struct yv3_yolo_loss_desc (include/yv3.h)."""
    _fields_ = [("logits", c_void_p), ("grad", c_void_p),
                ("stride_b", c_longlong), ("stride_p", c_longlong), ("stride_c", c_longlong),
                ("target", c_void_p), ("B", c_int), ("H", c_int), ("W", c_int), ("T", c_int), ("num_class", c_int),
                ("img_dim_h", c_float), ("anchors", c_float * 18), ("mask", c_int * 3),
                ("sums", c_void_p), ("counts", c_void_p), ("status", c_void_p)]


JPEG_OK, JPEG_NOT_JPEG, JPEG_MALFORMED, JPEG_PROGRESSIVE, JPEG_SOF, JPEG_PRECISION, JPEG_COMPONENTS = range(7)
JPEG_COLORSPACE, JPEG_SAMPLING, JPEG_MULTISCAN, JPEG_TABLES, JPEG_SIZE = range(7, 12)
(JPEG_S_INFO, JPEG_S_BOUNDS, JPEG_S_HUFFTABLE, JPEG_S_CODE, JPEG_S_OVERRUN, JPEG_S_COEF, JPEG_S_MARKER, JPEG_S_EXTRA,
 JPEG_S_DC, JPEG_S_RANGE) = range(1, 11)
# progressive files (the YV3_JPEGP_ names of include/yv3.h): the accept flag, the record's capacities, further reasons and statuses
JPEGP_ACCEPT, JPEGP_MAX_SCANS, JPEGP_MAX_TABLES = 1, 64, 66
JPEGP_SCAN, JPEGP_SCRIPT, JPEGP_CAPACITY, JPEGP_DQT = range(12, 16)
JPEGP_S_REFINE, JPEGP_S_VALUE = 11, 12


class JpegInfo(ctypes.Structure):
    """struct yv3_jpeg_info (include/yv3.h)."""
    _fields_ = [("scan_offset", c_longlong), ("scan_length", c_longlong),
                ("width", c_int), ("height", c_int), ("ncomp", c_int), ("restart_interval", c_int),
                ("reason", c_int), ("has_exif", c_int),
                ("h", ctypes.c_ubyte * 4), ("v", ctypes.c_ubyte * 4),
                ("tq", ctypes.c_ubyte * 4), ("td", ctypes.c_ubyte * 4), ("ta", ctypes.c_ubyte * 4),
                ("quant_defined", ctypes.c_ubyte * 4), ("huff_defined", ctypes.c_ubyte * 8),
                ("quant", ctypes.c_ubyte * 64 * 4), ("huff_counts", ctypes.c_ubyte * 16 * 8),
                ("huff_values", ctypes.c_ubyte * 256 * 8)]


class JpegBatchDesc(ctypes.Structure):
    """struct yv3_jpeg_batch_desc (include/yv3.h)."""
    _fields_ = [("src", c_void_p), ("src_bytes", c_longlong), ("src_offsets", c_void_p),
                ("infos", c_void_p), ("infos_host", c_void_p),
                ("dst", c_void_p), ("dst_bytes", c_longlong), ("dst_offsets", c_void_p),
                ("status", c_void_p), ("B", c_int)]


class JpegpScan(ctypes.Structure):
    """struct yv3_jpegp_scan (include/yv3.h)."""
    _fields_ = [("offset", c_longlong), ("length", c_longlong), ("restart_interval", c_int), ("pad0", c_int),
                ("ns", ctypes.c_ubyte), ("ss", ctypes.c_ubyte), ("se", ctypes.c_ubyte), ("ah", ctypes.c_ubyte), ("al", ctypes.c_ubyte),
                ("level", ctypes.c_ubyte), ("comp", ctypes.c_ubyte * 3), ("tab", ctypes.c_ubyte * 3), ("pad1", ctypes.c_ubyte * 4)]


class JpegpTable(ctypes.Structure):
    """struct yv3_jpegp_table (include/yv3.h)."""
    _fields_ = [("counts", ctypes.c_ubyte * 16), ("values", ctypes.c_ubyte * 256)]


class JpegProg(ctypes.Structure):
    """struct yv3_jpeg_prog (include/yv3.h)."""
    _fields_ = [("accepted", c_int), ("nscans", c_int), ("ntables", c_int), ("nlevels", c_int),
                ("scans", JpegpScan * JPEGP_MAX_SCANS), ("tables", JpegpTable * JPEGP_MAX_TABLES)]


class JpegBatchDescProg(ctypes.Structure):
    """struct yv3_jpeg_batch_desc_prog (include/yv3.h)."""
    _fields_ = [("base", JpegBatchDesc), ("progs", c_void_p), ("progs_host", c_void_p), ("prog_of", c_void_p),
                ("prog_of_host", c_void_p), ("P", c_int)]


JPEGE_444, JPEGE_422, JPEGE_420 = 0, 1, 2
JPEGE_S_INFO, JPEGE_S_BOUNDS, JPEGE_S_SPACE, JPEGE_S_RANGE = 1, 2, 3, 4


class JpegEncImage(ctypes.Structure):
    """struct yv3_jpeg_enc_image (include/yv3.h)."""
    _fields_ = [("pixels", c_void_p), ("pitch", c_longlong), ("out", c_void_p), ("out_cap", c_longlong),
                ("width", c_int), ("height", c_int), ("ncomp", c_int), ("subsampling", c_int), ("quality", c_int), ("reserved", c_int)]


class JpegEncDesc(ctypes.Structure):
    """struct yv3_jpeg_enc_desc (include/yv3.h)."""
    _fields_ = [("images", c_void_p), ("images_host", c_void_p), ("out_len", c_void_p), ("status", c_void_p), ("B", c_int)]


class DrawImage(ctypes.Structure):
    """struct yv3_draw_image (include/yv3.h)."""
    _fields_ = [("pixels", c_void_p), ("pitch", c_longlong), ("width", c_int), ("height", c_int), ("first_box", c_int), ("num_boxes", c_int)]


class DrawBox(ctypes.Structure):
    """struct yv3_draw_box (include/yv3.h)."""
    _fields_ = [("x1", c_int), ("y1", c_int), ("x2", c_int), ("y2", c_int), ("tag", c_int), ("rgb", ctypes.c_ubyte * 3), ("reserved", ctypes.c_ubyte)]


class DrawTag(ctypes.Structure):
    """struct yv3_draw_tag (include/yv3.h)."""
    _fields_ = [("offset", c_longlong), ("width", c_int), ("height", c_int)]


class AffineProgram(ctypes.Structure):
    """struct yv3_affine_program (include/yv3.h)."""
    _fields_ = [("active", c_int), ("reserved", c_int), ("fwd", ctypes.c_double * 6), ("inv", ctypes.c_double * 6)]


_SIGNATURES = {
    "yv3_version": (c_int, []),
    "yv3_conv_workspace_bytes": (ctypes.c_size_t, []),
    "yv3_wino_workspace_bytes": (ctypes.c_size_t, [c_int, c_int, c_int, c_int]),
    "yv3_wino4_workspace_bytes": (ctypes.c_size_t, [c_int, c_int, c_int, c_int]),
    "yv3_pack_wino4_weight_f32": (c_int, [c_void_p, c_void_p, c_int, c_int, c_void_p]),
    "yv3_error_string": (ctypes.c_char_p, [c_int]),
    "yv3_pack_conv_weight": (c_int, [c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int, c_void_p]),
    "yv3_fold_bn": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_float, c_void_p, c_void_p, c_int, c_void_p]),
    "yv3_split_planes": (c_int, [c_void_p, c_void_p, c_longlong, c_int, c_void_p]),
    "yv3_merge_planes": (c_int, [c_void_p, c_void_p, c_longlong, c_int, c_void_p]),
    "yv3_split_plane_f16": (c_int, [c_void_p, c_void_p, c_longlong, c_void_p]),
    "yv3_quantize_bf16_i8": (c_int, [c_void_p, c_void_p, c_longlong, c_float, c_void_p]),
    "yv3_merge_plane_f16": (c_int, [c_void_p, c_void_p, c_longlong, c_void_p]),
    "yv3_conv0": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_void_p, c_void_p]),
    "yv3_conv_front": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_void_p, c_void_p]),
    "yv3_conv_front_bf16": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_void_p, c_void_p]),
    "yv3_res_block64": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_void_p, c_void_p]),
    "yv3_res_block64_bf16": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_void_p, c_void_p]),
    "yv3_conv_front_f16": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_void_p, c_void_p]),
    "yv3_res_block64_f16": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_void_p, c_void_p]),
    "yv3_conv_front_f32": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_void_p]),
    "yv3_res_block64_f32": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_void_p]),
    "yv3_conv2d": (c_int, [ctypes.POINTER(ConvDesc), c_void_p]),
    "yv3_conv2d_form": (c_int, [ctypes.POINTER(ConvDesc)]),
    "yv3_conv2d_launches": (c_int, [ctypes.POINTER(ConvDesc)]),
    "yv3_conv2d_kernel": (c_int, [ctypes.POINTER(ConvDesc), ctypes.c_char_p, c_size_t]),
    "yv3_conv2d_sequence": (c_int, [ctypes.POINTER(ConvDesc), c_int, c_void_p]),
    "yv3_decode": (c_int, [c_void_p, c_int, ctypes.POINTER(c_float), c_float, c_void_p, c_longlong,
                           c_int, c_int, c_int, c_int, c_void_p]),
    "yv3_decode_nchw": (c_int, [c_void_p, ctypes.POINTER(c_float), c_float, c_void_p, c_longlong,
                                c_int, c_int, c_int, c_int, c_void_p]),
    "yv3_decode_bwd_nchw": (c_int, [c_void_p, c_void_p, ctypes.POINTER(c_float), c_float, c_void_p,
                                    c_int, c_int, c_int, c_int, c_void_p]),
    "yv3_cxcywh_to_xyxy": (c_int, [c_void_p, c_void_p, c_longlong, c_void_p]),
    "yv3_iou_matrix": (c_int, [c_void_p, c_int, c_int, c_void_p, c_int, c_int, c_int, c_void_p, c_void_p]),
    "yv3_letterbox": (c_int, [c_void_p, c_int, c_int, c_void_p, c_int, c_int, c_void_p]),
    "yv3_letterbox_ex": (c_int, [c_void_p, c_int, c_int, c_void_p, c_int, c_int, c_int, c_int, c_int, c_int, c_void_p]),
    "yv3_resize_linear": (c_int, [c_void_p, c_int, c_int, c_void_p, c_int, c_int, c_void_p]),
    "yv3_augment_workspace_bytes": (c_size_t, [c_longlong]),
    "yv3_augment_images": (c_int, [c_void_p, c_longlong, c_void_p, c_void_p, c_void_p, c_int, c_void_p, c_int, c_int,
                                   c_void_p, c_size_t, c_void_p, c_void_p]),
    "yv3_augment_images_from": (c_int, [c_void_p, c_longlong, c_void_p, c_void_p, c_longlong, c_void_p, c_void_p, c_int, c_void_p,
                                        c_int, c_int, c_void_p, c_size_t, c_void_p, c_void_p]),
    "yv3_augment_labels": (c_int, [c_void_p, c_int, c_int, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_void_p, c_void_p]),
    "yv3_extra_augment_workspace_bytes": (c_size_t, [c_longlong]),
    "yv3_extra_augment": (c_int, [c_void_p, c_longlong, c_void_p, c_void_p, c_void_p, c_int, c_void_p, c_longlong, c_void_p,
                                  c_void_p, c_size_t, c_void_p, c_void_p]),
    "yv3_affine_augment": (c_int, [c_void_p, c_longlong, c_void_p, c_void_p, c_void_p, c_int, c_void_p, c_longlong, c_void_p,
                                   c_void_p, c_void_p]),
    "yv3_affine_labels": (c_int, [c_void_p, c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "yv3_upsample2x_concat": (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int, c_void_p]),
    "yv3_correct_boxes": (c_int, [c_void_p, c_int, c_int, c_int, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_void_p, c_void_p]),
    "yv3_gather_boxes": (c_int, [c_void_p, c_void_p, c_int, c_int, c_void_p, c_void_p]),
    "yv3_postproc_cand_bytes": (c_size_t, [c_int, c_int, c_int]),
    "yv3_postproc_nms_workspace_bytes": (c_size_t, [c_int, c_int, c_int]),
    "yv3_postproc_filter": (c_int, [c_void_p, c_int, c_int, c_int, c_float, c_int, c_void_p, c_int, c_void_p, c_void_p]),
    "yv3_postproc_nms": (c_int, [c_void_p, c_int, c_int, c_int, c_float, c_int, c_void_p, c_int, c_void_p, c_int,
                                 c_void_p, c_int, c_void_p, c_void_p, c_size_t, c_void_p]),
    "yv3_cocoeval_workspace_bytes": (c_size_t, [c_int, c_int, c_int, c_int, c_int]),
    "yv3_cocoeval": (c_int, [ctypes.POINTER(CocoEvalDesc), c_void_p, c_size_t, c_void_p]),
    "yv3_yolo_loss_workspace_bytes": (c_size_t, [c_int, c_int, c_int, c_int]),
    "yv3_yolo_loss": (c_int, [ctypes.POINTER(YoloLossDesc), c_void_p, c_size_t, c_void_p]),
    "yv3_train_pack_weight": (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_void_p]),
    "yv3_train_conv_fwd": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p] + [c_int] * 9 + [c_void_p]),
    "yv3_train_conv_dgrad": (c_int, [c_void_p, c_void_p, c_void_p] + [c_int] * 8 + [c_void_p]),
    "yv3_train_conv0_dgrad": (c_int, [c_void_p, c_void_p, c_void_p] + [c_int] * 4 + [c_void_p]),
    "yv3_train_conv_wgrad_workspace_bytes": (c_size_t, [c_int] * 7),
    "yv3_train_conv_wgrad": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p] + [c_int] * 9 + [c_void_p, c_size_t, c_void_p]),
    "yv3_train_channel_workspace_bytes": (c_size_t, [c_longlong, c_int]),
    "yv3_train_bn_stats": (c_int, [c_void_p, c_longlong, c_int, c_float, c_float] + [c_void_p] * 7 + [c_size_t, c_void_p]),
    "yv3_train_bn_eval_stats": (c_int, [c_void_p, c_void_p, c_float, c_void_p, c_void_p, c_int, c_void_p]),
    "yv3_train_bn_act_fwd": (c_int, [c_void_p] * 7 + [c_longlong, c_int, c_void_p]),
    "yv3_train_bn_act_bwd": (c_int, [c_void_p] * 9 + [c_longlong, c_int, c_int, c_void_p, c_size_t, c_void_p]),
    "yv3_train_bias_bwd": (c_int, [c_void_p] * 4 + [c_longlong, c_int, c_void_p, c_size_t, c_void_p]),
    "yv3_train_add": (c_int, [c_void_p, c_void_p, c_longlong, c_void_p]),
    "yv3_train_upcat_bwd": (c_int, [c_void_p] * 3 + [c_int] * 7 + [c_void_p]),
    "yv3_train_to_bf16": (c_int, [c_void_p, c_void_p, c_longlong, c_int, c_int, c_void_p]),
    "yv3_train_conv_fwd_bf16o": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p] + [c_int] * 9 + [c_void_p]),
    "yv3_jpeg_parse": (c_int, [c_void_p, c_size_t, ctypes.POINTER(JpegInfo)]),
    "yv3_jpeg_workspace_bytes": (c_size_t, [c_void_p, c_int]),
    "yv3_jpeg_decode_batch": (c_int, [ctypes.POINTER(JpegBatchDesc), c_void_p, c_size_t, c_void_p]),
    "yv3_jpeg_workspace_bytes_ex": (c_size_t, [c_void_p, c_int, c_int]),
    "yv3_jpeg_decode_batch_ex": (c_int, [ctypes.POINTER(JpegBatchDesc), c_int, c_void_p, c_void_p, c_size_t, c_void_p]),
    "yv3_jpeg_parse_ex": (c_int, [c_void_p, c_size_t, c_int, ctypes.POINTER(JpegInfo), ctypes.POINTER(JpegProg)]),
    "yv3_jpeg_workspace_bytes_prog": (c_size_t, [c_void_p, c_void_p, c_void_p, c_int, c_int, c_int]),
    "yv3_jpeg_decode_batch_prog": (c_int, [ctypes.POINTER(JpegBatchDescProg), c_int, c_void_p, c_void_p, c_size_t, c_void_p]),
    "yv3_jpeg_launch_count": (c_longlong, []),
    "yv3_jpeg_encode_header": (c_longlong, [c_int, c_int, c_int, c_int, c_int, c_void_p, c_longlong]),
    "yv3_jpeg_encode_bound": (c_longlong, [c_int, c_int, c_int, c_int]),
    "yv3_jpeg_encode_workspace_bytes": (c_size_t, [c_void_p, c_int]),
    "yv3_jpeg_encode_batch": (c_int, [ctypes.POINTER(JpegEncDesc), c_void_p, c_size_t, c_void_p]),
    "yv3_draw_boxes": (c_int, [c_void_p, c_int, c_void_p, c_int, c_void_p, c_int, c_void_p, c_longlong, c_int, c_int, c_int, c_void_p]),
    "yv3_optim_chunk": (c_int, []),
    "yv3_grad_sumsq": (c_int, [c_void_p, c_void_p, c_int, c_void_p, c_longlong, c_void_p]),
    "yv3_clip_coef": (c_int, [c_void_p, c_longlong, c_float, c_void_p, c_void_p]),
    "yv3_grad_scale": (c_int, [c_void_p, c_void_p, c_int, c_void_p, c_void_p]),
    "yv3_sgd_step": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_void_p, c_float, c_float, c_float, c_float, c_int, c_void_p]),
    "yv3_adam_step": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_void_p,
                              c_float, c_float, c_float, c_float, c_float, c_float, c_float, c_int, c_void_p]),
}
# a _bf16 twin takes its base entry's arguments, with bf16 tensors where the base has fp32 ones (all void* here)
_SIGNATURES.update({twin: _SIGNATURES[twin.replace("_bf16", "")] for twin in (
    "yv3_train_pack_weight_bf16", "yv3_train_conv_fwd_bf16", "yv3_train_conv_dgrad_bf16", "yv3_train_conv0_dgrad_bf16",
    "yv3_train_conv_wgrad_bf16_workspace_bytes", "yv3_train_conv_wgrad_bf16", "yv3_train_channel_bf16_workspace_bytes",
    "yv3_train_bn_stats_bf16", "yv3_train_bn_act_fwd_bf16", "yv3_train_bn_act_bwd_bf16", "yv3_train_bias_bwd_bf16")})

EXPORTS = tuple(_SIGNATURES)
_lib = None


class Yv3Error(RuntimeError):
    code = None          # the YV3_E* code (or hipError_t) behind the error, when it came from the library


class GpuOnlyError(Yv3Error, NotImplementedError):
    """A CPU tensor where only the GPU path exists (the reference's training branch runs on CPU tensors; this package does not)."""


def lib():
    """Load libyv3.so once; raise if it has not been built."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise Yv3Error("HIP extension %s is missing: build it with "
                           "`python -c 'import __graft_entry__ as g; g.build()'` "
                           "(or `make -C yolo_v3_amd/csrc`). There is no CPU fallback." % LIB_PATH)
        handle = ctypes.CDLL(LIB_PATH)
        for name, (res, args) in _SIGNATURES.items():
            fn = getattr(handle, name)
            fn.restype = res
            fn.argtypes = args
        _lib = handle
    return _lib


def check(rc, what=""):
    if rc != 0:
        msg = lib().yv3_error_string(rc).decode()
        err = Yv3Error("%s failed: %s (code %d)" % (what or "libyv3 call", msg, rc))
        err.code = rc
        raise err


def stream_ptr():
    """hipStream_t of torch's current stream on the current device."""
    import torch
    return torch.cuda.current_stream().cuda_stream


def require_cuda(t, name="tensor"):
    if not t.is_cuda:
        raise Yv3Error("%s must live on the GPU: this package runs only on MI355X (HIP kernels), "
                       "there is no CPU path" % name)
    return t
