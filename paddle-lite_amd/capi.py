"""ctypes binding of libplhip.so (include/plhip.h) — the only way Python reaches the device code.

There is deliberately NO fallback: if the HIP library is missing or a call fails this raises.
Used by tests/ (parity checks through the C ABI), bench.py and __graft_entry__.py.
"""
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("PLHIP_LIB_PATH") or os.path.join(_HERE, "libplhip.so")  # override: diagnostic builds only (tools/slp_hazard_variants.py)

OUT_I32, OUT_F32, OUT_I8 = 0, 1, 2
OUT_F32_GAP = 3  # plhip_dwpw_fused_int8 only: the fp32 output averaged over each plane, [n][cout]
ACT_NONE, ACT_RELU, ACT_RELU6, ACT_LEAKY = 0, 1, 2, 4
_OUT_DTYPE = {OUT_I32: np.int32, OUT_F32: np.float32, OUT_I8: np.int8}

# every symbol include/plhip.h declares (tests check that the library exports all of them)
EXPORTS = [
    "plhip_device_count", "plhip_ctx_create", "plhip_ctx_create_on_stream", "plhip_ctx_destroy",
    "plhip_ctx_stream", "plhip_last_error", "plhip_malloc", "plhip_free", "plhip_memcpy_h2d",
    "plhip_memcpy_d2h", "plhip_memcpy_d2d", "plhip_memset", "plhip_stream_sync", "plhip_event_create",
    "plhip_event_record", "plhip_event_elapsed_ms", "plhip_event_destroy",
    "plhip_conv_packed_weight_bytes", "plhip_pack_conv_weights", "plhip_conv_workspace_bytes",
    "plhip_deconv_out_dims", "plhip_deconv_packed_weight_bytes", "plhip_pack_deconv_weights", "plhip_conv2d_transpose_int8",
    "plhip_deconv_impl_name",
    "plhip_conv2d_int8", "plhip_conv2d_int8_fused", "plhip_conv2d_fused_supported", "plhip_conv_impl_name", "plhip_depthwise_conv_int8", "plhip_dwpw_fused_int8", "plhip_dwpw_fused_supported", "plhip_dw_conv1x1_fused_int8", "plhip_dw_conv1x1_fused_supported", "plhip_graph_begin", "plhip_graph_end", "plhip_graph_launch", "plhip_graph_destroy",
    "plhip_fc_packed_weight_bytes", "plhip_pack_fc_weights", "plhip_fc_int8",
    "plhip_calib_f32_to_i8", "plhip_calib_i8_to_f32", "plhip_global_avg_pool_f32", "plhip_softmax_f32",
    "plhip_pool2d_f32", "plhip_pool2d_max_i8", "plhip_elementwise_add_f32", "plhip_selftest",
    "plhip_debug_set", "plhip_debug_dw_plan", "plhip_conv2d_calib_supported", "plhip_conv2d_calib_int8",
    "plhip_image_to_tensor_f32", "plhip_image_to_tensor_i8", "plhip_conv2d_image_supported", "plhip_conv2d_image_int8",
    "plhip_image_resize_tables", "plhip_image_convert_u8", "plhip_image_resize_u8", "plhip_frame_to_tensor_f32", "plhip_frame_to_tensor_i8",
    "plhip_hard_act_f32", "plhip_se_scale_f32",
    "plhip_se_gate_supported", "plhip_se_gate_packed_weight_bytes", "plhip_pack_se_gate_weights", "plhip_se_gate_int8",
    "plhip_concat_f32", "plhip_split_f32", "plhip_shuffle_channel_f32", "plhip_shuffle_unit_f32",
    "plhip_concat_calib_f32",
    "plhip_interp_f32", "plhip_arg_max_f32", "plhip_interp_argmax_f32",
    "plhip_transpose_f32", "plhip_concat_nhwc_f32", "plhip_box_coder_decode_f32",
    "plhip_multiclass_nms_workspace_bytes", "plhip_multiclass_nms_f32",
    "plhip_yolo_box_f32", "plhip_yolo_head_f32",
]

# plhip_hard_act_kind, and the reference's default parameters (lite/operators/op_params.h:406-412)
HARD_SWISH, HARD_SIGMOID = 0, 1
HARD_SWISH_DEFAULTS = (6.0, 6.0, 3.0)   # threshold, scale, offset
HARD_SIGMOID_DEFAULTS = (0.2, 0.5)      # slope, offset

# plhip_interp_method; the arg_max output dtypes (ArgmaxParam::dtype: -1 and 3 are int64, 2 is int32)
INTERP_BILINEAR, INTERP_NEAREST = 0, 1
INTERP_METHODS = {"bilinear": INTERP_BILINEAR, "nearest": INTERP_NEAREST}
ARGMAX_DTYPES = {-1: np.int64, 3: np.int64, 2: np.int32}

# plhip_image_format == cv::ImageFormat (lite/utils/cv/paddle_image_preprocess.h)
IMG_RGBA, IMG_BGRA, IMG_RGB, IMG_BGR, IMG_GRAY = 0, 1, 2, 3, 4
IMG_NV21, IMG_NV12 = 11, 12  # frame formats only (plhip_frame_desc): lite/utils/cv/cv_enum.h
IMG_BYTES = {IMG_RGBA: 4, IMG_BGRA: 4, IMG_RGB: 3, IMG_BGR: 3, IMG_GRAY: 1}      # bytes a pixel of the interleaved image has
IMG_CHANNELS = {IMG_RGBA: 3, IMG_BGRA: 3, IMG_RGB: 3, IMG_BGR: 3, IMG_GRAY: 1}   # channels of the NCHW tensor made from it


class ConvDesc(C.Structure):
    _fields_ = [("n", C.c_int), ("cin", C.c_int), ("h", C.c_int), ("w", C.c_int),
                ("cout", C.c_int), ("kh", C.c_int), ("kw", C.c_int),
                ("pad", C.c_int * 4), ("stride", C.c_int * 2), ("dil", C.c_int * 2),
                ("groups", C.c_int), ("act", C.c_int), ("act_alpha", C.c_float)]


class DeconvDesc(C.Structure):
    _fields_ = [("conv", ConvDesc), ("out_h", C.c_int), ("out_w", C.c_int)]


class PoolDesc(C.Structure):
    _fields_ = [("planes", C.c_int), ("h", C.c_int), ("w", C.c_int), ("oh", C.c_int), ("ow", C.c_int),
                ("kh", C.c_int), ("kw", C.c_int), ("pad", C.c_int * 4), ("stride", C.c_int * 2),
                ("is_max", C.c_int), ("exclusive", C.c_int)]


class ImageDesc(C.Structure):
    _fields_ = [("n", C.c_int), ("h", C.c_int), ("w", C.c_int), ("format", C.c_int),
                ("means", C.c_float * 3), ("scales", C.c_float * 3)]


def image_desc(n, h, w, fmt, means, scales):
    """plhip_image_desc; means / scales: one value per source byte of a pixel (the first only for GRAY)."""
    d = ImageDesc()
    d.n, d.h, d.w, d.format = n, h, w, fmt
    m, s = list(means) + [0.0] * (3 - len(means)), list(scales) + [0.0] * (3 - len(scales))
    d.means[:] = [float(v) for v in m[:3]]
    d.scales[:] = [float(v) for v in s[:3]]
    return d


class SeGateDesc(C.Structure):
    _fields_ = [("n", C.c_int), ("c", C.c_int), ("cr", C.c_int), ("calib_scale", C.c_float), ("act1", C.c_int), ("act2", C.c_int),
                ("act1_alpha", C.c_float), ("act2_alpha", C.c_float), ("slope", C.c_float), ("offset", C.c_float)]


class NmsDesc(C.Structure):
    _fields_ = [("n", C.c_int), ("c", C.c_int), ("p", C.c_int), ("score_stride_class", C.c_int64), ("score_stride_prior", C.c_int64),
                ("background_label", C.c_int), ("score_threshold", C.c_float), ("nms_top_k", C.c_int), ("nms_threshold", C.c_float),
                ("nms_eta", C.c_float), ("keep_top_k", C.c_int), ("normalized", C.c_int)]


def nms_desc(n, c, p, background_label, score_threshold, nms_top_k, nms_threshold, keep_top_k, normalized=True, nms_eta=1.0,
             layout="ncp"):
    """plhip_nms_desc; layout: "ncp" scores [N, C, P] (strides P, 1) or "npc" scores [N, P, C] (strides 1, C)."""
    d = NmsDesc()
    d.n, d.c, d.p = int(n), int(c), int(p)
    d.score_stride_class, d.score_stride_prior = {"ncp": (int(p), 1), "npc": (1, int(c))}[layout]
    d.background_label, d.score_threshold, d.nms_top_k = int(background_label), float(score_threshold), int(nms_top_k)
    d.nms_threshold, d.nms_eta, d.keep_top_k, d.normalized = float(nms_threshold), float(nms_eta), int(keep_top_k), int(bool(normalized))
    return d


class FrameDesc(C.Structure):
    _fields_ = [("n", C.c_int), ("h", C.c_int), ("w", C.c_int), ("format", C.c_int)]


def frame_desc(n, h, w, fmt):
    """plhip_frame_desc: n frames of h x w in an interleaved IMG_* format ([n, h, w, cs] bytes) or IMG_NV12 / IMG_NV21
    ([n, h * 3 / 2, w] bytes)."""
    d = FrameDesc()
    d.n, d.h, d.w, d.format = n, h, w, fmt
    return d


def resize_tables(n_in, n_out):
    """plhip_image_resize_tables for one axis (host only): (ofs int32 [n_out], coef int16 [n_out, 2]), or None when refused."""
    L = load()
    ofs, coef = np.zeros(max(n_out, 1), np.int32), np.zeros((max(n_out, 1), 2), np.int16)
    if L.plhip_image_resize_tables(int(n_in), int(n_out), ofs.ctypes.data_as(C.c_void_p), coef.ctypes.data_as(C.c_void_p)) != 0:
        return None
    return ofs, coef


def conv_desc(n, cin, h, w, cout, kh, kw, pad=(0, 0, 0, 0), stride=(1, 1), dil=(1, 1), groups=1,
              act=ACT_NONE, alpha=0.0):
    d = ConvDesc()
    d.n, d.cin, d.h, d.w, d.cout, d.kh, d.kw = n, cin, h, w, cout, kh, kw
    if len(pad) == 2:
        pad = (pad[0], pad[0], pad[1], pad[1])
    d.pad[:] = [int(p) for p in pad]
    d.stride[:] = [int(s) for s in stride]
    d.dil[:] = [int(s) for s in dil]
    d.groups, d.act, d.act_alpha = groups, act, alpha
    return d


def deconv_desc(n, cin, h, w, cout, kh, kw, pad=(0, 0, 0, 0), stride=(1, 1), dil=(1, 1), groups=1, act=ACT_NONE, alpha=0.0,
                output_size=(0, 0)):
    """plhip_deconv_desc: conv_desc's fields with cout the OUTPUT channels (filter [cin][cout / groups][kh][kw]) and
    output_size (0 = the default of that dimension)."""
    d = DeconvDesc()
    d.conv = conv_desc(n, cin, h, w, cout, kh, kw, pad, stride, dil, groups, act, alpha)
    d.out_h, d.out_w = int(output_size[0]), int(output_size[1])
    return d


def deconv_out_hw(d):
    """plhip_deconv_out_dims (host only); raises PlhipError with the library's text for a descriptor it refuses."""
    L = load()
    oh, ow = C.c_int(), C.c_int()
    st = L.plhip_deconv_out_dims(C.byref(d), C.byref(oh), C.byref(ow))
    if st != 0:
        raise PlhipError("plhip_deconv_out_dims failed (%d): %s" % (st, L.plhip_last_error(None).decode()))
    return oh.value, ow.value


def deconv_impl_name(d):
    return load().plhip_deconv_impl_name(C.byref(d)).decode()


def out_hw(d):
    keh = d.dil[0] * (d.kh - 1) + 1
    kew = d.dil[1] * (d.kw - 1) + 1
    return (int((d.h + d.pad[0] + d.pad[1] - keh) / d.stride[0]) + 1,
            int((d.w + d.pad[2] + d.pad[3] - kew) / d.stride[1]) + 1)


class PlhipError(RuntimeError):
    pass


_lib = None
# Diagnostic knobs this PROCESS set through plhip_debug_set (the library itself never reads the environment).  The binding
# forwards PLHIP_<KNOB>=<int> variables of the A/B scripts (tools/*.sh) explicitly and records them here;
# bench.py prints the dict in its JSON line, so a measurement taken with a knob says so.  The same keys, in the same order, as
# the library's knob table (plhip_capi_ctx.hip); STAMPS exists in a `make EXPERIMENTS=1` build only, a default one refuses it.
KNOBS = ("STEM_MFMA", "CONV_PATCH", "CONV_PATCH_S2", "STEM7", "DW_STAGE", "DW_STAGE_NP2", "DW_FASTV", "DW5_DIRECT", "DW_RS1",
         "DW_RS2", "GEMM_VARIANT", "GEMM_AREG", "GEMM_MA", "SUBSAMPLE_1X1", "GEMM_TR", "TR_CFG", "GEMM_WIDE", "WIDE_NTT", "FC_MFMA",
         "IMPLICIT_GEMM", "FUSED_STREAM", "FUSED_SMALL", "DWCONV_FUSED", "CONV_GROUPED", "DECONV_ROUTE", "STAMPS")
KNOBS_SET = {}


TAIL_RESIDUAL, TAIL_INT8_COPY, TAIL_NO_F32, TAIL_UNALIGNED, TAIL_X_UNALIGNED = 1, 2, 4, 8, 16


def gemm_plan_text(d, out, tail=0):
    """The GEMM launch plan (csrc/gemm_plan.h) the library makes for conv descriptor d with output kind `out` and the fused tail
    `tail` (TAIL_* bits) under the knobs in force: 'name family=... grid=... lds=...'.  Pointers are assumed aligned unless
    TAIL_UNALIGNED says that an output or the residual is off its vector alignment, TAIL_X_UNALIGNED that the input of a 1x1
    conv is off a dword.  '' for a conv on a non-GEMM route.  Host
    only: launches nothing, needs no context."""
    buf = C.create_string_buffer(512)
    if load().plhip_debug_gemm_plan(C.byref(d), int(out), int(tail), buf, len(buf)) < 0:
        raise PlhipError("plhip_debug_gemm_plan: bad conv descriptor")
    return buf.value.decode()


def patch_plan_text(d):
    """The patch kernel's launch plan (conv_patch_plan, csrc/conv_patch_i8.hip) of conv descriptor d on one of the two patch
    routes: 'patch_stat_a glob=... TPI=... pitch=...'.  '' for a conv on another route.  Host only."""
    buf = C.create_string_buffer(512)
    if load().plhip_debug_patch_plan(C.byref(d), buf, len(buf)) < 0:
        raise PlhipError("plhip_debug_patch_plan: bad conv descriptor")
    return buf.value.decode()


DW_PLAN_DEPTHWISE, DW_PLAN_PAIR_D, DW_PLAN_PAIR_G = 0, 1, 2


def dw_plan_text(d, kind, pw_cout=0, out=2, has_tail=0, x_aligned=1):
    """The launch plan (csrc/dw_plan.h) the library makes for depthwise descriptor d as a depthwise conv, a fused depthwise ->
    pointwise pair or a fused depthwise -> 1x1 conv (DW_PLAN_*) under the knobs in force: 'name KS=... grid=... lds=... | ...', or
    'none why=...'.  Host only: launches nothing, needs no context."""
    buf = C.create_string_buffer(768)
    if load().plhip_debug_dw_plan(C.byref(d), int(kind), int(pw_cout), int(out), int(has_tail), int(x_aligned), buf, len(buf)) < 0:
        raise PlhipError("plhip_debug_dw_plan: bad kind")
    return buf.value.decode()


def load():
    """dlopen libplhip.so and declare prototypes.  Raises if the library is absent (no CPU fallback)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise PlhipError("%s is missing: build it with __graft_entry__.build() (hipcc --offload-arch=gfx950)" % LIB_PATH)
    L = C.CDLL(LIB_PATH)
    vp, i32, f32, sz = C.c_void_p, C.c_int, C.c_float, C.c_size_t
    L.plhip_device_count.restype = i32
    L.plhip_debug_set.argtypes = [C.c_char_p, i32]
    L.plhip_debug_set.restype = i32
    for k in KNOBS:
        v = os.environ.get("PLHIP_" + k)
        if v is not None:
            if L.plhip_debug_set(k.encode(), int(v)) != 0:
                raise PlhipError("unknown diagnostic knob %s" % k)
            KNOBS_SET[k] = int(v)
    if KNOBS_SET:
        import sys
        sys.stderr.write("capi: diagnostic knobs set from the environment: %s\n" % KNOBS_SET)
    L.plhip_ctx_create.argtypes = [i32, C.POINTER(vp)]
    L.plhip_ctx_create_on_stream.argtypes = [i32, vp, C.POINTER(vp)]
    L.plhip_ctx_destroy.argtypes = [vp]
    L.plhip_ctx_destroy.restype = None
    L.plhip_ctx_stream.argtypes = [vp]
    L.plhip_ctx_stream.restype = vp
    L.plhip_last_error.argtypes = [vp]
    L.plhip_last_error.restype = C.c_char_p
    L.plhip_malloc.argtypes = [vp, sz, C.POINTER(vp)]
    L.plhip_free.argtypes = [vp, vp]
    L.plhip_memcpy_h2d.argtypes = [vp, vp, vp, sz]
    L.plhip_memcpy_d2h.argtypes = [vp, vp, vp, sz]
    L.plhip_memcpy_d2d.argtypes = [vp, vp, vp, sz]
    L.plhip_memset.argtypes = [vp, vp, i32, sz]
    L.plhip_stream_sync.argtypes = [vp]
    L.plhip_event_create.argtypes = [vp, C.POINTER(vp)]
    L.plhip_event_record.argtypes = [vp, vp]
    L.plhip_event_elapsed_ms.argtypes = [vp, vp, vp, C.POINTER(f32)]
    L.plhip_event_destroy.argtypes = [vp, vp]
    L.plhip_conv_packed_weight_bytes.argtypes = [C.POINTER(ConvDesc)]
    L.plhip_conv_packed_weight_bytes.restype = sz
    L.plhip_pack_conv_weights.argtypes = [vp, C.POINTER(ConvDesc), vp, vp]
    L.plhip_conv_workspace_bytes.argtypes = [C.POINTER(ConvDesc)]
    L.plhip_conv_workspace_bytes.restype = sz
    L.plhip_conv2d_int8.argtypes = [vp, C.POINTER(ConvDesc), vp, vp, vp, vp, vp, i32, vp, sz]
    L.plhip_conv2d_int8_fused.argtypes = [vp, C.POINTER(ConvDesc), vp, vp, vp, vp, vp, vp, i32, vp, f32, vp, sz]
    L.plhip_conv2d_calib_supported.argtypes = [C.POINTER(ConvDesc)]
    L.plhip_conv2d_fused_supported.argtypes = [C.POINTER(ConvDesc)]
    L.plhip_conv2d_calib_int8.argtypes = [vp, C.POINTER(ConvDesc), vp, f32, vp, vp, vp, vp, i32]
    L.plhip_deconv_out_dims.argtypes = [C.POINTER(DeconvDesc), C.POINTER(i32), C.POINTER(i32)]
    L.plhip_deconv_packed_weight_bytes.argtypes = [C.POINTER(DeconvDesc)]
    L.plhip_deconv_packed_weight_bytes.restype = sz
    L.plhip_pack_deconv_weights.argtypes = [vp, C.POINTER(DeconvDesc), vp, vp]
    L.plhip_conv2d_transpose_int8.argtypes = [vp, C.POINTER(DeconvDesc), vp, vp, vp, vp, vp, i32]
    L.plhip_deconv_impl_name.argtypes = [C.POINTER(DeconvDesc)]
    L.plhip_deconv_impl_name.restype = C.c_char_p
    L.plhip_image_to_tensor_f32.argtypes = [vp, C.POINTER(ImageDesc), vp, vp]
    L.plhip_image_to_tensor_i8.argtypes = [vp, C.POINTER(ImageDesc), vp, vp, f32]
    L.plhip_image_resize_tables.argtypes = [i32, i32, vp, vp]
    L.plhip_image_resize_tables.restype = i32
    L.plhip_image_convert_u8.argtypes = [vp, C.POINTER(FrameDesc), vp, i32, vp]
    L.plhip_image_resize_u8.argtypes = [vp, C.POINTER(FrameDesc), vp, i32, i32, vp]
    L.plhip_frame_to_tensor_f32.argtypes = [vp, C.POINTER(FrameDesc), C.POINTER(ImageDesc), vp, vp]
    L.plhip_frame_to_tensor_i8.argtypes = [vp, C.POINTER(FrameDesc), C.POINTER(ImageDesc), vp, vp, f32]
    L.plhip_conv2d_image_supported.argtypes = [C.POINTER(ConvDesc), C.POINTER(ImageDesc)]
    L.plhip_conv2d_image_supported.restype = i32
    L.plhip_conv2d_image_int8.argtypes = [vp, C.POINTER(ConvDesc), C.POINTER(ImageDesc), vp, f32, vp, vp, vp, vp, i32]
    L.plhip_conv_impl_name.argtypes = [C.POINTER(ConvDesc)]
    L.plhip_conv_impl_name.restype = C.c_char_p
    # diagnostics outside include/plhip.h: the GEMM launch plan of a conv as text (gemm_plan_text below), the wide tile override
    L.plhip_debug_gemm_plan.argtypes = [C.POINTER(ConvDesc), i32, i32, C.c_char_p, sz]
    L.plhip_debug_gemm_plan.restype = i32
    L.plhip_debug_patch_plan.argtypes = [C.POINTER(ConvDesc), C.c_char_p, sz]
    L.plhip_debug_patch_plan.restype = i32
    L.plhip_debug_dw_plan.argtypes = [C.POINTER(ConvDesc), i32, i32, i32, i32, i32, C.c_char_p, sz]
    L.plhip_debug_dw_plan.restype = i32
    L.plhip_debug_wide_ntt.argtypes = [i32]
    L.plhip_debug_wide_ntt.restype = None
    L.plhip_depthwise_conv_int8.argtypes = [vp, C.POINTER(ConvDesc), vp, vp, vp, vp, vp, i32]
    L.plhip_dwpw_fused_int8.argtypes = [vp, C.POINTER(ConvDesc), vp, vp, vp, vp, i32, vp, vp, vp, i32, f32, vp, i32]
    L.plhip_dwpw_fused_supported.argtypes = [C.POINTER(ConvDesc), i32, i32]
    L.plhip_dwpw_fused_supported.restype = i32
    L.plhip_dw_conv1x1_fused_int8.argtypes = [vp, C.POINTER(ConvDesc), vp, vp, vp, vp, i32, vp, vp, vp, i32, f32, vp, i32,
                                              vp, i32, vp, f32]
    L.plhip_dw_conv1x1_fused_supported.argtypes = [C.POINTER(ConvDesc), i32, i32, i32]
    L.plhip_dw_conv1x1_fused_supported.restype = i32
    L.plhip_fc_packed_weight_bytes.argtypes = [i32, i32]
    L.plhip_fc_packed_weight_bytes.restype = sz
    L.plhip_pack_fc_weights.argtypes = [vp, i32, i32, vp, vp]
    L.plhip_fc_int8.argtypes = [vp, i32, i32, i32, vp, vp, vp, vp, i32, vp, i32]
    L.plhip_calib_f32_to_i8.argtypes = [vp, vp, vp, f32, C.c_int64]
    L.plhip_calib_i8_to_f32.argtypes = [vp, vp, vp, f32, C.c_int64]
    L.plhip_global_avg_pool_f32.argtypes = [vp, vp, i32, i32, vp]
    L.plhip_softmax_f32.argtypes = [vp, vp, i32, i32, vp]
    L.plhip_pool2d_f32.argtypes = [vp, C.POINTER(PoolDesc), vp, vp]
    L.plhip_pool2d_max_i8.argtypes = [vp, C.POINTER(PoolDesc), vp, vp]
    L.plhip_elementwise_add_f32.argtypes = [vp, vp, vp, vp, C.c_int64, i32]
    L.plhip_hard_act_f32.argtypes = [vp, i32, C.POINTER(f32), vp, vp, vp, f32, C.c_int64]
    L.plhip_se_scale_f32.argtypes = [vp, vp, vp, i32, i32, i32, vp, vp, f32]
    L.plhip_se_gate_supported.argtypes = [i32, i32, i32, i32]
    L.plhip_se_gate_packed_weight_bytes.argtypes = [i32, i32]
    L.plhip_se_gate_packed_weight_bytes.restype = C.c_size_t
    L.plhip_pack_se_gate_weights.argtypes = [vp, i32, i32, vp, vp, vp]
    L.plhip_se_gate_int8.argtypes = [vp, C.POINTER(SeGateDesc), vp, vp, vp, vp, vp, vp, vp]
    L.plhip_concat_f32.argtypes = [vp, C.POINTER(vp), C.POINTER(C.c_int64), i32, C.c_int64, C.c_int64, vp]
    L.plhip_concat_calib_f32.argtypes = [vp, C.POINTER(vp), C.POINTER(C.c_int64), i32, C.c_int64, C.c_int64, vp, vp, f32]
    L.plhip_split_f32.argtypes = [vp, vp, C.c_int64, C.c_int64, C.c_int64, i32, C.POINTER(C.c_int64), i32, C.POINTER(vp)]
    L.plhip_shuffle_channel_f32.argtypes = [vp, vp, i32, i32, i32, i32, vp, vp, f32]
    L.plhip_shuffle_unit_f32.argtypes = [vp, vp, vp, i32, i32, i32, i32, vp, vp, vp, f32]
    L.plhip_interp_f32.argtypes = [vp, vp, C.c_int64, i32, i32, i32, i32, i32, i32, i32, vp, vp, f32]
    L.plhip_arg_max_f32.argtypes = [vp, vp, C.c_int64, i32, C.c_int64, vp, i32]
    L.plhip_interp_argmax_f32.argtypes = [vp, vp, i32, i32, i32, i32, i32, i32, i32, i32, i32, vp, i32]
    L.plhip_transpose_f32.argtypes = [vp, vp, C.POINTER(C.c_int64), C.POINTER(i32), i32, vp]
    L.plhip_concat_nhwc_f32.argtypes = [vp, C.POINTER(vp), C.POINTER(C.c_int64), C.POINTER(C.c_int64), i32, C.c_int64, vp]
    L.plhip_box_coder_decode_f32.argtypes = [vp, vp, vp, C.POINTER(f32), vp, C.c_int64, C.c_int64, i32, i32, vp]
    L.plhip_multiclass_nms_workspace_bytes.argtypes = [C.POINTER(NmsDesc)]
    L.plhip_multiclass_nms_workspace_bytes.restype = sz
    L.plhip_multiclass_nms_f32.argtypes = [vp, vp, vp, C.POINTER(NmsDesc), vp, vp, vp, vp]
    ip = C.POINTER(i32)
    L.plhip_yolo_box_f32.argtypes = [vp, vp, vp, i32, i32, i32, i32, i32, ip, f32, i32, i32, f32, vp, vp]
    L.plhip_yolo_head_f32.argtypes = [vp, C.POINTER(vp), ip, ip, C.POINTER(ip), ip, ip, i32, vp, i32, i32, f32, i32, f32, vp, vp]
    L.plhip_selftest.argtypes = [vp]
    _lib = L
    return L


def read_stamps(family, shape):
    """The in-kernel timeline of the last stamping launch of a kernel family ("gemm", "tr", "wide", "patch", "fw", "fs",
    "f7") as a uint64 array of `shape`.  Needs a `make EXPERIMENTS=1` library and PLHIP_STAMPS=1."""
    L = load()
    if not hasattr(L, "plhip_debug_read_stamps"):
        raise PlhipError("this library has no timeline stamps: rebuild with `make -C paddle-lite_amd/csrc clean && "
                         "make -C paddle-lite_amd/csrc EXPERIMENTS=1`")
    if not KNOBS_SET.get("STAMPS"):
        raise PlhipError("run with PLHIP_STAMPS=1")
    L.plhip_debug_read_stamps.argtypes = [C.c_char_p, C.c_void_p, C.c_size_t]
    buf = np.zeros(shape, np.uint64)
    if L.plhip_debug_read_stamps(family.encode(), buf.ctypes.data, buf.nbytes) != 0:
        raise PlhipError("no %s stamps: no launch of that kernel family since PLHIP_STAMPS=1" % family)
    return buf


def _outer_inner(shape, axis):
    """(axis made non-negative, the product of the extents in front of it, the product of those behind it)."""
    axis = axis + len(shape) if axis < 0 else axis
    return axis, int(np.prod(shape[:axis], dtype=np.int64)), int(np.prod(shape[axis + 1:], dtype=np.int64))


SCOPE_SLACK = 64  # bytes every DeviceScope allocation has behind its tensor, beyond any guard
MARGIN_GUARD = 64  # bytes a helper that returns an output's margins adds on both sides of it


class DeviceOut:
    """An output tensor inside one DeviceScope allocation: .ptr for the library, .get() the tensor, .margins() the allocation's
    bytes in front of and behind the tensor, concatenated."""

    def __init__(self, ctx, base, total, lead, shape, dtype):
        self.ctx, self.base, self.total, self.lead = ctx, base, total, lead
        self.shape, self.dtype = tuple(shape), np.dtype(dtype)
        self.nbytes = int(np.prod(self.shape, dtype=np.int64)) * self.dtype.itemsize
        self.ptr = C.c_void_p(base.value + lead)

    def get(self):
        return self.ctx.to_host(self.ptr, self.shape, self.dtype)

    def margins(self):
        raw = self.ctx.to_host(self.base, (self.total,), np.uint8)
        return np.concatenate([raw[:self.lead], raw[self.lead + self.nbytes:]])


class _NoOut:
    """The handle of an output the caller did not ask for: a null pointer and nothing to download."""
    ptr = None

    def get(self):
        return None

    def margins(self):
        return None


class DeviceScope:
    """The owner of a whole-op helper's temporary device buffers (Context.scope()): a context manager that frees everything it
    handed out when it exits, an exception passing through or not.  Every allocation is [guard][off][tensor][guard][SCOPE_SLACK]
    with a 16-byte-aligned base, so `off` (bytes) is the tensor's misalignment."""

    def __init__(self, ctx):
        self.ctx, self._owned = ctx, []

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.release()

    def release(self):
        """Frees everything handed out so far; the scope can go on handing out buffers."""
        owned, self._owned = self._owned, []
        for p in owned:
            self.ctx.free(p)

    def _place(self, nbytes, off, fill, guard):
        assert guard % 16 == 0 and off >= 0
        total = guard + off + nbytes + guard + SCOPE_SLACK
        base = self.ctx.malloc(total)
        self._owned.append(base)
        assert base.value % 16 == 0
        if fill is not None:
            self.ctx.check(self.ctx.L.plhip_memset(self.ctx.h, base, int(fill), total), "memset")
        return base, total

    def put(self, arr, dtype=None, off=0):
        """Uploads a contiguous copy of arr (cast to dtype if given); the pointer lies `off` bytes past a 16-byte boundary."""
        arr = np.ascontiguousarray(arr, dtype)
        base, _total = self._place(arr.nbytes, off, None, 0)
        p = C.c_void_p(base.value + off)
        if arr.nbytes:
            self.ctx.check(self.ctx.L.plhip_memcpy_h2d(self.ctx.h, p, arr.ctypes.data_as(C.c_void_p), arr.nbytes), "h2d")
        return p

    def put_opt(self, arr, dtype):
        """put() of an optional operand: a null pointer and no allocation when arr is None."""
        return self.put(arr, dtype) if arr is not None else C.c_void_p()

    def alloc(self, nbytes):
        """Raw scratch (packed weights, workspaces)."""
        return self._place(int(nbytes), 0, None, 0)[0]

    def out(self, shape, dtype, off=0, fill=None, guard=0):
        """An output tensor `off` bytes past a 16-byte boundary, as a DeviceOut; fill: the byte the whole allocation is set to
        first; guard: bytes (a multiple of 16) added on both sides."""
        nbytes = int(np.prod(tuple(shape), dtype=np.int64)) * np.dtype(dtype).itemsize
        base, total = self._place(nbytes, off, fill, guard)
        return DeviceOut(self.ctx, base, total, guard + off, shape, dtype)

    def out_opt(self, wanted, shape, dtype, off=0, fill=None, guard=0):
        """out() of an optional output: a handle with a null .ptr whose .get() and .margins() are None when not wanted."""
        return self.out(shape, dtype, off, fill, guard) if wanted else _NoOut()

    def out_by_mode(self, shape, mode, misalign):
        """The outputs `mode` names ("f32", "i8" or "both") as the handle pair (f32, i8), each base `misalign` ELEMENTS off its
        allocation's alignment: the fp32 output 4 * misalign bytes, the int8 output misalign bytes."""
        assert mode in ("f32", "i8", "both")
        return self.out_opt(mode != "i8", shape, np.float32, 4 * misalign), self.out_opt(mode != "f32", shape, np.int8, misalign)


class Context:
    """One plhip_ctx (device + stream).  Thin, explicit device-memory helpers for tests/bench."""

    def __init__(self, device=0, stream=None):
        self.L = load()
        h = C.c_void_p()
        if stream is None:
            st = self.L.plhip_ctx_create(device, C.byref(h))
        else:
            st = self.L.plhip_ctx_create_on_stream(device, C.c_void_p(stream), C.byref(h))
        if st != 0:
            raise PlhipError("plhip_ctx_create failed (%d): %s" % (st, self.L.plhip_last_error(None).decode()))
        self.h = h
        self._allocs = []

    def check(self, st, what=""):
        if st != 0:
            raise PlhipError("%s failed (%d): %s" % (what, st, self.L.plhip_last_error(self.h).decode()))

    def close(self):
        if self.h:
            for p in self._allocs:
                self.L.plhip_free(self.h, p)
            self._allocs = []
            self.L.plhip_ctx_destroy(self.h)
            self.h = None

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    # ---- memory ----
    def malloc(self, nbytes):
        p = C.c_void_p()
        self.check(self.L.plhip_malloc(self.h, nbytes, C.byref(p)), "plhip_malloc")
        self._allocs.append(p)
        return p

    def free(self, p):
        self._allocs = [q for q in self._allocs if q.value != p.value]
        self.check(self.L.plhip_free(self.h, p), "plhip_free")

    def outstanding(self):
        """The number of live allocations."""
        return len(self._allocs)

    def free_all(self):
        for p in list(self._allocs):
            self.free(p)

    def scope(self):
        """A DeviceScope: `with ctx.scope() as s:` owns the temporary buffers of one op and frees them on the way out."""
        return DeviceScope(self)

    def to_device(self, arr):
        arr = np.ascontiguousarray(arr)
        p = self.malloc(max(1, arr.nbytes))
        if arr.nbytes:
            self.check(self.L.plhip_memcpy_h2d(self.h, p, arr.ctypes.data_as(C.c_void_p), arr.nbytes), "h2d")
        return p

    def to_host(self, p, shape, dtype):
        out = np.empty(shape, dtype)
        if out.nbytes:
            self.check(self.L.plhip_memcpy_d2h(self.h, out.ctypes.data_as(C.c_void_p), p, out.nbytes), "d2h")
        return out

    def sync(self):
        self.check(self.L.plhip_stream_sync(self.h), "sync")

    def selftest(self):
        self.check(self.L.plhip_selftest(self.h), "plhip_selftest")

    # ---- whole-op helpers on host arrays (upload, run through the C ABI, download); every device buffer belongs to a scope
    def _packed_conv(self, s, d, w):
        """Uploads the int8 filter w of conv descriptor d and packs it: the packed pointer."""
        dw = s.put(w, np.int8)
        dwp = s.alloc(self.L.plhip_conv_packed_weight_bytes(C.byref(d)))
        self.check(self.L.plhip_pack_conv_weights(self.h, C.byref(d), dw, dwp), "pack")
        return dwp

    def _conv_workspace(self, s, d):
        """(pointer, bytes) of the workspace conv descriptor d asks for; a null pointer when it asks for none."""
        wsb = self.L.plhip_conv_workspace_bytes(C.byref(d))
        return (s.alloc(wsb) if wsb else C.c_void_p()), wsb

    def conv2d(self, d, x, w, scale, bias, out_kind, depthwise=False, misalign=0, sentinel=None):
        """plhip_conv2d_int8 / plhip_depthwise_conv_int8 on host arrays.  misalign: (x, y), as in conv2d_fused: x starts that
        many BYTES past a 16-byte boundary, y that many ELEMENTS; one number stands for both.  sentinel: a byte value the output
        allocation (MARGIN_GUARD more bytes on either side) is filled with first; the result is then (y, the bytes around y)."""
        oh, ow = out_hw(d)
        xo, yo = (misalign,) * 2 if isinstance(misalign, int) else misalign
        dtype = _OUT_DTYPE[out_kind]
        with self.scope() as s:
            dx = s.put(x, np.int8, off=xo)
            ds, db = s.put_opt(scale, np.float32), s.put_opt(bias, np.float32)
            y = s.out((d.n, d.cout, oh, ow), dtype, np.dtype(dtype).itemsize * yo, sentinel, 0 if sentinel is None else MARGIN_GUARD)
            if depthwise:
                self.check(self.L.plhip_depthwise_conv_int8(self.h, C.byref(d), dx, s.put(w, np.int8), ds, db, y.ptr, out_kind), "depthwise")
            else:
                dwp = self._packed_conv(s, d, w)
                dws, wsb = self._conv_workspace(s, d)
                self.check(self.L.plhip_conv2d_int8(self.h, C.byref(d), dx, dwp, ds, db, y.ptr, out_kind, dws, wsb), "conv2d")
            return y.get() if sentinel is None else (y.get(), y.margins())

    def conv2d_transpose(self, d, x, w, scale, bias, out_kind, misalign=0, sentinel=None):
        """plhip_conv2d_transpose_int8 on host arrays: x [n, cin, h, w], w [cin, cout / groups, kh, kw] (packed here).  misalign:
        y starts that many BYTES into its buffer; sentinel: a byte value the buffer is filled with first, then the result is
        (y, the bytes in front of and behind y)."""
        oh, ow = deconv_out_hw(d)
        c = d.conv
        with self.scope() as s:
            dx, dw = s.put(x, np.int8), s.put(w, np.int8)
            ds, db = s.put_opt(scale, np.float32), s.put_opt(bias, np.float32)
            y = s.out((c.n, c.cout, oh, ow), _OUT_DTYPE[out_kind], off=misalign, fill=0 if sentinel is None else sentinel)
            dwp = s.alloc(self.L.plhip_deconv_packed_weight_bytes(C.byref(d)))
            self.check(self.L.plhip_pack_deconv_weights(self.h, C.byref(d), dw, dwp), "pack_deconv")
            self.check(self.L.plhip_conv2d_transpose_int8(self.h, C.byref(d), dx, dwp, ds, db, y.ptr, out_kind), "conv2d_transpose")
            return y.get() if sentinel is None else (y.get(), y.margins())

    def conv2d_calib(self, d, x_f32, calib_scale, w, scale, bias, out_kind):
        """plhip_conv2d_calib_int8 on host arrays: calib[fp32_to_int8](calib_scale) + conv2d in one launch."""
        oh, ow = out_hw(d)
        with self.scope() as s:
            dx = s.put(x_f32, np.float32)
            ds, db = s.put_opt(scale, np.float32), s.put_opt(bias, np.float32)
            y = s.out((d.n, d.cout, oh, ow), _OUT_DTYPE[out_kind])
            dwp = self._packed_conv(s, d, w)
            self.check(self.L.plhip_conv2d_calib_int8(self.h, C.byref(d), dx, calib_scale, dwp, ds, db, y.ptr, out_kind), "conv2d_calib")
            return y.get()

    def image_to_tensor(self, img, src_u8, calib_scale=None):
        """plhip_image_to_tensor_f32 (calib_scale None) or _i8 on a host uint8 image [n, h, w, cs]: the NCHW tensor."""
        shape = (img.n, IMG_CHANNELS.get(img.format, 3), img.h, img.w)  # a format the library refuses gets its PlhipError
        with self.scope() as s:
            dx = s.put(src_u8, np.uint8)
            y = s.out(shape, np.float32 if calib_scale is None else np.int8)
            if calib_scale is None:
                self.check(self.L.plhip_image_to_tensor_f32(self.h, C.byref(img), dx, y.ptr), "image_to_tensor_f32")
            else:
                self.check(self.L.plhip_image_to_tensor_i8(self.h, C.byref(img), dx, y.ptr, float(calib_scale)), "image_to_tensor_i8")
            return y.get()

    def image_convert(self, frame, src_u8, dst_format=IMG_BGR):
        """plhip_image_convert_u8 on a host NV12 / NV21 frame [n, h * 3 / 2, w]: the interleaved image [n, h, w, 3 | 4]."""
        with self.scope() as s:
            dx = s.put(src_u8, np.uint8)
            y = s.out((frame.n, frame.h, frame.w, IMG_BYTES.get(dst_format, 4)), np.uint8)
            self.check(self.L.plhip_image_convert_u8(self.h, C.byref(frame), dx, int(dst_format), y.ptr), "image_convert_u8")
            return y.get()

    def image_resize(self, frame, src_u8, h_out, w_out):
        """plhip_image_resize_u8 on a host frame: the resized interleaved image [n, h_out, w_out, cs] (BGR from an NV frame)."""
        with self.scope() as s:
            dx = s.put(src_u8, np.uint8)
            y = s.out((frame.n, h_out, w_out, IMG_BYTES.get(frame.format, 3)), np.uint8)
            self.check(self.L.plhip_image_resize_u8(self.h, C.byref(frame), dx, int(h_out), int(w_out), y.ptr), "image_resize_u8")
            return y.get()

    def frame_to_tensor(self, frame, img, src_u8, calib_scale=None):
        """plhip_frame_to_tensor_f32 (calib_scale None) or _i8 on a host frame: the NCHW tensor of the resized image, one launch."""
        with self.scope() as s:
            dx = s.put(src_u8, np.uint8)
            y = s.out((img.n, IMG_CHANNELS.get(img.format, 3), img.h, img.w), np.float32 if calib_scale is None else np.int8)
            if calib_scale is None:
                self.check(self.L.plhip_frame_to_tensor_f32(self.h, C.byref(frame), C.byref(img), dx, y.ptr), "frame_to_tensor_f32")
            else:
                self.check(self.L.plhip_frame_to_tensor_i8(self.h, C.byref(frame), C.byref(img), dx, y.ptr, float(calib_scale)), "frame_to_tensor_i8")
            return y.get()

    def conv2d_image(self, d, img, src_u8, calib_scale, w, scale, bias, out_kind):
        """plhip_conv2d_image_int8 on host arrays: image_to_tensor + calib[fp32_to_int8](calib_scale) + conv2d in one launch."""
        oh, ow = out_hw(d)
        with self.scope() as s:
            dx = s.put(src_u8, np.uint8)
            ds, db = s.put_opt(scale, np.float32), s.put_opt(bias, np.float32)
            y = s.out((d.n, d.cout, oh, ow), _OUT_DTYPE[out_kind])
            dwp = self._packed_conv(s, d, w)
            self.check(self.L.plhip_conv2d_image_int8(self.h, C.byref(d), C.byref(img), dx, float(calib_scale), dwp, ds, db, y.ptr, out_kind),
                       "conv2d_image")
            return y.get()

    def conv2d_fused(self, d, x, w, scale, bias, residual, residual_relu, calib_scale, want_f32=True, misalign=0, sentinel=None):
        """plhip_conv2d_int8_fused on host arrays: returns (y_f32 or None, y_i8 or None).  misalign: (x, y, residual, y_i8), as in
        dw_conv1x1_fused: x and y_i8 start that many BYTES past a 16-byte boundary, y and the residual that many ELEMENTS; one
        number stands for all four.  sentinel: a byte value both output allocations (MARGIN_GUARD more bytes on either side)
        are filled with first; the result is then (y_f32, y_i8, the bytes around y_f32, the bytes around y_i8), None for an
        output not asked for."""
        oh, ow = out_hw(d)
        shape = (d.n, d.cout, oh, ow)
        xo, yo, ro, qo = (misalign,) * 4 if isinstance(misalign, int) else misalign
        guard = 0 if sentinel is None else MARGIN_GUARD
        with self.scope() as s:
            dx, ds = s.put(x, np.int8, off=xo), s.put(scale, np.float32)
            db = s.put_opt(bias, np.float32)
            dr = s.put(residual, np.float32, off=4 * ro) if residual is not None else C.c_void_p()
            yf = s.out_opt(want_f32, shape, np.float32, 4 * yo, sentinel, guard)
            yq = s.out_opt(calib_scale is not None, shape, np.int8, qo, sentinel, guard)
            dwp = self._packed_conv(s, d, w)
            dws, wsb = self._conv_workspace(s, d)
            self.check(self.L.plhip_conv2d_int8_fused(self.h, C.byref(d), dx, dwp, ds, db, yf.ptr, dr, int(residual_relu), yq.ptr,
                                                      float(calib_scale) if calib_scale is not None else 0.0, dws, wsb), "conv2d_fused")
            return (yf.get(), yq.get()) if sentinel is None else (yf.get(), yq.get(), yf.margins(), yq.margins())

    def dwpw_fused(self, d_dw, x, w_dw, s_dw, b_dw, w_pw, s_pw, b_pw, pw_act, pw_alpha, out_kind):
        """Fused depthwise -> pointwise through the C ABI (host arrays in, host array out)."""
        oh, ow = out_hw(d_dw)
        cout = w_pw.shape[0]
        d_pw = conv_desc(d_dw.n, d_dw.cin, oh, ow, cout, 1, 1, act=pw_act, alpha=pw_alpha)
        with self.scope() as s:
            dx, dwd, dsd, dbd = s.put(x, np.int8), s.put(w_dw, np.int8), s.put(s_dw, np.float32), s.put_opt(b_dw, np.float32)
            dwp = self._packed_conv(s, d_pw, w_pw)
            dsp, dbp = s.put_opt(s_pw, np.float32), s.put_opt(b_pw, np.float32)
            y = s.out((d_dw.n, cout, oh, ow), _OUT_DTYPE.get(out_kind, np.float32))
            self.check(self.L.plhip_dwpw_fused_int8(self.h, C.byref(d_dw), dx, dwd, dsd, dbd, cout, dwp, dsp, dbp, pw_act, pw_alpha,
                                                    y.ptr, out_kind), "dwpw_fused")
            return self.to_host(y.ptr, (d_dw.n, cout, 1, 1), np.float32) if out_kind == OUT_F32_GAP else y.get()

    def dw_conv1x1_fused(self, d_dw, x, w_dw, s_dw, b_dw, w_pw, s_pw, b_pw, pw_act, pw_alpha, out_kind,
                         residual=None, residual_relu=0, calib_scale=None, want_y=True, misalign=0, sentinel=None):
        """Fused depthwise 3x3 -> 1x1 conv with the conv's graph tail (plhip_dw_conv1x1_fused_int8) on host arrays:
        returns (y or None, y_i8 or None); y is of `out_kind`, y_i8 the calib copy when calib_scale is given.  misalign: (x, y,
        y_i8): x starts that many BYTES past a 16-byte boundary (off 4 bytes the kernel stages its rows byte by byte), y that
        many ELEMENTS, y_i8 that many bytes; one number stands for all three.  sentinel: a byte value both output allocations
        (MARGIN_GUARD more bytes on either side) are filled with first; the result is then (y, y_i8, the bytes around y, the
        bytes around y_i8), None for an output not asked for."""
        oh, ow = out_hw(d_dw)
        cout = w_pw.shape[0]
        shape = (d_dw.n, cout, oh, ow)
        d_pw = conv_desc(d_dw.n, d_dw.cin, oh, ow, cout, 1, 1, act=pw_act, alpha=pw_alpha)
        xo, yo, qo = (misalign,) * 3 if isinstance(misalign, int) else misalign
        ydt = np.dtype(_OUT_DTYPE[out_kind])
        guard = 0 if sentinel is None else MARGIN_GUARD
        with self.scope() as s:
            dx, dwd, dsd, dbd = s.put(x, np.int8, off=xo), s.put(w_dw, np.int8), s.put(s_dw, np.float32), s.put_opt(b_dw, np.float32)
            dwp = self._packed_conv(s, d_pw, w_pw)
            dsp, dbp, dr = s.put_opt(s_pw, np.float32), s.put_opt(b_pw, np.float32), s.put_opt(residual, np.float32)
            y = s.out_opt(want_y, shape, ydt, yo * ydt.itemsize, sentinel, guard)
            yq = s.out_opt(calib_scale is not None, shape, np.int8, qo, sentinel, guard)
            self.check(self.L.plhip_dw_conv1x1_fused_int8(self.h, C.byref(d_dw), dx, dwd, dsd, dbd, cout, dwp, dsp, dbp, pw_act,
                                                          pw_alpha, y.ptr, out_kind, dr, int(residual_relu), yq.ptr,
                                                          float(calib_scale) if calib_scale is not None else 0.0),
                       "dw_conv1x1_fused")
            return (y.get(), yq.get()) if sentinel is None else (y.get(), yq.get(), y.margins(), yq.margins())

    def fc(self, x, w, scale, bias, relu, out_kind):
        x = np.ascontiguousarray(x, np.int8)
        w = np.ascontiguousarray(w, np.int8)
        m, k = x.shape
        n = w.shape[1]
        with self.scope() as s:
            dx, dw = s.put(x), s.put(w)
            dwp = s.alloc(self.L.plhip_fc_packed_weight_bytes(k, n))
            self.check(self.L.plhip_pack_fc_weights(self.h, k, n, dw, dwp), "pack_fc")
            ds, db = s.put_opt(scale, np.float32), s.put_opt(bias, np.float32)
            y = s.out((m, n), _OUT_DTYPE[out_kind])
            self.check(self.L.plhip_fc_int8(self.h, m, k, n, dx, dwp, ds, db, int(relu), y.ptr, out_kind), "fc")
            return y.get()

    def calib_f32_to_i8(self, x, scale):
        x = np.ascontiguousarray(x, np.float32)
        with self.scope() as s:
            y = s.out(x.shape, np.int8)
            self.check(self.L.plhip_calib_f32_to_i8(self.h, s.put(x), y.ptr, scale, x.size), "calib_f32_to_i8")
            return y.get()

    def calib_i8_to_f32(self, x, scale):
        x = np.ascontiguousarray(x, np.int8)
        with self.scope() as s:
            y = s.out(x.shape, np.float32)
            self.check(self.L.plhip_calib_i8_to_f32(self.h, s.put(x), y.ptr, scale, x.size), "calib_i8_to_f32")
            return y.get()

    def global_avg_pool(self, x):
        x = np.ascontiguousarray(x, np.float32)
        n, c = x.shape[:2]
        sp = int(np.prod(x.shape[2:]))
        with self.scope() as s:
            y = s.out((n, c, 1, 1), np.float32)
            self.check(self.L.plhip_global_avg_pool_f32(self.h, s.put(x), n * c, sp, y.ptr), "pool")
            return y.get()

    def softmax(self, x):
        x = np.ascontiguousarray(x, np.float32)
        rows, cols = int(np.prod(x.shape[:-1])), x.shape[-1]
        with self.scope() as s:
            y = s.out(x.shape, np.float32)
            self.check(self.L.plhip_softmax_f32(self.h, s.put(x), rows, cols, y.ptr), "softmax")
            return y.get()

    def pool2d(self, x, pooling_type, ksize, strides, pads, exclusive=True, ceil_mode=False):
        """x [n,c,h,w] fp32; pads {top, bottom, left, right}; output dims by PoolOutputSize (pool_op.cc:44-61)."""
        i8 = np.asarray(x).dtype == np.int8
        x = np.ascontiguousarray(x, np.int8 if i8 else np.float32)
        n, c, h, w = x.shape

        def osz(i, k, p0, p1, s):
            return (i - k + p0 + p1 + (s - 1 if ceil_mode else 0)) // s + 1
        d = PoolDesc()
        d.planes, d.h, d.w = n * c, h, w
        d.oh, d.ow = osz(h, ksize[0], pads[0], pads[1], strides[0]), osz(w, ksize[1], pads[2], pads[3], strides[1])
        d.kh, d.kw = ksize
        d.pad[:] = list(pads)
        d.stride[:] = list(strides)
        d.is_max, d.exclusive = int(pooling_type == "max"), int(exclusive)
        fn = self.L.plhip_pool2d_max_i8 if i8 else self.L.plhip_pool2d_f32
        with self.scope() as s:
            y = s.out((n, c, d.oh, d.ow), x.dtype)
            self.check(fn(self.h, C.byref(d), s.put(x), y.ptr), "pool2d")
            return y.get()

    def elementwise_add(self, x, y, relu=False):
        x = np.ascontiguousarray(x, np.float32)
        with self.scope() as s:
            dx, dy = s.put(x), s.put(y, np.float32)
            o = s.out(x.shape, np.float32)
            self.check(self.L.plhip_elementwise_add_f32(self.h, dx, dy, o.ptr, x.size, int(relu)), "elementwise_add")
            return o.get()

    # ---- misalign below: ELEMENTS every device base of the helper is moved off its allocation's alignment (the scalar path)
    def hard_act(self, kind, x, params=None, mode="f32", calib_scale=1.0, misalign=0):
        """plhip_hard_act_f32: kind HARD_SWISH (params threshold, scale, offset) or HARD_SIGMOID (slope, offset)."""
        x = np.ascontiguousarray(x, np.float32)
        if params is None:
            params = HARD_SWISH_DEFAULTS if kind == HARD_SWISH else HARD_SIGMOID_DEFAULTS
        pr = (C.c_float * 3)(*(list(map(float, params)) + [0.0] * 3)[:3])
        with self.scope() as s:
            dx = s.put(x, off=4 * misalign)
            yf, yq = s.out_by_mode(x.shape, mode, misalign)
            self.check(self.L.plhip_hard_act_f32(self.h, int(kind), pr, dx, yf.ptr, yq.ptr, float(calib_scale), x.size), "hard_act")
            return yf.get(), yq.get()

    def se_scale(self, x, gate, mode="f32", calib_scale=1.0, misalign=0):
        """plhip_se_scale_f32: x [n, c, ...] fp32 times gate [n, c] (any trailing 1s)."""
        x = np.ascontiguousarray(x, np.float32)
        gate = np.ascontiguousarray(gate, np.float32)
        n, c = x.shape[:2]
        hw = int(np.prod(x.shape[2:]))
        assert gate.size == n * c
        with self.scope() as s:
            dg, dx = s.put(gate), s.put(x, off=4 * misalign)
            yf, yq = s.out_by_mode(x.shape, mode, misalign)
            self.check(self.L.plhip_se_scale_f32(self.h, dx, dg, n, c, hw, yf.ptr, yq.ptr, float(calib_scale)), "se_scale")
            return yf.get(), yq.get()

    def se_gate(self, pooled, calib_scale, w1, s1, b1, act1, alpha1, w2, s2, b2, act2=ACT_NONE, alpha2=0.0, slope=0.2, offset=0.5):
        """plhip_se_gate_int8: pooled fp32 [n, c]; w1 [cr, c] / w2 [c, cr] int8; s / b the convs' folded scale / bias arrays
        (b may be None).  Returns the fp32 gate [n, c]."""
        pooled = np.ascontiguousarray(pooled, np.float32)
        n, c = pooled.shape[0], int(np.prod(pooled.shape[1:]))
        w1 = np.ascontiguousarray(w1, np.int8).reshape(-1, c)
        cr = w1.shape[0]
        w2 = np.ascontiguousarray(w2, np.int8).reshape(c, cr)
        d = SeGateDesc(n, c, cr, float(calib_scale), int(act1), int(act2), float(alpha1), float(alpha2), float(slope), float(offset))
        with self.scope() as s:
            dx, dw1, dw2 = s.put(pooled), s.put(w1), s.put(w2)
            dwp = s.alloc(self.L.plhip_se_gate_packed_weight_bytes(c, cr))
            ds1, ds2 = s.put(s1, np.float32), s.put(s2, np.float32)
            db1, db2 = s.put_opt(b1, np.float32), s.put_opt(b2, np.float32)
            y = s.out((n, c), np.float32)
            self.check(self.L.plhip_pack_se_gate_weights(self.h, c, cr, dw1, dw2, dwp), "pack_se_gate")
            self.check(self.L.plhip_se_gate_int8(self.h, C.byref(d), dx, dwp, ds1, db1, ds2, db2, y.ptr), "se_gate")
            return y.get()

    # ---- concat / split / shuffle_channel and the fused unit tail (shuffle_ops.hip)
    def concat(self, xs, axis, misalign=0):
        """plhip_concat_f32 of fp32 arrays along `axis`."""
        xs = [np.ascontiguousarray(x, np.float32) for x in xs]
        axis, outer, inner = _outer_inner(xs[0].shape, axis)
        shape = xs[0].shape[:axis] + (sum(x.shape[axis] for x in xs),) + xs[0].shape[axis + 1:]
        ext = (C.c_int64 * len(xs))(*[x.shape[axis] for x in xs])
        with self.scope() as s:
            ptrs = (C.c_void_p * len(xs))(*[s.put(x, off=4 * misalign) for x in xs])
            y = s.out(shape, np.float32, 4 * misalign)
            self.check(self.L.plhip_concat_f32(self.h, ptrs, ext, len(xs), outer, inner, y.ptr), "concat")
            return y.get()

    def concat_calib(self, xs, axis, calib_scale, with_f32=True, misalign=0):
        """plhip_concat_calib_f32 of fp32 arrays along `axis`: returns (y_f32 or None, y_i8)."""
        xs = [np.ascontiguousarray(x, np.float32) for x in xs]
        axis, outer, inner = _outer_inner(xs[0].shape, axis)
        shape = xs[0].shape[:axis] + (sum(x.shape[axis] for x in xs),) + xs[0].shape[axis + 1:]
        ext = (C.c_int64 * len(xs))(*[x.shape[axis] for x in xs])
        with self.scope() as s:
            ptrs = (C.c_void_p * len(xs))(*[s.put(x, off=4 * misalign) for x in xs])
            yf, yq = s.out_opt(with_f32, shape, np.float32, 4 * misalign), s.out(shape, np.int8, misalign)
            self.check(self.L.plhip_concat_calib_f32(self.h, ptrs, ext, len(xs), outer, inner, yf.ptr, yq.ptr, float(calib_scale)), "concat_calib")
            return yf.get(), yq.get()

    def split(self, x, axis, num=0, sections=(), misalign=0):
        """plhip_split_f32: num > 0 equal parts, else `sections`.  Returns the list of parts."""
        x = np.ascontiguousarray(x, np.float32)
        axis, outer, inner = _outer_inner(x.shape, axis)
        ext = [x.shape[axis] // num] * num if num > 0 else list(sections)
        sec = (C.c_int64 * max(1, len(sections)))(*sections) if num == 0 else None
        with self.scope() as s:
            dx = s.put(x, off=4 * misalign)
            outs = [s.out(x.shape[:axis] + (e,) + x.shape[axis + 1:], np.float32, 4 * misalign) for e in ext]
            ptrs = (C.c_void_p * len(ext))(*[o.ptr for o in outs])
            self.check(self.L.plhip_split_f32(self.h, dx, outer, x.shape[axis], inner, int(num), sec, len(ext), ptrs), "split")
            return [o.get() for o in outs]

    def shuffle_channel(self, x, group, mode="f32", calib_scale=1.0, misalign=0):
        """plhip_shuffle_channel_f32: x [n, c, ...]; returns (y_f32 or None, y_i8 or None)."""
        x = np.ascontiguousarray(x, np.float32)
        n, c = x.shape[:2]
        hw = int(np.prod(x.shape[2:], dtype=np.int64))
        with self.scope() as s:
            dx = s.put(x, off=4 * misalign)
            yf, yq = s.out_by_mode(x.shape, mode, misalign)
            self.check(self.L.plhip_shuffle_channel_f32(self.h, dx, n, c, hw, int(group), yf.ptr, yq.ptr, float(calib_scale)), "shuffle_channel")
            return yf.get(), yq.get()

    def shuffle_unit(self, a, b, split_at, mode="f32", calib_scale=1.0, misalign=0):
        """plhip_shuffle_unit_f32: a, b [n, h, ...].  Returns (lo_f32 or None, hi_f32 or None, hi_i8 or None); mode names the
        outputs of the high part ("f32", "i8", "both")."""
        a = np.ascontiguousarray(a, np.float32)
        b = np.ascontiguousarray(b, np.float32)
        n, h = a.shape[:2]
        hw = int(np.prod(a.shape[2:], dtype=np.int64))
        rest = tuple(a.shape[2:])
        with self.scope() as s:
            da, db = s.put(a, off=4 * misalign), s.put(b, off=4 * misalign)
            lo = s.out_opt(split_at > 0, (n, split_at) + rest, np.float32, 4 * misalign)
            hf, hq = s.out_by_mode((n, 2 * h - split_at) + rest, mode, misalign)
            self.check(self.L.plhip_shuffle_unit_f32(self.h, da, db, n, h, hw, int(split_at), lo.ptr, hf.ptr, hq.ptr, float(calib_scale)),
                       "shuffle_unit")
            return lo.get(), hf.get(), hq.get()

    # ---- bilinear_interp / nearest_interp / arg_max and interp -> arg_max in one launch (interp_ops.hip)
    def interp(self, x, out_hw, method="bilinear", align_corners=False, align_mode=1, mode="f32", calib_scale=1.0, misalign=0):
        """plhip_interp_f32: x [..., h, w] fp32 resampled to out_hw.  Returns (y_f32 or None, y_i8 or None); mode names the outputs
        ("f32", "i8", "both"); misalign: elements every device base is moved off its allocation's alignment."""
        x = np.ascontiguousarray(x, np.float32)
        ih, iw = x.shape[-2:]
        oh, ow = (int(v) for v in out_hw)
        planes = int(np.prod(x.shape[:-2], dtype=np.int64))
        with self.scope() as s:
            dx = s.put(x, off=4 * misalign)
            yf, yq = s.out_by_mode(tuple(x.shape[:-2]) + (oh, ow), mode, misalign)
            self.check(self.L.plhip_interp_f32(self.h, dx, planes, ih, iw, oh, ow, INTERP_METHODS[method], int(align_corners),
                                               int(align_mode), yf.ptr, yq.ptr, float(calib_scale)), "interp")
            return yf.get(), yq.get()

    def arg_max(self, x, axis, dtype=-1, keepdims=False, misalign=0):
        """plhip_arg_max_f32 along `axis` of an fp32 array; dtype as ArgmaxParam's (-1 / 3 int64, 2 int32)."""
        x = np.ascontiguousarray(x, np.float32)
        axis, outer, inner = _outer_inner(x.shape, axis)
        np_t = np.dtype(ARGMAX_DTYPES[dtype])
        with self.scope() as s:
            dx = s.put(x, off=4 * misalign)
            y = s.out(x.shape[:axis] + ((1,) if keepdims else ()) + x.shape[axis + 1:], np_t, np_t.itemsize * misalign)
            self.check(self.L.plhip_arg_max_f32(self.h, dx, outer, x.shape[axis], inner, y.ptr, int(dtype)), "arg_max")
            return y.get()

    def interp_argmax(self, x, out_hw, method="bilinear", align_corners=False, align_mode=1, dtype=-1, misalign=0):
        """plhip_interp_argmax_f32: x [n, c, h, w] fp32 -> labels [n, oh, ow] of the resampled tensor, which is never written."""
        x = np.ascontiguousarray(x, np.float32)
        n, c, ih, iw = x.shape
        oh, ow = (int(v) for v in out_hw)
        np_t = np.dtype(ARGMAX_DTYPES[dtype])
        with self.scope() as s:
            dx = s.put(x, off=4 * misalign)
            y = s.out((n, oh, ow), np_t, np_t.itemsize * misalign)
            self.check(self.L.plhip_interp_argmax_f32(self.h, dx, n, c, ih, iw, oh, ow, INTERP_METHODS[method], int(align_corners),
                                                      int(align_mode), y.ptr, int(dtype)), "interp_argmax")
            return y.get()

    # ---- detection heads: transpose, the one-launch head join, box_coder, multiclass_nms (transpose_ops.hip, detection_ops.hip)
    def transpose(self, x, perm, misalign=0):
        """plhip_transpose_f32: np.transpose(x, perm) of an fp32 array of rank 2 .. 4, the bits moved."""
        x = np.ascontiguousarray(x, np.float32)
        dims = (C.c_int64 * x.ndim)(*x.shape)
        pm = (C.c_int * len(perm))(*[int(v) for v in perm])
        with self.scope() as s:
            dx = s.put(x, off=4 * misalign)
            y = s.out(tuple(x.shape[k] for k in perm), np.float32, 4 * misalign)
            self.check(self.L.plhip_transpose_f32(self.h, dx, dims, pm, x.ndim, y.ptr), "transpose")
            return y.get()

    def concat_nhwc(self, xs, misalign=0):
        """plhip_concat_nhwc_f32 of NCHW fp32 arrays [n, c_i, h_i, w_i]: returns [n, sum c_i * h_i * w_i]."""
        xs = [np.ascontiguousarray(x, np.float32) for x in xs]
        n = xs[0].shape[0]
        ch = (C.c_int64 * len(xs))(*[x.shape[1] for x in xs])
        hw = (C.c_int64 * len(xs))(*[x.shape[2] * x.shape[3] for x in xs])
        with self.scope() as s:
            ptrs = (C.c_void_p * len(xs))(*[s.put(x, off=4 * misalign) for x in xs])
            y = s.out((n, sum(x[0].size for x in xs)), np.float32, 4 * misalign)
            self.check(self.L.plhip_concat_nhwc_f32(self.h, ptrs, ch, hw, len(xs), n, y.ptr), "concat_nhwc")
            return y.get()

    def box_coder_decode(self, prior, target, prior_var=None, variance=None, axis=0, normalized=True, misalign=0):
        """plhip_box_coder_decode_f32: target [rows, cols, 4]; prior (and prior_var) [cols, 4] with axis 0, [rows, 4] with axis 1;
        variance: the 4-float attribute, read when prior_var is None."""
        target = np.ascontiguousarray(target, np.float32)
        rows, cols = target.shape[:2]
        v4 = (C.c_float * 4)(*[float(v) for v in variance]) if variance is not None else None
        with self.scope() as s:
            dp, dt = s.put(prior, np.float32, 4 * misalign), s.put(target, off=4 * misalign)
            dv = s.put(prior_var, np.float32, 4 * misalign) if prior_var is not None else None
            y = s.out(target.shape, np.float32, 4 * misalign)
            self.check(self.L.plhip_box_coder_decode_f32(self.h, dp, dv, v4, dt, rows, cols, int(axis), int(bool(normalized)), y.ptr),
                       "box_coder_decode")
            return y.get()

    # ---- YOLOv3 heads (yolo_ops.hip)
    def yolo_box_launch(self, dx, dimg, shape, anchors, class_num, conf_thresh, downsample_ratio, clip_bbox, scale_x_y, dboxes, dscores):
        """plhip_yolo_box_f32 on device pointers; shape: x's [n, an * (5 + class_num), h, w].  Returns the status."""
        n, _ch, h, w = shape
        av = (C.c_int * max(1, len(anchors)))(*[int(v) for v in anchors])
        return self.L.plhip_yolo_box_f32(self.h, dx, dimg, n, len(anchors) // 2, int(class_num), h, w, av, float(conf_thresh),
                                         int(downsample_ratio), int(bool(clip_bbox)), float(scale_x_y), dboxes, dscores)

    def yolo_head_launch(self, dxs, dimg, shapes, anchors, class_num, conf_thresh, downsample_ratios, clip_bbox, scale_x_y, dboxes, dscores):
        """plhip_yolo_head_f32 on device pointers; shapes[i]: xs[i]'s [n, an_i * (5 + class_num), h_i, w_i].  Returns the status."""
        k = len(dxs)
        avs = [(C.c_int * max(1, len(a)))(*[int(v) for v in a]) for a in anchors]
        ptrs = (C.c_void_p * k)(*dxs)
        hs = (C.c_int * k)(*[s[2] for s in shapes])
        ws = (C.c_int * k)(*[s[3] for s in shapes])
        ap = (C.POINTER(C.c_int) * k)(*[C.cast(a, C.POINTER(C.c_int)) for a in avs])
        lens = (C.c_int * k)(*[len(a) for a in anchors])
        ratios = (C.c_int * k)(*[int(v) for v in downsample_ratios])
        return self.L.plhip_yolo_head_f32(self.h, ptrs, hs, ws, ap, lens, ratios, k, dimg, shapes[0][0] if k else 1, int(class_num), float(conf_thresh),
                                          int(bool(clip_bbox)), float(scale_x_y), dboxes, dscores)

    def yolo_box(self, x, img_size, anchors, class_num, conf_thresh, downsample_ratio, clip_bbox=True, scale_x_y=1.0, misalign=0):
        """plhip_yolo_box_f32: x [n, an * (5 + class_num), h, w] fp32, img_size [n, 2] int32 (height, width).  Returns
        (boxes [n, an * h * w, 4], scores [n, an * h * w, class_num]); the outputs hold 0xFF bytes before the call."""
        x = np.ascontiguousarray(x, np.float32)
        n, _ch, h, w = x.shape
        p = (len(anchors) // 2) * h * w
        with self.scope() as s:
            dx, dimg = s.put(x, off=4 * misalign), s.put(img_size, np.int32)
            boxes = s.out((n, p, 4), np.float32, 4 * misalign, fill=0xFF)
            scores = s.out((n, p, class_num), np.float32, 4 * misalign, fill=0xFF)
            self.check(self.yolo_box_launch(dx, dimg, x.shape, anchors, class_num, conf_thresh, downsample_ratio, clip_bbox, scale_x_y,
                                            boxes.ptr, scores.ptr), "yolo_box")
            return boxes.get(), scores.get()

    def yolo_head(self, xs, img_size, anchors, class_num, conf_thresh, downsample_ratios, clip_bbox=True, scale_x_y=1.0, misalign=0):
        """plhip_yolo_head_f32 of the feature maps xs[i] with anchors[i] and downsample_ratios[i].  Returns (boxes [n, P, 4],
        scores [n, class_num, P]); the outputs hold 0xFF bytes before the call."""
        xs = [np.ascontiguousarray(x, np.float32) for x in xs]
        n = xs[0].shape[0]
        p = sum((len(a) // 2) * x.shape[2] * x.shape[3] for a, x in zip(anchors, xs))
        with self.scope() as s:
            dxs, dimg = [s.put(x, off=4 * misalign) for x in xs], s.put(img_size, np.int32)
            boxes = s.out((n, p, 4), np.float32, 4 * misalign, fill=0xFF)
            scores = s.out((n, class_num, p), np.float32, 4 * misalign, fill=0xFF)
            self.check(self.yolo_head_launch(dxs, dimg, [x.shape for x in xs], anchors, class_num, conf_thresh, downsample_ratios,
                                             clip_bbox, scale_x_y, boxes.ptr, scores.ptr), "yolo_head")
            return boxes.get(), scores.get()

    def multiclass_nms(self, boxes, scores, desc, with_index=True, misalign=0):
        """plhip_multiclass_nms_f32: boxes [N, P, 4], scores in the layout desc's strides name.  Returns the padded device outputs
        (out [N, keep_top_k, 6], count [N], index [N, keep_top_k] or None)."""
        n, keep = desc.n, desc.keep_top_k
        nbytes = self.L.plhip_multiclass_nms_workspace_bytes(C.byref(desc))
        if nbytes == 0:
            raise PlhipError("multiclass_nms refused: %s" % self.L.plhip_last_error(None).decode())
        with self.scope() as s:
            db, dsc = s.put(boxes, np.float32, 4 * misalign), s.put(scores, np.float32, 4 * misalign)
            ws = s.alloc(nbytes)
            out, count = s.out((n, keep, 6), np.float32), s.out((n,), np.int32)
            index = s.out_opt(with_index, (n, keep), np.int32)
            self.check(self.L.plhip_multiclass_nms_f32(self.h, db, dsc, C.byref(desc), ws, out.ptr, index.ptr, count.ptr), "multiclass_nms")
            return out.get(), count.get(), index.get()

