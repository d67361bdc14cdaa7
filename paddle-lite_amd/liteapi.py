"""ctypes binding of libpaddle_lite_hip.so (lite/api/lite_capi.h): drives the C++ KernelLite classes and the mini
predictor.  No fallback: a missing library or a failing call raises."""
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libpaddle_lite_hip.so")
PREC_FLOAT, PREC_INT8, PREC_ANY = 1, 2, 4
PREC_INT32 = 3  # the ImgSize feed of yolo_box: lowering leaves it alone (no calib, an io_copy of 4-byte elements)
PREC_UINT8 = 9  # the uint8 image of graph_feed_image / graph_feed_frame (add_feed resizes it)
LAYOUT_NCHW, LAYOUT_ANY = 1, 2
# image formats of graph_feed_image == cv::ImageFormat (lite/utils/cv/paddle_image_preprocess.h) == plhip_image_format
IMG_RGBA, IMG_BGRA, IMG_RGB, IMG_BGR, IMG_GRAY = 0, 1, 2, 3, 4
IMG_NV21, IMG_NV12 = 11, 12  # frame formats of graph_feed_frame only


class LiteError(RuntimeError):
    pass


_lib = None


def load():
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise LiteError("%s is missing: run __graft_entry__.build()" % LIB_PATH)
    L = C.CDLL(LIB_PATH)
    vp, i32, f32, i64, cs = C.c_void_p, C.c_int, C.c_float, C.c_int64, C.c_char_p
    L.pllite_last_error.restype = cs
    L.pllite_registered_kernels.argtypes = [cs, i32, i32]
    L.pllite_adopt_stream.argtypes = [i32, vp]
    L.pllite_packed_weight_cache_stats.argtypes = [C.POINTER(C.c_long), C.POINTER(C.c_long)]
    L.pllite_packed_weight_cache_stats.restype = None
    L.pllite_predictor_create.argtypes = [i32]
    L.pllite_predictor_create.restype = vp
    L.pllite_predictor_destroy.argtypes = [vp]
    L.pllite_predictor_destroy.restype = None
    L.pllite_add_feed.argtypes = [vp, cs, C.POINTER(i64), i32, i32]
    L.pllite_add_io_copy.argtypes = [vp, cs, cs, i32]
    L.pllite_add_calib.argtypes = [vp, cs, cs, f32, i32]
    L.pllite_add_conv.argtypes = [vp, cs, cs, cs, vp, C.POINTER(i64), vp, C.POINTER(i32), C.POINTER(i32), i32,
                                  C.POINTER(i32), i32, i32, f32, f32, vp, i32, f32, i32, cs]
    L.pllite_add_fc.argtypes = [vp, cs, cs, vp, i32, i32, vp, f32, vp, i32, f32, i32, i32]
    L.pllite_add_global_avg_pool.argtypes = [vp, cs, cs]
    L.pllite_add_softmax.argtypes = [vp, cs, cs]
    L.pllite_add_pool.argtypes = [vp, cs, cs, cs, C.POINTER(i32), C.POINTER(i32), C.POINTER(i32), i32, i32, i32]
    L.pllite_add_elementwise_add.argtypes = [vp, cs, cs, cs, cs]
    L.pllite_predictor_create_planner.restype = vp
    L.pllite_graph_feed.argtypes = [vp, cs, C.POINTER(i64), i32, i32]
    L.pllite_graph_feed_image.argtypes = [vp, cs, i32, i32, i32, i32, C.POINTER(f32), C.POINTER(f32)]
    L.pllite_graph_feed_frame.argtypes = [vp, cs, i32, i32, i32, i32, i32, i32, C.POINTER(f32), C.POINTER(f32)]
    L.pllite_graph_conv.argtypes = [vp, cs, cs, cs, vp, C.POINTER(i64), vp, C.POINTER(i32), C.POINTER(i32), i32,
                                    C.POINTER(i32), i32, i32, f32, f32, vp, i32, cs]
    L.pllite_graph_conv2d_transpose.argtypes = [vp, cs, cs, vp, C.POINTER(i64), vp, C.POINTER(i32), C.POINTER(i32), i32,
                                                C.POINTER(i32), i32, i32, f32, f32, vp, i32, C.POINTER(i32)]
    L.pllite_graph_fc.argtypes = [vp, cs, cs, vp, i32, i32, vp, f32, vp, i32, i32]
    L.pllite_graph_pool.argtypes = [vp, cs, cs, cs, C.POINTER(i32), C.POINTER(i32), C.POINTER(i32), i32, i32, i32]
    L.pllite_graph_elementwise_add.argtypes = [vp, cs, cs, cs, cs]
    L.pllite_graph_softmax.argtypes = [vp, cs, cs]
    L.pllite_graph_activation.argtypes = [vp, cs, cs, cs]
    L.pllite_graph_elementwise_mul.argtypes = [vp, cs, cs, cs, i32]
    L.pllite_graph_set_fuse_hard_act.argtypes = [vp, i32]
    L.pllite_elementwise_mul_prepare.argtypes = [C.POINTER(i64), i32, C.POINTER(i64), i32, i32]
    L.pllite_add_activation.argtypes = [vp, cs, cs, cs, cs, f32, i32]
    L.pllite_add_elementwise_mul.argtypes = [vp, cs, cs, cs, i32, cs, f32, i32]
    L.pllite_graph_concat.argtypes = [vp, C.POINTER(cs), i32, cs, i32]
    L.pllite_graph_split.argtypes = [vp, cs, C.POINTER(cs), i32, i32, i32, C.POINTER(i32), i32]
    L.pllite_graph_shuffle_channel.argtypes = [vp, cs, cs, i32]
    L.pllite_graph_set_fuse_shuffle.argtypes = [vp, i32]
    L.pllite_add_concat.argtypes = [vp, C.POINTER(cs), i32, cs, i32]
    L.pllite_add_split.argtypes = [vp, cs, C.POINTER(cs), i32, i32, i32, C.POINTER(i32), i32]
    L.pllite_add_shuffle_channel.argtypes = [vp, cs, cs, i32]
    L.pllite_add_shuffle_unit.argtypes = [vp, cs, cs, cs, cs, cs, f32, i32]
    L.pllite_add_concat_calib.argtypes = [vp, C.POINTER(cs), i32, cs, i32, cs, f32, i32]
    L.pllite_graph_set_fuse_concat.argtypes = [vp, i32]
    L.pllite_graph_interp.argtypes = [vp, cs, cs, cs, i32, i32, f32, i32, i32]
    L.pllite_graph_arg_max.argtypes = [vp, cs, cs, i32, i32, i32]
    L.pllite_graph_set_fuse_interp_argmax.argtypes = [vp, i32]
    L.pllite_graph_set_fuse_interp_calib.argtypes = [vp, i32]
    L.pllite_add_interp.argtypes = [vp, cs, cs, cs, i32, i32, f32, i32, i32, cs, f32, i32]
    L.pllite_add_arg_max.argtypes = [vp, cs, cs, i32, i32, i32]
    L.pllite_add_interp_arg_max.argtypes = [vp, cs, cs, cs, i32, i32, f32, i32, i32, i32, i32]
    fp, ip = C.POINTER(f32), C.POINTER(i32)
    L.pllite_add_transpose.argtypes = [vp, cs, cs, ip, i32]
    L.pllite_add_reshape.argtypes = [vp, cs, cs, ip, i32]
    L.pllite_add_prior_box.argtypes = [vp, cs, cs, cs, cs, fp, i32, fp, i32, fp, i32, fp, i32, i32, f32, f32, f32, i32]
    L.pllite_add_box_coder.argtypes = [vp, cs, cs, cs, cs, fp, i32, i32]
    L.pllite_add_multiclass_nms.argtypes = [vp, cs, cs, cs, cs, i32, f32, i32, f32, f32, i32, i32, i32]
    L.pllite_add_concat_nhwc.argtypes = [vp, C.POINTER(cs), i32, cs, i32]
    L.pllite_graph_transpose.argtypes = [vp, cs, cs, ip, i32]
    L.pllite_graph_reshape.argtypes = [vp, cs, cs, ip, i32]
    L.pllite_graph_prior_box.argtypes = [vp, cs, cs, cs, cs, fp, i32, fp, i32, fp, i32, fp, i32, i32, f32, f32, f32, i32]
    L.pllite_graph_box_coder.argtypes = [vp, cs, cs, cs, cs, fp, i32, i32]
    L.pllite_graph_multiclass_nms.argtypes = [vp, cs, cs, cs, cs, i32, f32, i32, f32, f32, i32, i32]
    L.pllite_graph_set_fuse_detection_head.argtypes = [vp, i32]
    L.pllite_graph_yolo_box.argtypes = [vp, cs, cs, cs, cs, C.POINTER(i32), i32, i32, f32, i32, i32, f32]
    L.pllite_graph_set_fuse_yolo_head.argtypes = [vp, i32]
    L.pllite_graph_fetch.argtypes = [vp, cs]
    L.pllite_graph_set_fuse.argtypes = [vp, i32]
    L.pllite_graph_set_fuse_dwpw.argtypes = [vp, i32]
    L.pllite_graph_set_fuse_dwconv.argtypes = [vp, i32]
    L.pllite_graph_plan.argtypes = [vp, cs, i32]
    L.pllite_graph_lower.argtypes = [vp, cs, i32]
    L.pllite_load_model.argtypes = [vp, vp, i64, i32]
    L.pllite_graph_num_ops.argtypes = [vp]
    L.pllite_graph_op_params.argtypes = [vp, i32, cs, i32, vp, C.POINTER(i64), vp, C.POINTER(i32), vp, C.POINTER(i32),
                                         C.POINTER(f32), C.POINTER(i32), C.POINTER(f32)]
    L.pllite_set_input.argtypes = [vp, cs, vp, i64]
    L.pllite_run.argtypes = [vp, i32]
    L.pllite_run_graph.argtypes = [vp]
    L.pllite_sync.argtypes = [vp]
    L.pllite_num_instructions.argtypes = [vp]
    L.pllite_run_instruction.argtypes = [vp, i32]
    L.pllite_get_var.argtypes = [vp, cs, vp, i64, C.POINTER(i64), C.POINTER(i64), C.POINTER(i32)]
    L.pllite_var_device_ptr.argtypes = [vp, cs]
    L.pllite_var_device_ptr.restype = vp
    L.pllite_kernel_names.argtypes = [vp, cs, i32]
    L.pllite_time_instruction.argtypes = [vp, i32, i32, C.POINTER(f32), C.POINTER(f32), cs, i32]
    L.pllite_copy_var_to_device.argtypes = [vp, cs, vp, i64]
    _lib = L
    return L


def _ia(vals, t=C.c_int):
    return (t * len(vals))(*[int(v) for v in vals])


def _names(vals):
    return (C.c_char_p * len(vals))(*[v.encode() for v in vals])


def elementwise_mul_prepare(x_dims, y_dims, axis=0):
    """The elementwise_mul kernel class's PrepareForRun on these shapes (host only).  Raises LiteError where it refuses the broadcast."""
    L = load()
    if L.pllite_elementwise_mul_prepare(_ia(x_dims, C.c_int64), len(x_dims), _ia(y_dims, C.c_int64), len(y_dims), int(axis)) != 0:
        raise LiteError(L.pllite_last_error().decode())


class Predictor:
    """Mini CxxPredictor on TARGET(kHIP) (lite/api/hip_predictor.h)."""

    def __init__(self, device=0, stream=None, planner=False):
        """planner=True: an object that can only build and plan a graph (no device touched) — CPU tests of the
        lowering rules."""
        self.L = load()
        if planner:
            self.h = self.L.pllite_predictor_create_planner()
        else:
            if stream is not None:
                self._ck(self.L.pllite_adopt_stream(device, C.c_void_p(stream)))
            self.h = self.L.pllite_predictor_create(device)
        if not self.h:
            raise LiteError("pllite_predictor_create: " + self.L.pllite_last_error().decode())
        self._keep = []

    def _ck(self, rc):
        if rc != 0:
            raise LiteError(self.L.pllite_last_error().decode())

    def close(self):
        if self.h:
            self.L.pllite_predictor_destroy(self.h)
            self.h = None

    def add_feed(self, name, dims, precision=PREC_FLOAT):
        self._ck(self.L.pllite_add_feed(self.h, name.encode(), _ia(dims, C.c_int64), len(dims), precision))

    def add_io_copy(self, src, dst, host_to_device=True):
        self._ck(self.L.pllite_add_io_copy(self.h, src.encode(), dst.encode(), int(host_to_device)))

    def add_calib(self, src, dst, scale, fp32_to_int8=True):
        self._ck(self.L.pllite_add_calib(self.h, src.encode(), dst.encode(), scale, int(fp32_to_int8)))

    def add_conv(self, op_type, src, dst, w, bias, strides, paddings, dilations, groups, act, act_coef, input_scale,
                 weight_scale, output_scale, int8_out, padding_algorithm=""):
        w = np.ascontiguousarray(w, np.int8)
        ws = np.ascontiguousarray(weight_scale, np.float32)
        bp = None
        if bias is not None:
            bias = np.ascontiguousarray(bias, np.float32)
            bp = bias.ctypes.data_as(C.c_void_p)
        self._ck(self.L.pllite_add_conv(self.h, op_type.encode(), src.encode(), dst.encode(), w.ctypes.data_as(C.c_void_p),
                                        _ia(w.shape, C.c_int64), bp, _ia(strides), _ia(paddings), len(paddings),
                                        _ia(dilations), groups, act, act_coef, input_scale, ws.ctypes.data_as(C.c_void_p),
                                        ws.size, output_scale, int(int8_out), padding_algorithm.encode()))

    def add_fc(self, src, dst, w, bias, input_scale, weight_scale, output_scale, int8_out, relu):
        w = np.ascontiguousarray(w, np.int8)
        ws = np.ascontiguousarray(weight_scale, np.float32)
        bp = None
        if bias is not None:
            bias = np.ascontiguousarray(bias, np.float32)
            bp = bias.ctypes.data_as(C.c_void_p)
        self._ck(self.L.pllite_add_fc(self.h, src.encode(), dst.encode(), w.ctypes.data_as(C.c_void_p), w.shape[0],
                                      w.shape[1], bp, input_scale, ws.ctypes.data_as(C.c_void_p), ws.size, output_scale,
                                      int(int8_out), int(relu)))

    def add_global_avg_pool(self, src, dst):
        self._ck(self.L.pllite_add_global_avg_pool(self.h, src.encode(), dst.encode()))

    def add_softmax(self, src, dst):
        self._ck(self.L.pllite_add_softmax(self.h, src.encode(), dst.encode()))

    def add_pool(self, src, dst, pooling_type, ksize, strides, paddings, global_pooling=False, exclusive=True,
                 ceil_mode=False):
        self._ck(self.L.pllite_add_pool(self.h, src.encode(), dst.encode(), pooling_type.encode(), _ia(ksize), _ia(strides),
                                        _ia(paddings), int(global_pooling), int(exclusive), int(ceil_mode)))

    def add_elementwise_add(self, x, y, dst, act_type=""):
        self._ck(self.L.pllite_add_elementwise_add(self.h, x.encode(), y.encode(), dst.encode(), act_type.encode()))

    def add_activation(self, op_type, src, dst, calib_out="", calib_scale=1.0, drop_fp32=False):
        """hard_swish | hard_sigmoid; calib_out: the int8 alias (the calib behind the op in the same launch writes that variable)."""
        self._ck(self.L.pllite_add_activation(self.h, op_type.encode(), src.encode(), dst.encode(), calib_out.encode(),
                                              calib_scale, int(drop_fp32)))

    def add_elementwise_mul(self, x, y, dst, axis=0, calib_out="", calib_scale=1.0, drop_fp32=False):
        self._ck(self.L.pllite_add_elementwise_mul(self.h, x.encode(), y.encode(), dst.encode(), int(axis), calib_out.encode(),
                                                   calib_scale, int(drop_fp32)))

    def add_concat(self, srcs, dst, axis=1):
        self._ck(self.L.pllite_add_concat(self.h, _names(srcs), len(srcs), dst.encode(), int(axis)))

    def add_concat_calib(self, srcs, dst, axis, calib_out, calib_scale, drop_fp32=False):
        """concat -> calib[fp32_to_int8] in one launch (concat/int8): dst the fp32 tensor, calib_out its int8 image; drop_fp32: dst
        is not written."""
        self._ck(self.L.pllite_add_concat_calib(self.h, _names(srcs), len(srcs), dst.encode(), int(axis), calib_out.encode(),
                                                calib_scale, int(drop_fp32)))

    def add_split(self, src, dsts, axis=1, num=0, sections=()):
        """num > 0: equal parts; else one section per output."""
        self._ck(self.L.pllite_add_split(self.h, src.encode(), _names(dsts), len(dsts), int(axis), int(num), _ia(sections), len(sections)))

    def add_shuffle_channel(self, src, dst, group):
        self._ck(self.L.pllite_add_shuffle_channel(self.h, src.encode(), dst.encode(), int(group)))

    def add_shuffle_unit(self, a, b, lo, hi, calib_out="", calib_scale=1.0, drop_fp32=False):
        """concat([a, b], 1) -> shuffle_channel(2) and what follows in one launch.  lo == "": shuffle_channel/int8, `hi` the shuffled
        tensor; else shuffle_channel/unit, lo / hi the two halves.  calib_out: the int8 image of `hi`; drop_fp32: `hi` is not written."""
        self._ck(self.L.pllite_add_shuffle_unit(self.h, a.encode(), b.encode(), lo.encode(), hi.encode(), calib_out.encode(),
                                                calib_scale, int(drop_fp32)))

    def add_interp(self, op_type, src, dst, out_hw=None, scale=0.0, align_corners=True, align_mode=1, calib_out="", calib_scale=1.0,
                   drop_fp32=False):
        """bilinear_interp | nearest_interp to out_hw, or by `scale` (int(in * scale)).  calib_out: the int8 alias (the calib behind the
        interp in the same launch writes that variable); drop_fp32: dst is not written."""
        oh, ow = out_hw if out_hw is not None else (-1, -1)
        self._ck(self.L.pllite_add_interp(self.h, op_type.encode(), src.encode(), dst.encode(), int(oh), int(ow), float(scale),
                                          int(align_corners), int(align_mode), calib_out.encode(), calib_scale, int(drop_fp32)))

    def add_arg_max(self, src, dst, axis, dtype=-1, keepdims=False):
        """dtype as ArgmaxParam's: -1 or 3 int64 labels, 2 int32."""
        self._ck(self.L.pllite_add_arg_max(self.h, src.encode(), dst.encode(), int(axis), int(dtype), int(keepdims)))

    def add_interp_arg_max(self, op_type, src, dst, out_hw=None, scale=0.0, align_corners=True, align_mode=1, dtype=-1, keepdims=False):
        """interp -> arg_max(axis 1) in one launch (arg_max/interp): src is the interp's low-resolution input."""
        oh, ow = out_hw if out_hw is not None else (-1, -1)
        self._ck(self.L.pllite_add_interp_arg_max(self.h, op_type.encode(), src.encode(), dst.encode(), int(oh), int(ow), float(scale),
                                                  int(align_corners), int(align_mode), int(dtype), int(keepdims)))

    # ---- detection heads (lite/kernels/hip/detection_compute.cc)
    def add_transpose(self, src, dst, perm):
        self._ck(self.L.pllite_add_transpose(self.h, src.encode(), dst.encode(), _ints(perm), len(perm)))

    def add_reshape(self, src, dst, shape):
        """The shape attribute: 0 copies the input's dim, one -1 is inferred.  No launch: dst shares src's memory."""
        self._ck(self.L.pllite_add_reshape(self.h, src.encode(), dst.encode(), _ints(shape), len(shape)))

    def add_prior_box(self, src, image, boxes, variances, min_sizes, max_sizes=(), aspect_ratios=(), variance=(0.1, 0.1, 0.2, 0.2), flip=True,
                      clip=False, step_w=0.0, step_h=0.0, offset=0.5, min_max_aspect_ratios_order=False):
        """Boxes and Variances [H, W, prior_num, 4] of the feature map src for the image; computed on the host once per shape."""
        self._ck(self.L.pllite_add_prior_box(self.h, src.encode(), image.encode(), boxes.encode(), variances.encode(), *_prior_box_args(
            min_sizes, max_sizes, aspect_ratios, variance, flip, clip, step_w, step_h, offset, min_max_aspect_ratios_order)))

    def add_box_coder(self, prior, target, dst, prior_var="", variance=None, axis=0, normalized=True):
        """decode_center_size.  The variance: the prior_var tensor, else the 4 values of `variance`, else none."""
        self._ck(self.L.pllite_add_box_coder(self.h, prior.encode(), prior_var.encode(), target.encode(), dst.encode(),
                                             _variance4(variance), int(axis), int(normalized)))

    def add_multiclass_nms(self, boxes, scores, dst, background_label=0, score_threshold=0.0, nms_top_k=-1, nms_threshold=0.3, nms_eta=1.0,
                           keep_top_k=100, normalized=True, index="", scores_npc=False):
        """dst [N, keep_top_k, 6] padded with -1, the counts in the int32 variable dst + "/count", index [N, keep_top_k] int32."""
        self._ck(self.L.pllite_add_multiclass_nms(self.h, boxes.encode(), scores.encode(), dst.encode(), index.encode(), int(background_label),
                                                  float(score_threshold), int(nms_top_k), float(nms_threshold), float(nms_eta), int(keep_top_k),
                                                  int(normalized), int(scores_npc)))

    def add_concat_nhwc(self, srcs, dst, k):
        """transpose(0,2,3,1) -> reshape([0,-1,k]) -> concat(axis 1) of NCHW variables in one launch (concat/nhwc)."""
        arr = (C.c_char_p * len(srcs))(*[s.encode() for s in srcs])
        self._ck(self.L.pllite_add_concat_nhwc(self.h, arr, len(srcs), dst.encode(), int(k)))

    def detections(self, name, index=None, suffix="/host"):
        """The reference's LoD form of a multiclass_nms output whose host copies were fetched: (rows [num_kept, 6], the batch offsets,
        the index column or None); see detections_lod."""
        out = self.get_var(name + suffix, np.float32)
        count = self.get_var(name + "/count" + suffix, np.int32)
        idx = self.get_var(index + suffix, np.int32) if index else None
        return detections_lod(out, count, idx)

    # ---- graph mode: ops as the optimiser sees them; graph_lower() applies the reference's kernel-pick / cast rules
    def graph_feed(self, name, dims, precision=PREC_FLOAT):
        self._ck(self.L.pllite_graph_feed(self.h, name.encode(), _ia(dims, C.c_int64), len(dims), precision))

    def graph_feed_image(self, name, n, h, w, fmt, means, scales):
        """A feed that takes a decoded uint8 image [n, h, w, cs] (fmt: IMG_*) instead of the normalised fp32 tensor: the ops
        name `name` as the NCHW tensor (ImagePreprocess::image_to_tensor runs on the device); set_input(name, uint8 array).
        means / scales: per source byte of a pixel (the first only for IMG_GRAY)."""
        m = (C.c_float * 3)(*(list(map(float, means)) + [0.0] * 3)[:3])
        s = (C.c_float * 3)(*(list(map(float, scales)) + [0.0] * 3)[:3])
        self._ck(self.L.pllite_graph_feed_image(self.h, name.encode(), int(n), int(h), int(w), int(fmt), m, s))

    def graph_feed_frame(self, name, n, src_h, src_w, src_fmt, dst_h, dst_w, means, scales):
        """A feed that takes a decoder's / camera's frame: n frames of src_h x src_w in src_fmt, an interleaved IMG_* format (uint8
        [n, src_h, src_w, cs]) or IMG_NV12 / IMG_NV21 (uint8 [n, src_h * 3 / 2, src_w]).  Convert, bilinear resize to dst_h x dst_w and
        image_to_tensor run on the device; the ops name `name` as the NCHW tensor, as with graph_feed_image.  means / scales: per
        byte of the pixel that is normalised (b, g, r for an NV frame)."""
        m = (C.c_float * 3)(*(list(map(float, means)) + [0.0] * 3)[:3])
        s = (C.c_float * 3)(*(list(map(float, scales)) + [0.0] * 3)[:3])
        self._ck(self.L.pllite_graph_feed_frame(self.h, name.encode(), int(n), int(src_h), int(src_w), int(src_fmt), int(dst_h),
                                                int(dst_w), m, s))

    def graph_conv(self, op_type, src, dst, w, bias, strides, paddings, dilations, groups, act, act_coef, input_scale,
                   weight_scale, padding_algorithm=""):
        w = np.ascontiguousarray(w, np.int8)
        ws = np.ascontiguousarray(weight_scale, np.float32)
        bp = None
        if bias is not None:
            bias = np.ascontiguousarray(bias, np.float32)
            bp = bias.ctypes.data_as(C.c_void_p)
        self._ck(self.L.pllite_graph_conv(self.h, op_type.encode(), src.encode(), dst.encode(), w.ctypes.data_as(C.c_void_p),
                                          _ia(w.shape, C.c_int64), bp, _ia(strides), _ia(paddings), len(paddings),
                                          _ia(dilations), groups, act, act_coef, input_scale, ws.ctypes.data_as(C.c_void_p),
                                          ws.size, padding_algorithm.encode()))

    def graph_conv2d_transpose(self, src, dst, w, bias, strides, paddings, dilations, groups, act, act_coef, input_scale,
                               weight_scale, output_size=None):
        """conv2d_transpose: w int8 [cin, cout / groups, kh, kw], bias per output channel or None, output_size (h, w) or None."""
        w = np.ascontiguousarray(w, np.int8)
        ws = np.ascontiguousarray(weight_scale, np.float32)
        bp = None
        if bias is not None:
            bias = np.ascontiguousarray(bias, np.float32)
            bp = bias.ctypes.data_as(C.c_void_p)
        self._ck(self.L.pllite_graph_conv2d_transpose(self.h, src.encode(), dst.encode(), w.ctypes.data_as(C.c_void_p),
                                                      _ia(w.shape, C.c_int64), bp, _ia(strides), _ia(paddings), len(paddings),
                                                      _ia(dilations), groups, act, act_coef, input_scale,
                                                      ws.ctypes.data_as(C.c_void_p), ws.size,
                                                      _ia(output_size) if output_size else None))

    def graph_fc(self, src, dst, w, bias, input_scale, weight_scale, relu=False):
        w = np.ascontiguousarray(w, np.int8)
        ws = np.ascontiguousarray(weight_scale, np.float32)
        bp = None
        if bias is not None:
            bias = np.ascontiguousarray(bias, np.float32)
            bp = bias.ctypes.data_as(C.c_void_p)
        self._ck(self.L.pllite_graph_fc(self.h, src.encode(), dst.encode(), w.ctypes.data_as(C.c_void_p), w.shape[0],
                                        w.shape[1], bp, input_scale, ws.ctypes.data_as(C.c_void_p), ws.size, int(relu)))

    def graph_pool(self, src, dst, pooling_type, ksize, strides, paddings, global_pooling=False, exclusive=True,
                   ceil_mode=False):
        self._ck(self.L.pllite_graph_pool(self.h, src.encode(), dst.encode(), pooling_type.encode(), _ia(ksize),
                                          _ia(strides), _ia(paddings), int(global_pooling), int(exclusive), int(ceil_mode)))

    def graph_elementwise_add(self, x, y, dst, act_type=""):
        self._ck(self.L.pllite_graph_elementwise_add(self.h, x.encode(), y.encode(), dst.encode(), act_type.encode()))

    def graph_softmax(self, src, dst):
        self._ck(self.L.pllite_graph_softmax(self.h, src.encode(), dst.encode()))

    def graph_hard_swish(self, src, dst):
        self._ck(self.L.pllite_graph_activation(self.h, b"hard_swish", src.encode(), dst.encode()))

    def graph_hard_sigmoid(self, src, dst):
        self._ck(self.L.pllite_graph_activation(self.h, b"hard_sigmoid", src.encode(), dst.encode()))

    def graph_elementwise_mul(self, x, y, dst, axis=0):
        """x [N, C, H, W] times y [N, C, 1, 1] / [N, C] (axis 0), or y of x's shape."""
        self._ck(self.L.pllite_graph_elementwise_mul(self.h, x.encode(), y.encode(), dst.encode(), int(axis)))

    def graph_concat(self, srcs, dst, axis=1):
        self._ck(self.L.pllite_graph_concat(self.h, _names(srcs), len(srcs), dst.encode(), int(axis)))

    def graph_split(self, src, dsts, axis=1, num=0, sections=()):
        """num > 0: `num` equal parts of the axis; else one section per output."""
        self._ck(self.L.pllite_graph_split(self.h, src.encode(), _names(dsts), len(dsts), int(axis), int(num), _ia(sections), len(sections)))

    def graph_shuffle_channel(self, src, dst, group):
        self._ck(self.L.pllite_graph_shuffle_channel(self.h, src.encode(), dst.encode(), int(group)))

    def graph_set_fuse_shuffle(self, on):
        """Fusion K (default on; with graph_set_fuse(True) only): concat -> shuffle_channel(2) -> split -> calib becomes one
        shuffle_channel/unit instruction (K1), concat -> shuffle_channel(2) -> calib one shuffle_channel/int8 instruction (K2)."""
        self._ck(self.L.pllite_graph_set_fuse_shuffle(self.h, int(on)))

    def graph_set_fuse_concat(self, on):
        """Fusion L (default on; with graph_set_fuse(True) only): a concat takes the calib[fp32_to_int8] that reads it over (concat/int8, L1), and a
        max pool behind the concat whose only reader is a calib of the same scale becomes an int8 max pool on the int8 copy (L2)."""
        self._ck(self.L.pllite_graph_set_fuse_concat(self.h, int(on)))

    def graph_interp(self, op_type, src, dst, out_hw=None, scale=0.0, align_corners=True, align_mode=1):
        """bilinear_interp | nearest_interp to out_hw, or by `scale` (int(in * scale)); the reference's attribute defaults."""
        oh, ow = out_hw if out_hw is not None else (-1, -1)
        self._ck(self.L.pllite_graph_interp(self.h, op_type.encode(), src.encode(), dst.encode(), int(oh), int(ow), float(scale),
                                            int(align_corners), int(align_mode)))

    def graph_arg_max(self, src, dst, axis, dtype=-1, keepdims=False):
        """dtype as ArgmaxParam's: -1 or 3 int64 labels, 2 int32."""
        self._ck(self.L.pllite_graph_arg_max(self.h, src.encode(), dst.encode(), int(axis), int(dtype), int(keepdims)))

    def graph_set_fuse_interp_argmax(self, on):
        """Fusion M (default on; with graph_set_fuse(True) only): an interp whose only reader is arg_max(axis 1) becomes one
        arg_max/interp instruction on the low-resolution tensor; the resampled tensor is never written."""
        self._ck(self.L.pllite_graph_set_fuse_interp_argmax(self.h, int(on)))

    def graph_set_fuse_interp_calib(self, on):
        """Fusion N (default on; with graph_set_fuse(True) only): an interp takes the calib[fp32_to_int8] that reads it over
        (bilinear_interp/int8, nearest_interp/int8)."""
        self._ck(self.L.pllite_graph_set_fuse_interp_calib(self.h, int(on)))

    def graph_transpose(self, src, dst, perm):
        self._ck(self.L.pllite_graph_transpose(self.h, src.encode(), dst.encode(), _ints(perm), len(perm)))

    def graph_reshape(self, src, dst, shape):
        self._ck(self.L.pllite_graph_reshape(self.h, src.encode(), dst.encode(), _ints(shape), len(shape)))

    def graph_prior_box(self, src, image, boxes, variances, min_sizes, max_sizes=(), aspect_ratios=(), variance=(0.1, 0.1, 0.2, 0.2), flip=True,
                        clip=False, step_w=0.0, step_h=0.0, offset=0.5, min_max_aspect_ratios_order=False):
        self._ck(self.L.pllite_graph_prior_box(self.h, src.encode(), image.encode(), boxes.encode(), variances.encode(), *_prior_box_args(
            min_sizes, max_sizes, aspect_ratios, variance, flip, clip, step_w, step_h, offset, min_max_aspect_ratios_order)))

    def graph_box_coder(self, prior, target, dst, prior_var="", variance=None, axis=0, normalized=True):
        self._ck(self.L.pllite_graph_box_coder(self.h, prior.encode(), prior_var.encode(), target.encode(), dst.encode(),
                                               _variance4(variance), int(axis), int(normalized)))

    def graph_multiclass_nms(self, boxes, scores, dst, background_label=0, score_threshold=0.0, nms_top_k=-1, nms_threshold=0.3, nms_eta=1.0,
                             keep_top_k=100, normalized=True, index=""):
        """The count variable is dst + "/count" (fetch it beside dst)."""
        self._ck(self.L.pllite_graph_multiclass_nms(self.h, boxes.encode(), scores.encode(), dst.encode(), index.encode(), int(background_label),
                                                    float(score_threshold), int(nms_top_k), float(nms_threshold), float(nms_eta), int(keep_top_k),
                                                    int(normalized)))

    def graph_yolo_box(self, x, img_size, boxes, scores, anchors, class_num, conf_thresh, downsample_ratio, clip_bbox=True, scale_x_y=1.0):
        """yolo_box: x [N, an * (5 + class_num), H, W]; img_size a feed of PREC_INT32 and dims [N, 2] = (height, width) per image;
        anchors: (width, height) pairs as a flat list of ints.  boxes [N, an * H * W, 4], scores [N, an * H * W, class_num]."""
        self._ck(self.L.pllite_graph_yolo_box(self.h, x.encode(), img_size.encode(), boxes.encode(), scores.encode(), _ints(anchors), len(anchors),
                                              int(class_num), float(conf_thresh), int(downsample_ratio), int(bool(clip_bbox)), float(scale_x_y)))

    def graph_set_fuse_yolo_head(self, on):
        """Fusion P (default on; with graph_set_fuse(True) only): the yolo_box ops of a YOLOv3 head, the concats of their Boxes and
        Scores and the transpose(0,2,1) in front of multiclass_nms become one yolo_box/head instruction."""
        self._ck(self.L.pllite_graph_set_fuse_yolo_head(self.h, int(on)))

    def graph_set_fuse_detection_head(self, on):
        """Fusion O (default on; with graph_set_fuse(True) only): (O1) a concat(axis 1) of transpose(0,2,3,1) ->
        reshape([0,-1,k]) chains becomes one concat/nhwc instruction; (O2) a transpose(0,2,1) in front of multiclass_nms's scores
        disappears into the kernel's strides."""
        self._ck(self.L.pllite_graph_set_fuse_detection_head(self.h, int(on)))

    def graph_set_fuse_hard_act(self, on):
        """Fusions J1 / J2 / J3 (default off; with graph_set_fuse(True) only): hard_swish / elementwise_mul take the calib[fp32_to_int8]
        behind them over, hard_sigmoid the excite chain calib -> conv 1x1 -> conv 1x1 in front of it."""
        self._ck(self.L.pllite_graph_set_fuse_hard_act(self.h, int(on)))

    def graph_set_fuse(self, on):
        self._ck(self.L.pllite_graph_set_fuse(self.h, int(on)))

    def graph_set_fuse_dwpw(self, on):
        """Opt-in: a depthwise conv [int8_out] takes its sole 1x1 consumer over (one instruction, one launch where the
        shape fits the fused kernel)."""
        self._ck(self.L.pllite_graph_set_fuse_dwpw(self.h, int(on)))

    def graph_set_fuse_dwconv(self, on):
        """Opt-in (default off), fusion G: a depthwise conv [int8_out] takes its sole 1x1 consumer over together with that
        conv's fused tail (residual add, calib copy), one launch of plhip_dw_conv1x1_fused_int8 where the shape fits."""
        self._ck(self.L.pllite_graph_set_fuse_dwconv(self.h, int(on)))

    def graph_fetch(self, name):
        self._ck(self.L.pllite_graph_fetch(self.h, name.encode()))

    def graph_plan(self):
        buf = C.create_string_buffer(1 << 18)
        self._ck(self.L.pllite_graph_plan(self.h, buf, len(buf)))
        return [s for s in buf.value.decode().split("\n") if s]

    def graph_lower(self):
        buf = C.create_string_buffer(1 << 16)
        self._ck(self.L.pllite_graph_lower(self.h, buf, len(buf)))
        return [s for s in buf.value.decode().split("\n") if s]

    def load_model(self, blob, batch):
        """Parse a PLHIPM01 container (bytes) into the predictor's graph (lite/model_parser/hip_model.h)."""
        buf = (C.c_char * len(blob)).from_buffer_copy(blob)
        self._ck(self.L.pllite_load_model(self.h, buf, len(blob), batch))

    def graph_ops(self):
        """[(type, w int8 flat, bias or None, weight_scale, input_scale, act, act_coef)] of the graph's ops."""
        res = []
        for i in range(self.L.pllite_graph_num_ops(self.h)):
            t = C.create_string_buffer(64)
            nw, nb, ns = C.c_int64(), C.c_int(), C.c_int()
            isc, act, coef = C.c_float(), C.c_int(), C.c_float()
            self._ck(self.L.pllite_graph_op_params(self.h, i, t, 64, None, C.byref(nw), None, C.byref(nb), None, C.byref(ns),
                                                   C.byref(isc), C.byref(act), C.byref(coef)))
            w = np.empty(nw.value, np.int8)
            b = np.empty(nb.value, np.float32)
            s_ = np.empty(ns.value, np.float32)
            self._ck(self.L.pllite_graph_op_params(self.h, i, None, 0, w.ctypes.data_as(C.c_void_p), None,
                                                   b.ctypes.data_as(C.c_void_p), None, s_.ctypes.data_as(C.c_void_p), None, None, None, None))
            res.append((t.value.decode(), w, b if nb.value else None, s_, isc.value, act.value, coef.value))
        return res

    def set_input(self, name, arr):
        arr = np.ascontiguousarray(arr)
        self._ck(self.L.pllite_set_input(self.h, name.encode(), arr.ctypes.data_as(C.c_void_p), arr.nbytes))

    def run(self, skip_io_copy=False):
        self._ck(self.L.pllite_run(self.h, int(skip_io_copy)))

    def run_graph(self):
        """Device part of the program as ONE recorded launch graph (records on the first call, after a plain run())."""
        self._ck(self.L.pllite_run_graph(self.h))

    def sync(self):
        self._ck(self.L.pllite_sync(self.h))

    def num_instructions(self):
        return self.L.pllite_num_instructions(self.h)

    def run_instruction(self, i):
        self._ck(self.L.pllite_run_instruction(self.h, i))

    def get_var(self, name, dtype, max_bytes=1 << 30):
        nb, nd = C.c_int64(), C.c_int()
        dims = (C.c_int64 * 4)()
        # first query the size with a tiny probe: capacity check raises, so allocate generously via dims
        buf = np.empty(max_bytes if max_bytes < (1 << 24) else (1 << 24), np.uint8)
        rc = self.L.pllite_get_var(self.h, name.encode(), buf.ctypes.data_as(C.c_void_p), buf.nbytes, C.byref(nb), dims, C.byref(nd))
        if rc != 0 and "too small" in self.L.pllite_last_error().decode():
            buf = np.empty(max_bytes, np.uint8)
            rc = self.L.pllite_get_var(self.h, name.encode(), buf.ctypes.data_as(C.c_void_p), buf.nbytes, C.byref(nb), dims, C.byref(nd))
        self._ck(rc)
        shape = tuple(dims[i] for i in range(nd.value))
        return buf[:nb.value].view(dtype).reshape(shape).copy()

    def device_ptr(self, name):
        return self.L.pllite_var_device_ptr(self.h, name.encode())

    def copy_var_to_device(self, name, dst_ptr, nbytes):
        self._ck(self.L.pllite_copy_var_to_device(self.h, name.encode(), C.c_void_p(dst_ptr), nbytes))

    def time_instruction(self, index, reps=10):
        """(avg_ms, min_ms, kernel_func_name) of one instruction, timed with DeviceTimer<kHIP> (lite/core/profile/timer.h)."""
        a, m = C.c_float(), C.c_float()
        buf = C.create_string_buffer(256)
        self._ck(self.L.pllite_time_instruction(self.h, index, reps, C.byref(a), C.byref(m), buf, len(buf)))
        return a.value, m.value, buf.value.decode()

    def kernel_names(self):
        buf = C.create_string_buffer(1 << 16)
        self._ck(self.L.pllite_kernel_names(self.h, buf, len(buf)))
        return [s for s in buf.value.decode().split("\n") if s]


def _ints(v):
    return (C.c_int * len(v))(*[int(x) for x in v])


def _floats(v):
    return (C.c_float * len(v))(*[float(x) for x in v])


def _variance4(v):
    """The 4-float variance attribute of box_coder as the C API takes it, or None."""
    if v is None:
        return None
    if len(v) != 4:
        raise ValueError("box_coder: the variance attribute has %d values, not 4" % len(v))
    return _floats(v)


def _prior_box_args(min_sizes, max_sizes, aspect_ratios, variance, flip, clip, step_w, step_h, offset, order):
    if len(variance) != 4:
        raise ValueError("prior_box: %d variances, not 4" % len(variance))
    return (_floats(min_sizes), len(min_sizes), _floats(max_sizes), len(max_sizes), _floats(aspect_ratios), len(aspect_ratios), _floats(variance),
            int(flip), int(clip), float(step_w), float(step_h), float(offset), int(order))


def detections_lod(out, count, index=None):
    """The reference's output form of multiclass_nms (lite/kernels/host/multiclass_nms_compute.cc:360-418) from the device's padded
    one: out [N, keep_top_k, 6], count [N], index [N, keep_top_k] or None -> (rows [num_kept, 6], the batch offsets [N + 1], the index
    column [num_kept, 1] or None).  No detection in any image: rows [[-1]] with offsets [0, 1] without an index output; rows [0, 6],
    offsets of zeros and index [0, 1] with one."""
    out = np.asarray(out, np.float32)
    count = np.asarray(count).astype(np.int64).reshape(-1)
    if out.ndim != 3 or out.shape[2] != 6 or out.shape[0] != count.size or (count < 0).any() or (count > out.shape[1]).any():
        raise ValueError("detections_lod: out %r and count %r do not belong together" % (out.shape, count.tolist()))
    offsets = np.concatenate([[0], np.cumsum(count)]).astype(np.int64)
    if offsets[-1] == 0:
        if index is None:
            return np.array([[-1]], np.float32), np.array([0, 1], np.int64), None
        return np.zeros((0, 6), np.float32), offsets, np.zeros((0, 1), np.int32)
    rows = np.concatenate([out[i, :count[i]] for i in range(count.size)], axis=0)
    if index is None:
        return rows, offsets, None
    index = np.asarray(index).reshape(count.size, -1)
    return rows, offsets, np.concatenate([index[i, :count[i]] for i in range(count.size)]).astype(np.int32)[:, None]
