// plhip_capi_ops.hip — the C ABI (include/plhip.h), part 4 of 4: fc, calib, pooling, softmax, elementwise add, the hard activations,
// squeeze-excite, concat / split / shuffle_channel, interp / arg_max, and the detection heads (transpose, concat_nhwc, box_coder,
// multiclass_nms) and the YOLOv3 heads (yolo_box, yolo_head).  Argument validation and one launch each (multiclass_nms: two).
#include "plhip_capi.h"

#include <vector>

extern "C" {

// ------------------------------------------------------------------ fc
size_t plhip_fc_packed_weight_bytes(int k, int n) {
  if (k < 1 || n < 1) return 0;
  return plhip::fc_packed_bytes(k, n);  // [dot4 layout][MFMA A fragments]
}

plhip_status plhip_pack_fc_weights(plhip_ctx* ctx, int k, int n, const int8_t* w_kn, void* w_packed) {
  if (!ctx || !w_kn || !w_packed || k < 1 || n < 1) return fail(ctx, PLHIP_ERR_INVALID, "plhip_pack_fc_weights: bad argument");
  plhip::launch_pack_fc(w_kn, (int8_t*)w_packed, k, n, ctx->stream);
  LAUNCHCHK(ctx, "pack_fc");
  return PLHIP_OK;
}

plhip_status plhip_fc_int8(plhip_ctx* ctx, int m, int k, int n, const int8_t* x, const void* w_packed, const float* scale,
                           const float* bias, int relu, void* y, plhip_out_kind out) {
  if (!ctx || !x || !w_packed || !y || m < 1 || k < 1 || n < 1) return fail(ctx, PLHIP_ERR_INVALID, "plhip_fc_int8: bad argument");
  if (plhip_status st = check_out_scale_act(ctx, "plhip_fc_int8", out, false, scale, "scale", nullptr)) return st;
  if (!aligned(w_packed, 4)) return fail(ctx, PLHIP_ERR_INVALID, "plhip_fc_int8: packed weights must be 4-byte aligned");
  plhip::launch_fc(x, (const int8_t*)w_packed, scale, bias, y, m, k, n, relu, (int)out, ctx->stream);
  LAUNCHCHK(ctx, "fc_i8");
  return PLHIP_OK;
}

// ------------------------------------------------------------------ calib / pool / softmax
plhip_status plhip_calib_f32_to_i8(plhip_ctx* ctx, const float* x, int8_t* y, float scale, int64_t count) {
  if (!ctx || !x || !y || count < 0 || !(scale > 0.f)) return fail(ctx, PLHIP_ERR_INVALID, "plhip_calib_f32_to_i8: bad argument");
  if (count == 0) return PLHIP_OK;
  plhip::launch_calib_f32_to_i8(x, y, scale, count, ctx->stream);
  LAUNCHCHK(ctx, "calib_f32_to_i8");
  return PLHIP_OK;
}

plhip_status plhip_calib_i8_to_f32(plhip_ctx* ctx, const int8_t* x, float* y, float scale, int64_t count) {
  if (!ctx || !x || !y || count < 0) return fail(ctx, PLHIP_ERR_INVALID, "plhip_calib_i8_to_f32: bad argument");
  if (count == 0) return PLHIP_OK;
  plhip::launch_calib_i8_to_f32(x, y, scale, count, ctx->stream);
  LAUNCHCHK(ctx, "calib_i8_to_f32");
  return PLHIP_OK;
}

plhip_status plhip_global_avg_pool_f32(plhip_ctx* ctx, const float* x, int nc, int spatial, float* y) {
  if (!ctx || !x || !y || nc < 1 || spatial < 1) return fail(ctx, PLHIP_ERR_INVALID, "plhip_global_avg_pool_f32: bad argument");
  plhip::launch_global_avg_pool(x, nc, spatial, y, ctx->stream);
  LAUNCHCHK(ctx, "global_avg_pool");
  return PLHIP_OK;
}

plhip_status plhip_softmax_f32(plhip_ctx* ctx, const float* x, int rows, int cols, float* y) {
  if (!ctx || !x || !y || rows < 1 || cols < 1) return fail(ctx, PLHIP_ERR_INVALID, "plhip_softmax_f32: bad argument");
  plhip::launch_softmax(x, rows, cols, y, ctx->stream);
  LAUNCHCHK(ctx, "softmax");
  return PLHIP_OK;
}

static plhip_status pool2d_impl(plhip_ctx* ctx, const plhip_pool_desc* d, const void* x, void* y, bool i8);
plhip_status plhip_pool2d_f32(plhip_ctx* ctx, const plhip_pool_desc* d, const float* x, float* y) {
  return pool2d_impl(ctx, d, x, y, false);
}
plhip_status plhip_pool2d_max_i8(plhip_ctx* ctx, const plhip_pool_desc* d, const int8_t* x, int8_t* y) {
  if (d && !d->is_max) return fail(ctx, PLHIP_ERR_UNSUPPORTED, "plhip_pool2d_max_i8: max pooling only (avg does not commute with the quantiser)");
  return pool2d_impl(ctx, d, x, y, true);
}
static plhip_status pool2d_impl(plhip_ctx* ctx, const plhip_pool_desc* d, const void* x, void* y, bool i8) {
  if (!ctx || !d || !x || !y) return fail(ctx, PLHIP_ERR_INVALID, "plhip_pool2d_f32: null argument");
  if (d->planes < 1 || d->h < 1 || d->w < 1 || d->oh < 1 || d->ow < 1 || d->kh < 1 || d->kw < 1 || d->stride[0] < 1 ||
      d->stride[1] < 1 || d->pad[0] < 0 || d->pad[1] < 0 || d->pad[2] < 0 || d->pad[3] < 0)
    return fail(ctx, PLHIP_ERR_INVALID, "plhip_pool2d_f32: bad descriptor");
  // every window must start inside the padded image (PoolOutputSize guarantees it, ceil_mode included; windows that
  // only cover padding yield 0 like pooling_basic)
  if ((d->oh - 1) * d->stride[0] - d->pad[0] >= d->h + d->pad[1] || (d->ow - 1) * d->stride[1] - d->pad[2] >= d->w + d->pad[3])
    return fail(ctx, PLHIP_ERR_INVALID, "plhip_pool2d_f32: output dims do not match the window geometry");
  if ((size_t)d->h * d->w >= ((size_t)1 << 31) || (size_t)d->oh * d->ow >= ((size_t)1 << 31))
    return fail(ctx, PLHIP_ERR_UNSUPPORTED, "plhip_pool2d_f32: plane too large");
  plhip::PoolArgs a;
  a.x = (const float*)x; a.y = (float*)y;
  a.planes = d->planes; a.h = d->h; a.w = d->w; a.oh = d->oh; a.ow = d->ow; a.kh = d->kh; a.kw = d->kw;
  a.sh = d->stride[0]; a.sw = d->stride[1]; a.pt = d->pad[0]; a.pb = d->pad[1]; a.pl = d->pad[2]; a.pr = d->pad[3];
  a.is_max = d->is_max ? 1 : 0; a.exclusive = d->exclusive ? 1 : 0;
  if (i8) plhip::launch_pool2d_max_i8(a, ctx->stream);
  else plhip::launch_pool2d(a, ctx->stream);
  LAUNCHCHK(ctx, "pool2d");
  return PLHIP_OK;
}

plhip_status plhip_elementwise_add_f32(plhip_ctx* ctx, const float* x, const float* y, float* out, int64_t count, int relu) {
  if (!ctx || !x || !y || !out || count < 0) return fail(ctx, PLHIP_ERR_INVALID, "plhip_elementwise_add_f32: bad argument");
  if (count == 0) return PLHIP_OK;
  plhip::launch_eltwise_add(x, y, out, count, relu, ctx->stream);
  LAUNCHCHK(ctx, "elementwise_add");
  return PLHIP_OK;
}

plhip_status plhip_hard_act_f32(plhip_ctx* ctx, plhip_hard_act_kind kind, const float* params, const float* x, float* y_f32,
                                int8_t* y_i8, float calib_scale, int64_t count) {
  if (!ctx || !params || !x || (!y_f32 && !y_i8) || count < 0 || (y_i8 && !(calib_scale > 0.f)))
    return fail(ctx, PLHIP_ERR_INVALID, "plhip_hard_act_f32: bad argument");
  if (kind != PLHIP_HARD_SWISH && kind != PLHIP_HARD_SIGMOID) return fail(ctx, PLHIP_ERR_UNSUPPORTED, "plhip_hard_act_f32: unknown kind");
  if (count == 0) return PLHIP_OK;
  plhip::launch_hard_act(kind == PLHIP_HARD_SWISH ? plhip::HARD_ACT_SWISH : plhip::HARD_ACT_SIGMOID, params, x, y_f32, y_i8,
                         calib_scale, count, ctx->stream);
  LAUNCHCHK(ctx, "hard_act");
  return PLHIP_OK;
}

plhip_status plhip_se_scale_f32(plhip_ctx* ctx, const float* x, const float* gate, int n, int c, int hw, float* y_f32, int8_t* y_i8,
                                float calib_scale) {
  if (!ctx || !x || !gate || (!y_f32 && !y_i8) || n < 1 || c < 1 || hw < 1 || (y_i8 && !(calib_scale > 0.f)))
    return fail(ctx, PLHIP_ERR_INVALID, "plhip_se_scale_f32: bad argument");
  const int64_t planes = (int64_t)n * c;
  if (planes > ((int64_t)1 << 30)) return fail(ctx, PLHIP_ERR_UNSUPPORTED, "plhip_se_scale_f32: too many planes");
  plhip::launch_se_scale(x, gate, y_f32, y_i8, calib_scale, planes, hw, ctx->stream);
  LAUNCHCHK(ctx, "se_scale");
  return PLHIP_OK;
}

static bool se_gate_act_ok(int act) { return act == PLHIP_ACT_NONE || act == PLHIP_ACT_RELU || act == PLHIP_ACT_RELU6 || act == PLHIP_ACT_LEAKY_RELU; }
int plhip_se_gate_supported(int c, int cr, int act1, int act2) {
  return c >= 8 && cr >= 8 && c <= plhip::SE_GATE_MAX_C && cr <= plhip::SE_GATE_MAX_C && se_gate_act_ok(act1) && se_gate_act_ok(act2);
}
size_t plhip_se_gate_packed_weight_bytes(int c, int cr) { return c < 1 || cr < 1 ? 0 : plhip::se_gate_packed_bytes(c, cr); }
plhip_status plhip_pack_se_gate_weights(plhip_ctx* ctx, int c, int cr, const int8_t* w1, const int8_t* w2, void* w_packed) {
  if (!ctx || !w1 || !w2 || !w_packed || !aligned(w_packed, 4)) return fail(ctx, PLHIP_ERR_INVALID, "plhip_pack_se_gate_weights: bad argument");
  if (!plhip_se_gate_supported(c, cr, 0, 0)) return fail(ctx, PLHIP_ERR_UNSUPPORTED, "plhip_pack_se_gate_weights: c / cr outside 8..960");
  plhip::launch_se_gate_pack(w1, w2, w_packed, c, cr, ctx->stream);
  LAUNCHCHK(ctx, "se_gate_pack");
  return PLHIP_OK;
}
plhip_status plhip_se_gate_int8(plhip_ctx* ctx, const plhip_se_gate_desc* d, const float* pooled, const void* w_packed,
                                const float* scale1, const float* bias1, const float* scale2, const float* bias2, float* gate) {
  if (!ctx || !d || !pooled || !w_packed || !scale1 || !scale2 || !gate || d->n < 1 || !(d->calib_scale > 0.f) || !aligned(w_packed, 4))
    return fail(ctx, PLHIP_ERR_INVALID, "plhip_se_gate_int8: bad argument");
  if (!plhip_se_gate_supported(d->c, d->cr, d->act1, d->act2)) return fail(ctx, PLHIP_ERR_UNSUPPORTED, "plhip_se_gate_int8: outside the envelope");
  plhip::SeGateArgs a;
  a.pooled = pooled;
  a.inv = 1.f / d->calib_scale;  // type_trans.cc:45, as launch_calib_f32_to_i8
  a.w1 = static_cast<const uint32_t*>(w_packed);
  a.w2 = a.w1 + (size_t)((d->c + 3) / 4) * d->cr;
  a.s1 = scale1; a.b1 = bias1; a.s2 = scale2; a.b2 = bias2;
  a.act1 = d->act1; a.act2 = d->act2; a.alpha1 = d->act1_alpha; a.alpha2 = d->act2_alpha;
  a.slope = d->slope; a.offset = d->offset;
  a.gate = gate; a.c = d->c; a.cr = d->cr;
  plhip::launch_se_gate(a, d->n, ctx->stream);
  LAUNCHCHK(ctx, "se_gate");
  return PLHIP_OK;
}

// ------------------------------------------------------------------ concat / split / shuffle_channel
// every extent, outer and inner >= 1 and the whole tensor outer * sum(extents) * inner at most 2^40 elements: no product of the
// launch code (extent * inner, total * inner, row * stride) can leave int64
static bool extents_ok(const int64_t* e, int count, int64_t outer, int64_t inner, int64_t* total) {
  const int64_t cap = (int64_t)1 << 40;
  if (!e || count < 1 || outer < 1 || inner < 1 || outer > cap || inner > cap) return false;
  *total = 0;
  for (int i = 0; i < count; ++i) {
    if (e[i] < 1 || e[i] > cap) return false;
    *total += e[i];
    if (*total > cap) return false;
  }
  return *total <= cap / inner && *total * inner <= cap / outer;
}

plhip_status plhip_concat_f32(plhip_ctx* ctx, const float* const* xs, const int64_t* extents, int count, int64_t outer, int64_t inner,
                              float* y) {
  int64_t total = 0;
  if (!ctx || !xs || !y || !extents_ok(extents, count, outer, inner, &total)) return fail(ctx, PLHIP_ERR_INVALID, "plhip_concat_f32: bad argument");
  for (int i = 0; i < count; ++i)
    if (!xs[i]) return fail(ctx, PLHIP_ERR_INVALID, "plhip_concat_f32: null input");
  plhip::launch_concat_split(const_cast<float* const*>(xs), extents, count, outer, inner, y, 0, ctx->stream);
  LAUNCHCHK(ctx, "concat");
  return PLHIP_OK;
}

plhip_status plhip_concat_calib_f32(plhip_ctx* ctx, const float* const* xs, const int64_t* extents, int count, int64_t outer, int64_t inner,
                                    float* y_f32, int8_t* y_i8, float calib_scale) {
  const char* who = "plhip_concat_calib_f32";
  if (!ctx || !xs || !extents) return fail(ctx, PLHIP_ERR_INVALID, "%s: null ctx, xs or extents", who);
  if (count < 1) return fail(ctx, PLHIP_ERR_INVALID, "%s: count must be at least 1", who);
  for (int i = 0; i < count; ++i) {
    if (!xs[i]) return fail(ctx, PLHIP_ERR_INVALID, "%s: null input", who);
    if (extents[i] < 1) return fail(ctx, PLHIP_ERR_INVALID, "%s: every extent must be at least 1", who);
  }
  if (outer < 1 || inner < 1) return fail(ctx, PLHIP_ERR_INVALID, "%s: outer and inner must be at least 1", who);
  if (!y_i8) return fail(ctx, PLHIP_ERR_INVALID, "%s: y_i8 is required", who);
  if (!(calib_scale > 0.f) || !(calib_scale <= 3.402823466e38f))
    return fail(ctx, PLHIP_ERR_INVALID, "%s: calib_scale must be a positive finite number", who);
  int64_t total = 0;
  if (!extents_ok(extents, count, outer, inner, &total)) return fail(ctx, PLHIP_ERR_INVALID, "%s: more than 2^40 elements", who);
  plhip::launch_concat_calib(xs, extents, count, outer, inner, y_f32, y_i8, calib_scale, ctx->stream);
  LAUNCHCHK(ctx, "concat_calib");
  return PLHIP_OK;
}

plhip_status plhip_split_f32(plhip_ctx* ctx, const float* x, int64_t outer, int64_t extent, int64_t inner, int num, const int64_t* sections,
                             int count, float* const* ys) {
  if (!ctx || !x || !ys || count < 1 || count > (1 << 20) || extent < 1 || num < 0) return fail(ctx, PLHIP_ERR_INVALID, "plhip_split_f32: bad argument");
  if (num > 0 && (count != num || extent % num != 0)) return fail(ctx, PLHIP_ERR_INVALID, "plhip_split_f32: num must divide the axis and equal count");
  if (num == 0 && !sections) return fail(ctx, PLHIP_ERR_INVALID, "plhip_split_f32: neither num nor sections");
  std::vector<int64_t> e(count);
  for (int i = 0; i < count; ++i) e[i] = num > 0 ? extent / num : sections[i];
  int64_t total = 0;
  if (!extents_ok(e.data(), count, outer, inner, &total) || total != extent)
    return fail(ctx, PLHIP_ERR_INVALID, "plhip_split_f32: the sections do not add up to the axis");
  for (int i = 0; i < count; ++i)
    if (!ys[i]) return fail(ctx, PLHIP_ERR_INVALID, "plhip_split_f32: null output");
  plhip::launch_concat_split(ys, e.data(), count, outer, inner, const_cast<float*>(x), 1, ctx->stream);
  LAUNCHCHK(ctx, "split");
  return PLHIP_OK;
}

plhip_status plhip_shuffle_channel_f32(plhip_ctx* ctx, const float* x, int n, int c, int hw, int group, float* y_f32, int8_t* y_i8,
                                       float calib_scale) {
  if (!ctx || !x || (!y_f32 && !y_i8) || n < 1 || c < 1 || hw < 1 || group < 1 || (y_i8 && !(calib_scale > 0.f)))
    return fail(ctx, PLHIP_ERR_INVALID, "plhip_shuffle_channel_f32: bad argument");
  if (c % group != 0) return fail(ctx, PLHIP_ERR_INVALID, "plhip_shuffle_channel_f32: group must divide c");
  if ((int64_t)n * c > ((int64_t)1 << 30)) return fail(ctx, PLHIP_ERR_UNSUPPORTED, "plhip_shuffle_channel_f32: too many planes");
  plhip::launch_shuffle_channel(x, y_f32, y_i8, calib_scale, n, c, hw, group, ctx->stream);
  LAUNCHCHK(ctx, "shuffle_channel");
  return PLHIP_OK;
}

plhip_status plhip_shuffle_unit_f32(plhip_ctx* ctx, const float* a, const float* b, int n, int h, int hw, int split_at, float* lo_f32,
                                    float* hi_f32, int8_t* hi_i8, float calib_scale) {
  if (!ctx || !a || !b || n < 1 || h < 1 || hw < 1) return fail(ctx, PLHIP_ERR_INVALID, "plhip_shuffle_unit_f32: bad argument");
  if ((int64_t)n * h > ((int64_t)1 << 29)) return fail(ctx, PLHIP_ERR_UNSUPPORTED, "plhip_shuffle_unit_f32: too many planes");
  if (split_at < 0 || split_at > 2 * h) return fail(ctx, PLHIP_ERR_INVALID, "plhip_shuffle_unit_f32: split_at outside 0 .. 2 h");
  if ((split_at == 0) != (lo_f32 == nullptr)) return fail(ctx, PLHIP_ERR_INVALID, "plhip_shuffle_unit_f32: lo_f32 is null exactly when split_at is 0");
  if (split_at == 2 * h) hi_f32 = nullptr, hi_i8 = nullptr;
  else if (!hi_f32 && !hi_i8) return fail(ctx, PLHIP_ERR_INVALID, "plhip_shuffle_unit_f32: no output for the channels from split_at on");
  if (hi_i8 && !(calib_scale > 0.f)) return fail(ctx, PLHIP_ERR_INVALID, "plhip_shuffle_unit_f32: int8 output needs a positive calib scale");
  plhip::launch_shuffle_unit(a, b, lo_f32, hi_f32, hi_i8, calib_scale, n, h, hw, split_at, ctx->stream);
  LAUNCHCHK(ctx, "shuffle_unit");
  return PLHIP_OK;
}

// ------------------------------------------------------------------ bilinear_interp / nearest_interp / arg_max
// the checks the three entry points share, in one order; planes_in / planes_out: how many planes of in_h x in_w are read and of
// out_h x out_w written (arg_max over c channels writes one plane per image)
static plhip_status interp_check(plhip_ctx* ctx, const char* who, const void* x, int64_t planes_in, int64_t planes_out, int in_h, int in_w,
                                 int out_h, int out_w, int method, int align_corners, int align_mode) {
  const int cap = 1 << 15;
  if (!ctx || !x) return fail(ctx, PLHIP_ERR_INVALID, "%s: null ctx or x", who);
  if (planes_in < 1 || planes_out < 1 || in_h < 1 || in_w < 1 || out_h < 1 || out_w < 1)
    return fail(ctx, PLHIP_ERR_INVALID, "%s: every dimension must be at least 1", who);
  if (in_h > cap || in_w > cap || out_h > cap || out_w > cap) return fail(ctx, PLHIP_ERR_UNSUPPORTED, "%s: a dimension above 2^15", who);
  if (method != PLHIP_INTERP_BILINEAR && method != PLHIP_INTERP_NEAREST) return fail(ctx, PLHIP_ERR_UNSUPPORTED, "%s: unknown method", who);
  if ((align_corners != 0 && align_corners != 1) || (align_mode != 0 && align_mode != 1))
    return fail(ctx, PLHIP_ERR_UNSUPPORTED, "%s: unknown align_corners or align_mode", who);
  const int64_t most = (int64_t)1 << 40;
  if (planes_in > most / ((int64_t)in_h * in_w) || planes_out > most / ((int64_t)out_h * out_w))
    return fail(ctx, PLHIP_ERR_UNSUPPORTED, "%s: more than 2^40 elements", who);
  return PLHIP_OK;
}

// dtype of an arg_max output (ArgmaxParam::dtype): -1 and 3 int64, 2 int32; -1: neither
static int label_is_i64(int dtype) { return dtype == -1 || dtype == 3 ? 1 : dtype == 2 ? 0 : -1; }

plhip_status plhip_interp_f32(plhip_ctx* ctx, const float* x, int64_t planes, int in_h, int in_w, int out_h, int out_w, int method,
                              int align_corners, int align_mode, float* y_f32, int8_t* y_i8, float calib_scale) {
  const char* who = "plhip_interp_f32";
  if (plhip_status st = interp_check(ctx, who, x, planes, planes, in_h, in_w, out_h, out_w, method, align_corners, align_mode)) return st;
  if (!y_f32 && !y_i8) return fail(ctx, PLHIP_ERR_INVALID, "%s: null y_f32 and y_i8, one output is required", who);
  if (y_i8 && (!(calib_scale > 0.f) || !(calib_scale <= 3.402823466e38f)))
    return fail(ctx, PLHIP_ERR_INVALID, "%s: calib_scale must be a positive finite number", who);
  plhip::launch_interp(plhip::interp_args(x, in_h, in_w, out_h, out_w, method, align_corners, align_mode), planes, y_f32, y_i8,
                       calib_scale, ctx->stream);
  LAUNCHCHK(ctx, "interp");
  return PLHIP_OK;
}

plhip_status plhip_arg_max_f32(plhip_ctx* ctx, const float* x, int64_t outer, int c, int64_t inner, void* y, int dtype) {
  const char* who = "plhip_arg_max_f32";
  if (!ctx || !x || !y) return fail(ctx, PLHIP_ERR_INVALID, "%s: null ctx, x or y", who);
  if (outer < 1 || c < 1 || inner < 1) return fail(ctx, PLHIP_ERR_INVALID, "%s: every dimension must be at least 1", who);
  if (c > (1 << 15)) return fail(ctx, PLHIP_ERR_UNSUPPORTED, "%s: a dimension above 2^15 (the axis)", who);
  const int i64 = label_is_i64(dtype);
  if (i64 < 0) return fail(ctx, PLHIP_ERR_UNSUPPORTED, "%s: dtype must be -1 or 3 (int64) or 2 (int32)", who);
  const int64_t most = (int64_t)1 << 40;
  if (outer > most || inner > most || inner > most / c || outer > most / (inner * c))
    return fail(ctx, PLHIP_ERR_UNSUPPORTED, "%s: more than 2^40 elements", who);
  plhip::launch_arg_max(x, outer, c, inner, y, i64, ctx->stream);
  LAUNCHCHK(ctx, "arg_max");
  return PLHIP_OK;
}

plhip_status plhip_interp_argmax_f32(plhip_ctx* ctx, const float* x, int n, int c, int in_h, int in_w, int out_h, int out_w, int method,
                                     int align_corners, int align_mode, void* y, int dtype) {
  const char* who = "plhip_interp_argmax_f32";
  if (n < 1 || c < 1) return fail(ctx, PLHIP_ERR_INVALID, "%s: every dimension must be at least 1", who);
  if (c > (1 << 15)) return fail(ctx, PLHIP_ERR_UNSUPPORTED, "%s: a dimension above 2^15", who);
  if (plhip_status st = interp_check(ctx, who, x, (int64_t)n * c, n, in_h, in_w, out_h, out_w, method, align_corners, align_mode)) return st;
  if (!y) return fail(ctx, PLHIP_ERR_INVALID, "%s: null y", who);
  const int i64 = label_is_i64(dtype);
  if (i64 < 0) return fail(ctx, PLHIP_ERR_UNSUPPORTED, "%s: dtype must be -1 or 3 (int64) or 2 (int32)", who);
  if ((int64_t)n * c > ((int64_t)1 << 40) / ((int64_t)out_h * out_w)) return fail(ctx, PLHIP_ERR_UNSUPPORTED, "%s: more than 2^40 elements", who);
  plhip::launch_interp_argmax(plhip::interp_args(x, in_h, in_w, out_h, out_w, method, align_corners, align_mode), n, c, y, i64, ctx->stream);
  LAUNCHCHK(ctx, "interp_argmax");
  return PLHIP_OK;
}

// ------------------------------------------------------------------ transpose / concat_nhwc / box_coder / multiclass_nms
plhip_status plhip_transpose_f32(plhip_ctx* ctx, const float* x, const int64_t* dims, const int* perm, int rank, float* y) {
  const char* who = "plhip_transpose_f32";
  if (!ctx || !x || !y) return fail(ctx, PLHIP_ERR_INVALID, "%s: null ctx, x or y", who);
  if (!dims || !perm) return fail(ctx, PLHIP_ERR_INVALID, "%s: null dims or perm", who);
  if (rank < 2 || rank > 4) return fail(ctx, PLHIP_ERR_UNSUPPORTED, "%s: rank must be 2, 3 or 4", who);
  const int64_t most = (int64_t)1 << 40;
  int64_t total = 1;
  unsigned seen = 0;
  for (int k = 0; k < rank; ++k) {
    if (dims[k] < 1) return fail(ctx, PLHIP_ERR_INVALID, "%s: every dimension must be at least 1", who);
    if (dims[k] > most / total) return fail(ctx, PLHIP_ERR_UNSUPPORTED, "%s: more than 2^40 elements", who);
    total *= dims[k];
    if (perm[k] < 0 || perm[k] >= rank || (seen & (1u << perm[k]))) return fail(ctx, PLHIP_ERR_INVALID, "%s: perm is not a permutation of the axes", who);
    seen |= 1u << perm[k];
  }
  plhip::launch_transpose(x, dims, perm, rank, y, ctx->stream);
  LAUNCHCHK(ctx, "transpose");
  return PLHIP_OK;
}

plhip_status plhip_concat_nhwc_f32(plhip_ctx* ctx, const float* const* xs, const int64_t* channels, const int64_t* hw, int count,
                                   int64_t n, float* y) {
  const char* who = "plhip_concat_nhwc_f32";
  if (!ctx || !xs || !channels || !hw || !y) return fail(ctx, PLHIP_ERR_INVALID, "%s: null ctx, xs, channels, hw or y", who);
  if (count < 1) return fail(ctx, PLHIP_ERR_INVALID, "%s: count must be at least 1", who);
  if (n < 1) return fail(ctx, PLHIP_ERR_INVALID, "%s: n must be at least 1", who);
  const int64_t most = (int64_t)1 << 40;
  int64_t total = 0;
  for (int i = 0; i < count; ++i) {
    if (!xs[i]) return fail(ctx, PLHIP_ERR_INVALID, "%s: null input", who);
    if (channels[i] < 1 || hw[i] < 1) return fail(ctx, PLHIP_ERR_INVALID, "%s: every extent must be at least 1", who);
    if (channels[i] > most / hw[i] || channels[i] * hw[i] > most - total) return fail(ctx, PLHIP_ERR_UNSUPPORTED, "%s: more than 2^40 elements", who);
    total += channels[i] * hw[i];
  }
  if (n > most / total) return fail(ctx, PLHIP_ERR_UNSUPPORTED, "%s: more than 2^40 elements", who);
  plhip::launch_concat_nhwc(xs, channels, hw, count, n, y, ctx->stream);
  LAUNCHCHK(ctx, "concat_nhwc");
  return PLHIP_OK;
}

plhip_status plhip_box_coder_decode_f32(plhip_ctx* ctx, const float* prior, const float* prior_var_or_null,
                                        const float* variance4_or_null, const float* target, int64_t rows, int64_t cols, int axis,
                                        int normalized, float* y) {
  const char* who = "plhip_box_coder_decode_f32";
  if (!ctx || !prior || !target || !y) return fail(ctx, PLHIP_ERR_INVALID, "%s: null ctx, prior, target or y", who);
  if (rows < 1 || cols < 1) return fail(ctx, PLHIP_ERR_INVALID, "%s: rows and cols must be at least 1", who);
  if (axis != 0 && axis != 1) return fail(ctx, PLHIP_ERR_INVALID, "%s: axis must be 0 or 1", who);
  if (rows > ((int64_t)1 << 38) / cols) return fail(ctx, PLHIP_ERR_UNSUPPORTED, "%s: more than 2^40 elements", who);
  plhip::BoxCoderArgs a;
  a.prior = prior; a.pvar = prior_var_or_null; a.target = target; a.y = y;
  a.var = prior_var_or_null ? 2 : variance4_or_null ? 1 : 0;
  for (int k = 0; k < 4; ++k) a.variance[k] = a.var == 1 ? variance4_or_null[k] : 1.f;
  a.rows = rows; a.cols = cols; a.axis = axis; a.normalized = normalized ? 1 : 0;
  plhip::launch_box_coder_decode(a, ctx->stream);
  LAUNCHCHK(ctx, "box_coder_decode");
  return PLHIP_OK;
}

// the descriptor's checks, shared by the workspace query (ctx == nullptr: the text goes to the calling thread's slot)
static plhip_status nms_check(plhip_ctx* ctx, const char* who, const plhip_nms_desc* d, int* kmax, int* cap, int* nact) {
  if (!d) return fail(ctx, PLHIP_ERR_INVALID, "%s: null desc", who);
  if (d->n < 1 || d->c < 1 || d->p < 1) return fail(ctx, PLHIP_ERR_INVALID, "%s: n, c and p must be at least 1", who);
  if (d->keep_top_k <= 0) return fail(ctx, PLHIP_ERR_INVALID, "%s: keep_top_k must be positive (it sizes the output)", who);
  if (!(d->nms_eta >= 1.f)) return fail(ctx, PLHIP_ERR_UNSUPPORTED, "%s: nms_eta < 1 (adaptive threshold) is outside the device kernel", who);
  if (d->p > 16384) return fail(ctx, PLHIP_ERR_UNSUPPORTED, "%s: more than 16384 priors", who);
  if (d->score_stride_class < 0 || d->score_stride_prior < 0 ||
      (int64_t)(d->c - 1) * d->score_stride_class + (int64_t)(d->p - 1) * d->score_stride_prior > (int64_t)d->c * d->p - 1)
    return fail(ctx, PLHIP_ERR_INVALID, "%s: the score strides leave the image's c * p scores", who);
  plhip::nms_sizes(d->c, d->p, d->background_label, d->nms_top_k, d->keep_top_k, kmax, cap, nact);
  if (*kmax > 4096) return fail(ctx, PLHIP_ERR_UNSUPPORTED, "%s: min(nms_top_k, p) above 4096", who);
  if ((int64_t)*nact * *cap > 16384)
    return fail(ctx, PLHIP_ERR_UNSUPPORTED, "%s: (classes other than the background) * min(nms_top_k, keep_top_k, p) above 16384", who);
  if (d->n > 65535 || (int64_t)d->n * d->p >= ((int64_t)1 << 31)) return fail(ctx, PLHIP_ERR_UNSUPPORTED, "%s: n above 65535 or n * p above 2^31", who);
  return PLHIP_OK;
}

size_t plhip_multiclass_nms_workspace_bytes(const plhip_nms_desc* desc) {
  int kmax, cap, nact;
  if (nms_check(nullptr, "plhip_multiclass_nms_workspace_bytes", desc, &kmax, &cap, &nact)) return 0;
  const size_t slots = (size_t)desc->n * desc->c;
  return slots * cap * 8 + slots * 4 + 16;
}

plhip_status plhip_multiclass_nms_f32(plhip_ctx* ctx, const float* boxes, const float* scores, const plhip_nms_desc* desc,
                                      void* workspace, float* out, int* index_or_null, int* count) {
  const char* who = "plhip_multiclass_nms_f32";
  if (!ctx || !boxes || !scores) return fail(ctx, PLHIP_ERR_INVALID, "%s: null ctx, boxes or scores", who);
  int kmax, cap, nact;
  if (plhip_status st = nms_check(ctx, who, desc, &kmax, &cap, &nact)) return st;
  if (!workspace || !aligned(workspace, 8)) return fail(ctx, PLHIP_ERR_INVALID, "%s: workspace is null or not 8-byte aligned", who);
  if (!out || !count) return fail(ctx, PLHIP_ERR_INVALID, "%s: null out or count", who);
  plhip::NmsArgs a;
  a.boxes = boxes; a.scores = scores; a.out = out; a.index = index_or_null; a.count = count;
  a.ws_list = (uint64_t*)workspace;
  a.ws_len = (int*)((char*)workspace + (size_t)desc->n * desc->c * cap * 8);
  a.C = desc->c; a.P = desc->p; a.ssc = desc->score_stride_class; a.ssp = desc->score_stride_prior;
  a.bg = desc->background_label; a.sthr = desc->score_threshold; a.nthr = desc->nms_threshold;
  a.keep = desc->keep_top_k; a.normalized = desc->normalized ? 1 : 0;
  a.kmax = kmax; a.cap = cap; a.nact = nact;
  plhip::launch_multiclass_nms(a, desc->n, ctx->stream);
  LAUNCHCHK(ctx, "multiclass_nms");
  return PLHIP_OK;
}

// ------------------------------------------------------------------ yolo_box / yolo_head
// one scale's checks and its YoloScale; *cells grows by an * h * w
static plhip_status yolo_scale(plhip_ctx* ctx, const char* who, const float* x, int h, int w, const int* anchors, int anchor_len,
                               int ratio, plhip::YoloScale* s, int64_t* cells) {
  if (!x) return fail(ctx, PLHIP_ERR_INVALID, "%s: null x", who);
  if (h < 1 || w < 1) return fail(ctx, PLHIP_ERR_INVALID, "%s: h and w must be at least 1", who);
  if (!anchors) return fail(ctx, PLHIP_ERR_INVALID, "%s: null anchors", who);
  if (anchor_len < 2 || (anchor_len & 1)) return fail(ctx, PLHIP_ERR_INVALID, "%s: the anchor list must hold at least one (width, height) pair and no odd value", who);
  if (ratio < 1) return fail(ctx, PLHIP_ERR_INVALID, "%s: downsample_ratio must be at least 1", who);
  if (anchor_len > 2 * plhip::YOLO_MAX_ANCHORS) return fail(ctx, PLHIP_ERR_UNSUPPORTED, "%s: more than 16 anchors in one scale", who);
  const int64_t top = (int64_t)1 << 31;
  if ((int64_t)h * w >= top / (anchor_len / 2)) return fail(ctx, PLHIP_ERR_UNSUPPORTED, "%s: n * P * max(c, 4) reaches 2^31", who);
  if ((int64_t)ratio * h >= top) return fail(ctx, PLHIP_ERR_UNSUPPORTED, "%s: downsample_ratio * h reaches 2^31", who);
  s->x = x; s->h = h; s->w = w; s->an = anchor_len / 2; s->ratio = ratio;
  for (int k = 0; k < 2 * plhip::YOLO_MAX_ANCHORS; ++k) s->anchors[k] = k < anchor_len ? anchors[k] : 0;
  s->p_off = s->chunks = s->vec = 0;
  *cells += (int64_t)s->an * h * w;
  return PLHIP_OK;
}

// what the scales share; P: the priors of one image
static plhip_status yolo_common(plhip_ctx* ctx, const char* who, const int* img_size, int n, int c, int64_t P, float conf_thresh,
                                int clip_bbox, float scale_x_y, const float* boxes, const float* scores, plhip::YoloCommon* o) {
  if (!img_size) return fail(ctx, PLHIP_ERR_INVALID, "%s: null img_size", who);
  if (!boxes || !scores) return fail(ctx, PLHIP_ERR_INVALID, "%s: null boxes or scores", who);
  const int64_t top = (int64_t)1 << 31, widest = c > 4 ? c : 4;
  if (P >= top || (int64_t)n * P >= top || (int64_t)n * P >= (top + widest - 1) / widest)
    return fail(ctx, PLHIP_ERR_UNSUPPORTED, "%s: n * P * max(c, 4) reaches 2^31", who);
  o->img_size = img_size; o->n = n; o->classes = c; o->clip = clip_bbox ? 1 : 0;
  o->thresh = conf_thresh; o->scale = scale_x_y;
  o->bias = (float)(-0.5 * ((double)scale_x_y - 1.));  // yolo_box_compute.cc:37: in double, then narrowed
  return PLHIP_OK;
}

plhip_status plhip_yolo_box_f32(plhip_ctx* ctx, const float* x, const int* img_size, int n, int an, int c, int h, int w,
                                const int* anchors, float conf_thresh, int downsample_ratio, int clip_bbox, float scale_x_y,
                                float* boxes, float* scores) {
  const char* who = "plhip_yolo_box_f32";
  if (!ctx) return fail(ctx, PLHIP_ERR_INVALID, "%s: null ctx", who);
  if (n < 1 || c < 1) return fail(ctx, PLHIP_ERR_INVALID, "%s: n and c must be at least 1", who);
  if (an < 1) return fail(ctx, PLHIP_ERR_INVALID, "%s: an must be at least 1 (an empty anchor list)", who);
  plhip::YoloBoxArgs a;
  int64_t P = 0;
  if (plhip_status st = yolo_scale(ctx, who, x, h, w, anchors, an > (1 << 20) ? (1 << 20) : 2 * an, downsample_ratio, &a.s, &P)) return st;
  if (plhip_status st = yolo_common(ctx, who, img_size, n, c, P, conf_thresh, clip_bbox, scale_x_y, boxes, scores, &a.c)) return st;
  a.boxes = boxes; a.scores = scores;
  plhip::launch_yolo_box(a, ctx->stream);
  LAUNCHCHK(ctx, "yolo_box");
  return PLHIP_OK;
}

plhip_status plhip_yolo_head_f32(plhip_ctx* ctx, const float* const* xs, const int* hs, const int* ws, const int* const* anchors,
                                 const int* anchor_lens, const int* downsample_ratios, int count, const int* img_size, int n, int c,
                                 float conf_thresh, int clip_bbox, float scale_x_y, float* boxes, float* scores) {
  const char* who = "plhip_yolo_head_f32";
  if (!ctx) return fail(ctx, PLHIP_ERR_INVALID, "%s: null ctx", who);
  if (!xs || !hs || !ws || !anchors || !anchor_lens || !downsample_ratios)
    return fail(ctx, PLHIP_ERR_INVALID, "%s: null xs, hs, ws, anchors, anchor_lens or downsample_ratios", who);
  if (count < 1 || count > plhip::YOLO_MAX_SCALES) return fail(ctx, PLHIP_ERR_INVALID, "%s: count must be 1 .. 8", who);
  if (n < 1 || c < 1) return fail(ctx, PLHIP_ERR_INVALID, "%s: n and c must be at least 1", who);
  if (c > (1 << 18)) return fail(ctx, PLHIP_ERR_UNSUPPORTED, "%s: c above 2^18", who);
  plhip::YoloHeadArgs a;
  memset(&a, 0, sizeof(a));
  int64_t P = 0;
  for (int i = 0; i < count; ++i) {
    if (plhip_status st = yolo_scale(ctx, who, xs[i], hs[i], ws[i], anchors[i], anchor_lens[i], downsample_ratios[i], &a.s[i], &P)) return st;
    if (P >= ((int64_t)1 << 31)) return fail(ctx, PLHIP_ERR_UNSUPPORTED, "%s: n * P * max(c, 4) reaches 2^31", who);
  }
  if (plhip_status st = yolo_common(ctx, who, img_size, n, c, P, conf_thresh, clip_bbox, scale_x_y, boxes, scores, &a.c)) return st;
  a.boxes = boxes; a.scores = scores; a.count = count;
  plhip::launch_yolo_head(a, ctx->stream);
  LAUNCHCHK(ctx, "yolo_head");
  return PLHIP_OK;
}

}  // extern "C"
