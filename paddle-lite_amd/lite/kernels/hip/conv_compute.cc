// conv_compute.cc — TARGET(kHIP) / PRECISION(kInt8) conv2d + depthwise_conv2d kernels.
//
// Mirrors lite/kernels/arm/conv_compute.cc:87-185 (impl selection), conv_gemmlike.cc:85-264 and
// conv_depthwise.cc:138-296 (shape-change re-init, weight pre-pack, scale / bias / relu6 folding) and the six
// registrations of conv_compute.cc:216-252.  Differences by design: 3x3s1 goes through the
// direct accumulator (im2col GEMM), not the integer Winograd transform, and 3x3s2 needs no special DirectConv.
#include "lite/kernels/hip/conv_compute.h"
#include "lite/kernels/hip/packed_weight_cache.h"
#include "lite/kernels/hip/quant_fold.h"

#include "lite/core/op_registry.h"

namespace paddle {
namespace lite {
namespace kernels {
namespace hip {

namespace {
// scale / bias / activation of one conv folded (quant_fold.h) into its descriptor and device tensors
void Fold(FoldedConv* c, const std::vector<float>& weight_scale, float in_scale, float out_scale, bool int8_out, const Tensor* bias,
          const operators::ActivationParam& act, bool fuse_relu) {
  const QuantFold f = FoldLayer(weight_scale, c->desc.cout, in_scale, out_scale, int8_out, bias, &act, fuse_relu);
  c->desc.act = f.act;
  c->desc.act_alpha = f.alpha;
  c->has_bias = UploadFold(f, &c->scale, &c->bias);
}

// Weights: pre-packed for the implementation the descriptor selects (trans_gemm_weights<kInt8> -> prepackA_int8 analogue), or
// kept OIHW for the depthwise path.  layout: the key predictors share the copy under (packed_weight_cache.h), "" = private.
// what: the conv's name in the refusal.  Returns the packed byte count.
size_t Pack(HIPContext* ctx, FoldedConv* c, const Tensor* filter, bool keep_oihw, const std::string& layout, const char* what) {
  const size_t w_bytes = static_cast<size_t>(filter->numel());
  const size_t packed = keep_oihw ? w_bytes : plhip_conv_packed_weight_bytes(&c->desc);
  CHECK_GT(packed, 0UL) << "invalid " << what << " configuration";
  c->weights = PackThroughCache(ctx, filter, layout, packed, [&](const int8_t* w_dev, void* d) {
    if (keep_oihw) {
      ctx->MemcpySync(d, w_dev, w_bytes, IoDirection::DtoD);
    } else {
      HIP_CALL(ctx->ctx(), plhip_pack_conv_weights(ctx->ctx(), &c->desc, w_dev, d));
    }
  });
  return packed;
}
}  // namespace

template <PrecisionType Ptype, PrecisionType OutType>
void ConvCompute<Ptype, OutType>::BuildDesc() {
  auto& param = this->template Param<param_t>();
  auto& d = conv_.desc;
  const auto x = param.x->dims(), w = param.filter->dims();
  CHECK_EQ(x.size(), 4UL);
  CHECK(param.paddings && param.paddings->size() == 4UL) << "paddings must be {top, bottom, left, right}";
  CHECK(param.dilations && param.dilations->size() == 2UL);
  d.n = static_cast<int>(x[0]);
  d.cin = static_cast<int>(x[1]);
  d.h = static_cast<int>(x[2]);
  d.w = static_cast<int>(x[3]);
  d.cout = static_cast<int>(w[0]);
  d.kh = static_cast<int>(w[2]);
  d.kw = static_cast<int>(w[3]);
  for (int i = 0; i < 4; ++i) d.pad[i] = (*param.paddings)[i];
  d.stride[0] = param.strides[0];
  d.stride[1] = param.strides[1];
  d.dil[0] = (*param.dilations)[0];
  d.dil[1] = (*param.dilations)[1];
  d.groups = param.groups;
}

// Packed once per IMPLEMENTATION.  The implementation plhip's conv_geom picks — and with it the packed layout — depends on the
// input shape (the patch kernels need a row pitch of 8..64, the 7x7 stem OW % 4 == 0 ...): ReInitWhenNeeded calls this again when
// a resized feed changes it.  One packed device copy per process and device (packed_weight_cache.h): predictors that run the
// same model — the three in flight of bench.py, a serving process with a predictor per thread (cxx_api.h:103-137) — share it.
template <PrecisionType Ptype, PrecisionType OutType>
void ConvCompute<Ptype, OutType>::PackWeights() {
  auto& param = this->template Param<param_t>();
  const auto& d = conv_.desc;
  packed_impl_ = is_depthwise_ ? std::string("dw_oihw") : std::string(plhip_conv_impl_name(&d));
  std::string layout = packed_impl_;
  const auto wd = param.filter->dims();
  for (size_t i = 0; i < wd.size(); ++i) layout += "_" + std::to_string(wd[i]);
  layout += "_g" + std::to_string(d.groups) + "_w" + std::to_string(d.w) + "_p" + std::to_string(d.pad[2]) + "_" + std::to_string(d.pad[3]);
  packed_bytes_ = Pack(&this->ctx_->template As<HIPContext>(), &conv_, param.filter, is_depthwise_, layout, "conv");
}

// What Run launches for the shape in conv_.desc.  The fused forms are asked for first; a shape outside them falls back inside
// the kernel object: the front into xq_ and then the plain conv, the depthwise pair as separate launches through mid_.
template <PrecisionType Ptype, PrecisionType OutType>
typename ConvCompute<Ptype, OutType>::Route ConvCompute<Ptype, OutType>::ResolveRoute() {
  auto& param = this->template Param<param_t>();
  const auto& d = conv_.desc;
  const bool has_tail = param.fuse_residual_connection || fusion_.calib_output != nullptr;
  CHECK(!fusion_.image_input || fusion_.calib_input_scale > 0.f) << "kHIP: an image source needs the calib scale of the int8 stem";
  CHECK(!fusion_.drop_fp32_output || fusion_.calib_output) << "kHIP: only a fused calib copy leaves the fp32 output without consumers";
  if (fusion_.calib_input_scale > 0.f) {
    CHECK(!is_depthwise_ && !fusion_.pw_filter && !has_tail) << "kHIP: a conv that took the calib in front of it over has no other fusion";
    if (fusion_.image_input) {  // fusion H1: the uint8 image is the source, image_to_tensor + calib fold in
      image_desc_ = plhip_image_desc{};
      image_desc_.n = d.n; image_desc_.h = d.h; image_desc_.w = d.w;
      image_desc_.format = fusion_.image_format;
      for (int i = 0; i < 3; ++i) {
        image_desc_.means[i] = fusion_.image_means[i];
        image_desc_.scales[i] = fusion_.image_scales[i];
      }
      if (plhip_conv2d_image_supported(&d, &image_desc_)) return Route::kImageStem;
    } else if (plhip_conv2d_calib_supported(&d)) {
      return Route::kCalibStem;
    }
    return Route::kConv;
  }
  if (OutType == PRECISION(kFloat) && has_tail) {
    CHECK(!is_depthwise_) << "kHIP: the fused conv tail exists on the GEMM-like convs only";
    return Route::kConvTail;
  }
  if (!fusion_.pw_filter) return is_depthwise_ ? Route::kDepthwise : Route::kConv;
  // the pointwise conv sees the depthwise conv's output plane (`output` may be the pooled one: from the descriptor)
  pw_.desc.n = d.n;
  pw_.desc.h = (d.h + d.pad[0] + d.pad[1] - (d.dil[0] * (d.kh - 1) + 1)) / d.stride[0] + 1;
  pw_.desc.w = (d.w + d.pad[2] + d.pad[3] - (d.dil[1] * (d.kw - 1) + 1)) / d.stride[1] + 1;
  const plhip_out_kind kind = fusion_.pw_int8_out ? PLHIP_OUT_I8 : PLHIP_OUT_F32;
  if (fusion_.pw_tail)  // fusion G: the 1x1 conv keeps its graph tail
    return plhip_dw_conv1x1_fused_supported(&d, pw_.desc.cout, kind, has_tail) ? Route::kDwConv1x1Fused : Route::kDwConv1x1Split;
  return plhip_dwpw_fused_supported(&d, pw_.desc.cout, fusion_.pw_global_avg_pool ? PLHIP_OUT_F32_GAP : kind) ? Route::kDwPwFused
                                                                                                            : Route::kDwPwSplit;
}

// The profile name of route_: the device function(s) Run dispatches to, for the shape in conv_.desc.
template <PrecisionType Ptype, PrecisionType OutType>
std::string ConvCompute<Ptype, OutType>::KernelFuncName() const {
  const auto& d = conv_.desc;
  const std::string gap = fusion_.pw_global_avg_pool ? "+pooling_global_avg" : "";
  switch (route_) {
    case Route::kImageStem: return std::string("image_to_tensor_int8+") + plhip_conv_impl_name(&d);
    case Route::kCalibStem: return std::string("calib_fp32_to_int8+") + plhip_conv_impl_name(&d);
    case Route::kDwConv1x1Fused: return "conv_depthwise_3x3_conv1x1_fused_int8_hip" + gap;
    case Route::kDwConv1x1Split: return "conv_depthwise_int8_hip+conv1x1_tail_gemm_int8_hip" + gap;
    case Route::kDwPwFused: return "conv_depthwise_3x3_pointwise_1x1_fused_int8_hip" + gap;
    case Route::kDwPwSplit: return "conv_depthwise_int8_hip+conv1x1s1_gemm_int8_mfma32x32x32" + gap;
    case Route::kDepthwise:
      return "conv_depthwise_" + std::to_string(d.kh) + "x" + std::to_string(d.kw) +
             (OutType == PRECISION(kInt8) ? "_int8_int8_hip" : "_int8_fp32_hip");
    case Route::kConvTail:
    case Route::kConv: break;
  }
  // (an image the stem cannot read: its own launch in front)
  return std::string(fusion_.image_input ? "image_to_tensor_int8_hip+" : "") + plhip_conv_impl_name(&d);
}

template <PrecisionType Ptype, PrecisionType OutType>
void ConvCompute<Ptype, OutType>::ReInitWhenNeeded() {
  auto& param = this->template Param<param_t>();
  if (last_shape_ == param.x->dims()) return;  // conv_gemmlike.cc:92 idiom
  BuildDesc();
  // a resized feed may cross an implementation boundary (3x3 64 -> 64 from W = 56 to W = 112: patch kernel -> implicit GEMM;
  // the ResNet stem from 224 to 226): the packed bytes belong to ONE implementation, so pack again for the new one
  // (through the shared cache: a layout seen before is reused) instead of running it on the old layout
  if (!is_depthwise_ && packed_bytes_ != 0 &&
      (packed_impl_ != plhip_conv_impl_name(&conv_.desc) || packed_bytes_ != plhip_conv_packed_weight_bytes(&conv_.desc))) {
    PackWeights();
  }
  workspace_bytes_ = is_depthwise_ ? 0 : plhip_conv_workspace_bytes(&conv_.desc);
  route_ = ResolveRoute();
  kernel_func_name_ = KernelFuncName();
  last_shape_ = param.x->dims();
}

// The 1x1 consumer taken over by a depthwise conv (graph_builder.cc, fusion D): folded and packed exactly as a stand-alone
// conv2d, with the depthwise output scale as its input scale; its weights stay private to this kernel object.
template <PrecisionType Ptype, PrecisionType OutType>
void ConvCompute<Ptype, OutType>::PreparePointwise() {
  auto& param = this->template Param<param_t>();
  CHECK(is_depthwise_ && OutType == PRECISION(kInt8)) << "kHIP: only a depthwise conv with int8 output takes a 1x1 consumer over";
  const auto wd = fusion_.pw_filter->dims();
  CHECK(wd.size() == 4UL && wd[2] == 1 && wd[3] == 1 && wd[1] == conv_.desc.cout) << "fused consumer must be a 1x1 conv over the depthwise channels";
  auto& d = pw_.desc;
  d = plhip_conv_desc{};
  d.n = conv_.desc.n; d.cin = conv_.desc.cout; d.h = 1; d.w = 1; d.cout = static_cast<int>(wd[0]);
  d.kh = d.kw = 1;
  d.stride[0] = d.stride[1] = 1;
  d.dil[0] = d.dil[1] = 1;
  d.groups = 1;
  Fold(&pw_, fusion_.pw_weight_scale, param.output_scale, fusion_.pw_output_scale, fusion_.pw_int8_out, fusion_.pw_bias,
       fusion_.pw_activation_param, false);
  Pack(&this->ctx_->template As<HIPContext>(), &pw_, fusion_.pw_filter, false, "", "fused pointwise");
}

template <PrecisionType Ptype, PrecisionType OutType>
void ConvCompute<Ptype, OutType>::PrepareForRun() {
  auto& param = this->template Param<param_t>();
  CHECK(this->ctx_) << "SetContext must precede PrepareForRun";
  const auto w_dims = param.filter->dims();
  const int oc = static_cast<int>(w_dims[0]);
  const int ic = static_cast<int>(w_dims[1]) * param.groups;
  BuildDesc();
  // impl selection (conv_compute.cc:87-134): depthwise iff groups == ic == oc; everything else is GEMM-like
  is_depthwise_ = param.groups == ic && ic == oc && param.groups > 1;
  // activation_param, fuse_relu the legacy flag (conv_gemmlike.cc:325-345); scales and bias: conv_gemmlike.cc:208-263
  Fold(&conv_, param.weight_scale, param.input_scale, param.output_scale, OutType == PRECISION(kInt8), param.bias, param.activation_param,
       param.fuse_relu);
  PackWeights();
  if (fusion_.pw_filter) PreparePointwise();
  last_shape_ = DDim();
  ReInitWhenNeeded();
}

// The conv's int8 input: `x`, or what the calib / image_to_tensor this conv took over makes of its source (fusions F / H1 on a
// shape without the one-launch form), in a private tensor.
template <PrecisionType Ptype, PrecisionType OutType>
const int8_t* ConvCompute<Ptype, OutType>::Int8Input() {
  auto& param = this->template Param<param_t>();
  auto& ctx = this->ctx_->template As<HIPContext>();
  if (!(fusion_.calib_input_scale > 0.f)) return param.x->template data<int8_t>();
  xq_.Resize(param.x->dims());
  int8_t* q = xq_.mutable_data<int8_t>(TARGET(kHIP));
  if (fusion_.image_input) {
    HIP_CALL(ctx.ctx(), plhip_image_to_tensor_i8(ctx.ctx(), &image_desc_, static_cast<const uint8_t*>(fusion_.image_input->raw_data()), q,
                                                 fusion_.calib_input_scale));
  } else {
    HIP_CALL(ctx.ctx(), plhip_calib_f32_to_i8(ctx.ctx(), param.x->template data<float>(), q, fusion_.calib_input_scale,
                                              static_cast<int64_t>(param.x->dims().production())));
  }
  return q;
}

// `output` allocated in the precision the route writes; drop: a fused tail left the fp32 tensor without consumers
// (drop_fp32_output), it is never allocated
template <PrecisionType Ptype, PrecisionType OutType>
void* ConvCompute<Ptype, OutType>::Output(bool int8, bool drop) {
  auto& param = this->template Param<param_t>();
  if (drop) return nullptr;
  return int8 ? static_cast<void*>(param.output->template mutable_data<int8_t>(TARGET(kHIP)))
              : static_cast<void*>(param.output->template mutable_data<float>(TARGET(kHIP)));
}

// f32: the output the tail hangs on is fp32 (always, for a conv's own tail; the 1x1 conv's precision under fusion G)
template <PrecisionType Ptype, PrecisionType OutType>
typename ConvCompute<Ptype, OutType>::Tail ConvCompute<Ptype, OutType>::GatherTail(bool f32) {
  auto& param = this->template Param<param_t>();
  Tail t;
  if (param.fuse_residual_connection) {
    CHECK(f32 && param.residualData && param.residualData->target() == TARGET(kHIP)) << "fused residual operand must live on the device";
    CHECK(param.residualData->dims() == param.output->dims()) << "fused residual operand must have the output's shape";
    t.residual = param.residualData->template data<float>();
  }
  if (fusion_.calib_output) {
    CHECK(f32) << "the fused calib reads the 1x1 conv's fp32 output";
    fusion_.calib_output->Resize(param.output->dims());
    t.calib_out = fusion_.calib_output->template mutable_data<int8_t>(TARGET(kHIP));
  }
  return t;
}

// shape outside the fused kernel: the depthwise result in a private tensor, the 1x1 conv reads it
template <PrecisionType Ptype, PrecisionType OutType>
const int8_t* ConvCompute<Ptype, OutType>::DepthwiseIntoMid(const int8_t* x) {
  auto& ctx = this->ctx_->template As<HIPContext>();
  mid_.Resize({conv_.desc.n, conv_.desc.cout, pw_.desc.h, pw_.desc.w});
  int8_t* mid = mid_.mutable_data<int8_t>(TARGET(kHIP));
  HIP_CALL(ctx.ctx(), plhip_depthwise_conv_int8(ctx.ctx(), &conv_.desc, x, conv_.weights->data<int8_t>(), conv_.sc(), conv_.bi(), mid,
                                                PLHIP_OUT_I8));
  return mid;
}

// fusions H1 / F: the uint8 image, or the fp32 input of the calib taken over, is the source (`x` only carries the NCHW shape of an image)
template <PrecisionType Ptype, PrecisionType OutType>
void ConvCompute<Ptype, OutType>::RunStem() {
  auto& param = this->template Param<param_t>();
  auto& ctx = this->ctx_->template As<HIPContext>();
  constexpr bool kInt8Out = OutType == PRECISION(kInt8);
  void* y = Output(kInt8Out);
  const plhip_out_kind kind = kInt8Out ? PLHIP_OUT_I8 : PLHIP_OUT_F32;
  if (route_ == Route::kImageStem) {
    HIP_CALL(ctx.ctx(), plhip_conv2d_image_int8(ctx.ctx(), &conv_.desc, &image_desc_, static_cast<const uint8_t*>(fusion_.image_input->raw_data()),
                                                fusion_.calib_input_scale, conv_.weights->raw_data(), conv_.sc(), conv_.bi(), y, kind));
  } else {
    HIP_CALL(ctx.ctx(), plhip_conv2d_calib_int8(ctx.ctx(), &conv_.desc, param.x->template data<float>(), fusion_.calib_input_scale,
                                                conv_.weights->raw_data(), conv_.sc(), conv_.bi(), y, kind));
  }
}

template <PrecisionType Ptype, PrecisionType OutType>
void ConvCompute<Ptype, OutType>::RunConvTail(const int8_t* x) {
  auto& ctx = this->ctx_->template As<HIPContext>();
  float* y = static_cast<float*>(Output(false, fusion_.drop_fp32_output));
  const Tail t = GatherTail(true);
  void* ws = workspace_bytes_ ? ctx.workspace(workspace_bytes_) : nullptr;
  HIP_CALL(ctx.ctx(), plhip_conv2d_int8_fused(ctx.ctx(), &conv_.desc, x, conv_.weights->raw_data(), conv_.sc(), conv_.bi(), y, t.residual,
                                              fusion_.fuse_residual_relu ? 1 : 0, t.calib_out, fusion_.calib_scale, ws, workspace_bytes_));
}

// fusion G: `output` is the 1x1 conv's tensor, with its tail (residual, calib copy, dropped fp32 output) as RunConvTail's
template <PrecisionType Ptype, PrecisionType OutType>
void ConvCompute<Ptype, OutType>::RunDwConv1x1(const int8_t* x) {
  auto& ctx = this->ctx_->template As<HIPContext>();
  const bool f32 = !fusion_.pw_int8_out;
  void* y = Output(!f32, f32 && fusion_.drop_fp32_output);
  const Tail t = GatherTail(f32);
  const plhip_out_kind kind = f32 ? PLHIP_OUT_F32 : PLHIP_OUT_I8;
  const int relu = fusion_.fuse_residual_relu ? 1 : 0;
  if (route_ == Route::kDwConv1x1Fused) {
    HIP_CALL(ctx.ctx(), plhip_dw_conv1x1_fused_int8(ctx.ctx(), &conv_.desc, x, conv_.weights->data<int8_t>(), conv_.sc(), conv_.bi(),
                                                    pw_.desc.cout, pw_.weights->raw_data(), pw_.sc(), pw_.bi(), pw_.desc.act, pw_.desc.act_alpha,
                                                    y, kind, t.residual, relu, t.calib_out, fusion_.calib_scale));
    return;
  }
  const int8_t* mid = DepthwiseIntoMid(x);
  if (t.residual || t.calib_out) {
    HIP_CALL(ctx.ctx(), plhip_conv2d_int8_fused(ctx.ctx(), &pw_.desc, mid, pw_.weights->raw_data(), pw_.sc(), pw_.bi(), static_cast<float*>(y),
                                                t.residual, relu, t.calib_out, fusion_.calib_scale, nullptr, 0));
  } else {
    HIP_CALL(ctx.ctx(), plhip_conv2d_int8(ctx.ctx(), &pw_.desc, mid, pw_.weights->raw_data(), pw_.sc(), pw_.bi(), y, kind, nullptr, 0));
  }
}

// fusions D / E: `output` is the pointwise conv's tensor (HipConvFusion::pw_*), or the pool's [n, cout, 1, 1] behind it
template <PrecisionType Ptype, PrecisionType OutType>
void ConvCompute<Ptype, OutType>::RunDwPw(const int8_t* x) {
  auto& ctx = this->ctx_->template As<HIPContext>();
  const bool gap = fusion_.pw_global_avg_pool;
  void* y = Output(fusion_.pw_int8_out);
  const plhip_out_kind kind = gap ? PLHIP_OUT_F32_GAP : (fusion_.pw_int8_out ? PLHIP_OUT_I8 : PLHIP_OUT_F32);
  if (route_ == Route::kDwPwFused) {
    HIP_CALL(ctx.ctx(), plhip_dwpw_fused_int8(ctx.ctx(), &conv_.desc, x, conv_.weights->data<int8_t>(), conv_.sc(), conv_.bi(),
                                              pw_.desc.cout, pw_.weights->raw_data(), pw_.sc(), pw_.bi(), pw_.desc.act, pw_.desc.act_alpha, y,
                                              kind));
    return;
  }
  const int8_t* mid = DepthwiseIntoMid(x);
  void* plane = y;
  if (gap) {  // the kernels one by one: the 1x1 conv's plane in a second private tensor, the pool behind it
    mid2_.Resize({conv_.desc.n, pw_.desc.cout, pw_.desc.h, pw_.desc.w});
    plane = mid2_.mutable_data<float>(TARGET(kHIP));
  }
  HIP_CALL(ctx.ctx(), plhip_conv2d_int8(ctx.ctx(), &pw_.desc, mid, pw_.weights->raw_data(), pw_.sc(), pw_.bi(), plane,
                                        gap ? PLHIP_OUT_F32 : kind, nullptr, 0));
  if (gap) {
    HIP_CALL(ctx.ctx(), plhip_global_avg_pool_f32(ctx.ctx(), static_cast<const float*>(plane), conv_.desc.n * pw_.desc.cout,
                                                  pw_.desc.h * pw_.desc.w, static_cast<float*>(y)));
  }
}

template <PrecisionType Ptype, PrecisionType OutType>
void ConvCompute<Ptype, OutType>::Run() {
  auto& param = this->template Param<param_t>();
  auto& ctx = this->ctx_->template As<HIPContext>();
  if (fusion_.image_input) {
    CHECK(fusion_.image_input->target() == TARGET(kHIP)) << "conv image source must live on the HIP device (io_copy missing?)";
  } else {
    CHECK(param.x->target() == TARGET(kHIP)) << "conv input must live on the HIP device (io_copy missing?)";
  }
  const bool stem = route_ == Route::kImageStem || route_ == Route::kCalibStem;  // the one-launch stems read their source themselves
  const int8_t* x = stem ? nullptr : Int8Input();
  constexpr bool kInt8Out = OutType == PRECISION(kInt8);
  const plhip_out_kind kind = kInt8Out ? PLHIP_OUT_I8 : PLHIP_OUT_F32;
  switch (route_) {
    case Route::kImageStem:
    case Route::kCalibStem: return RunStem();
    case Route::kConvTail: return RunConvTail(x);
    case Route::kDwConv1x1Fused:
    case Route::kDwConv1x1Split: return RunDwConv1x1(x);
    case Route::kDwPwFused:
    case Route::kDwPwSplit: return RunDwPw(x);
    case Route::kDepthwise:
      HIP_CALL(ctx.ctx(), plhip_depthwise_conv_int8(ctx.ctx(), &conv_.desc, x, conv_.weights->data<int8_t>(), conv_.sc(), conv_.bi(),
                                                    Output(kInt8Out), kind));
      return;
    case Route::kConv: {
      void* ws = workspace_bytes_ ? ctx.workspace(workspace_bytes_) : nullptr;
      HIP_CALL(ctx.ctx(), plhip_conv2d_int8(ctx.ctx(), &conv_.desc, x, conv_.weights->raw_data(), conv_.sc(), conv_.bi(), Output(kInt8Out), kind,
                                            ws, workspace_bytes_));
    }
  }
}

template class ConvCompute<PRECISION(kInt8), PRECISION(kInt8)>;
template class ConvCompute<PRECISION(kInt8), PRECISION(kFloat)>;

}  // namespace hip
}  // namespace kernels
}  // namespace lite
}  // namespace paddle

typedef paddle::lite::kernels::hip::ConvCompute<PRECISION(kInt8), PRECISION(kFloat)> ConvInt8_Fp32;
typedef paddle::lite::kernels::hip::ConvCompute<PRECISION(kInt8), PRECISION(kInt8)> ConvInt8_Int8;

// Same argument names, precisions and aliases as lite/kernels/arm/conv_compute.cc:216-252, target kHIP.
REGISTER_LITE_KERNEL(conv2d, kHIP, kInt8, kNCHW, ConvInt8_Int8, int8_out)
    .BindInput("Input", {LiteType::GetTensorTy(TARGET(kHIP), PRECISION(kInt8))})
    .BindInput("Bias", {LiteType::GetTensorTy(TARGET(kHIP), PRECISION(kFloat))})
    .BindInput("Filter", {LiteType::GetTensorTy(TARGET(kHIP), PRECISION(kInt8))})
    .BindOutput("Output", {LiteType::GetTensorTy(TARGET(kHIP), PRECISION(kInt8))})
    .Finalize();

REGISTER_LITE_KERNEL(conv2d, kHIP, kInt8, kNCHW, ConvInt8_Fp32, fp32_out)
    .BindInput("Input", {LiteType::GetTensorTy(TARGET(kHIP), PRECISION(kInt8))})
    .BindInput("Bias", {LiteType::GetTensorTy(TARGET(kHIP), PRECISION(kFloat))})
    .BindInput("Filter", {LiteType::GetTensorTy(TARGET(kHIP), PRECISION(kInt8))})
    .BindOutput("Output", {LiteType::GetTensorTy(TARGET(kHIP), PRECISION(kFloat))})
    .Finalize();

REGISTER_LITE_KERNEL(depthwise_conv2d, kHIP, kInt8, kNCHW, ConvInt8_Int8, int8_out)
    .BindInput("Input", {LiteType::GetTensorTy(TARGET(kHIP), PRECISION(kInt8))})
    .BindInput("Bias", {LiteType::GetTensorTy(TARGET(kHIP), PRECISION(kFloat))})
    .BindInput("Filter", {LiteType::GetTensorTy(TARGET(kHIP), PRECISION(kInt8))})
    .BindOutput("Output", {LiteType::GetTensorTy(TARGET(kHIP), PRECISION(kInt8))})
    .Finalize();

REGISTER_LITE_KERNEL(depthwise_conv2d, kHIP, kInt8, kNCHW, ConvInt8_Fp32, fp32_out)
    .BindInput("Input", {LiteType::GetTensorTy(TARGET(kHIP), PRECISION(kInt8))})
    .BindInput("Bias", {LiteType::GetTensorTy(TARGET(kHIP), PRECISION(kFloat))})
    .BindInput("Filter", {LiteType::GetTensorTy(TARGET(kHIP), PRECISION(kInt8))})
    .BindOutput("Output", {LiteType::GetTensorTy(TARGET(kHIP), PRECISION(kFloat))})
    .Finalize();
