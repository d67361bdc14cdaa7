// hip_predictor.cc — see hip_predictor.h.
#include "lite/api/hip_predictor.h"

#include "lite/kernels/hip/calib_tail.h"
#include "lite/kernels/hip/detection_fusion.h"
#include "lite/kernels/hip/interp_fusion.h"
#include "lite/kernels/hip/prior_box_host.h"
#include "lite/kernels/hip/conv_fusion.h"
#include "lite/kernels/hip/image_frame.h"
#include "lite/kernels/hip/se_gate_fusion.h"
#include "lite/kernels/hip/shuffle_fusion.h"
#include "lite/kernels/hip/yolo_fusion.h"
#include "lite/kernels/hip/image_to_tensor.h"
#include "plhip.h"

#include <cstring>

namespace paddle {
namespace lite {

std::unique_ptr<KernelBase> PickKernel(const std::string& op_type, const Place& place, const std::string& alias) {
  auto ks = KernelFactory::Global().Create(op_type, place.target, place.precision, place.layout);
  for (auto& k : ks)
    if (k->alias() == alias) return std::move(k);
  LOG(FATAL) << "no kernel registered for " << op_type << "/" << alias << " at " << place.DebugString()
             << "; registered ops:\n" << KernelFactory::Global().DebugString();
  return nullptr;
}

// The picked kernel, and in *as the interface I of lite/kernels/hip/*_fusion.h through which this target's fusion state reaches it
template <class I>
static std::unique_ptr<KernelBase> PickAs(const std::string& op_type, const Place& place, const std::string& alias, I** as) {
  auto kernel = PickKernel(op_type, place, alias);
  *as = dynamic_cast<I*>(kernel.get());
  CHECK(*as) << "the picked " << op_type << "/" << alias << " kernel does not take the kHIP fusion state it is handed";
  return kernel;
}

// The calib[fp32_to_int8](scale) an fp32 op took over: it writes the int8 variable `name`; drop: the op's fp32 output is not written
static kernels::hip::HipCalibTail MakeCalibTail(HipPredictor* pred, const std::string& name, float scale, bool drop) {
  kernels::hip::HipCalibTail t;
  t.calib_output = pred->Var(name);
  t.calib_output->set_precision(PRECISION(kInt8));
  t.calib_scale = scale;
  t.drop_fp32_output = drop;
  return t;
}

// ConvAttrs' act / act_coef as an ActivationParam.  ConvParam::fuse_relu has no counterpart here: the conv ops set it themselves.
static void FillActivation(operators::ActivationParam* ap, int act, float coef) {
  if (act == 0) return;
  ap->has_active = true;
  ap->active_type = static_cast<lite_api::ActivationType>(act);
  if (act == 2) ap->Relu_clipped_coef = coef;
  if (act == 4) ap->Leaky_relu_alpha = coef;
}

void HipPredictor::UploadWeights(const int8_t* w, const std::vector<int64_t>& w_dims, const float* bias, int64_t cout, Tensor** filter,
                                 Tensor** bias_out) {
  size_t wn = 1;
  for (auto d : w_dims) wn *= static_cast<size_t>(d);
  *filter = NewParam(w, wn, w_dims, PRECISION(kInt8));
  *bias_out = bias ? NewParam(bias, static_cast<size_t>(cout) * 4, {cout}, PRECISION(kFloat)) : nullptr;
}

Tensor* HipPredictor::Var(const std::string& name) {
  auto it = vars_.find(name);
  if (it == vars_.end()) it = vars_.emplace(name, std::unique_ptr<Tensor>(new Tensor)).first;
  return it->second.get();
}

Tensor* HipPredictor::NewParam(const void* host, size_t bytes, const std::vector<int64_t>& dims, PrecisionType prec) {
  params_.emplace_back(new Tensor);
  Tensor* t = params_.back().get();
  t->Resize(dims);
  t->set_persistable(true);
  void* p = t->mutable_data(TARGET(kHost), bytes);
  t->set_precision(prec);
  std::memcpy(p, host, bytes);
  return t;
}

const std::shared_ptr<HipExecState>& HipPredictor::state() {
  if (!state_) {
    TargetWrapperHip::SetDevice(device_);
    state_ = TargetWrapperHip::State();
  }
  return state_;
}

void HipPredictor::Emit(std::shared_ptr<OpLite> op, std::unique_ptr<KernelBase> kernel) {
  kernel->SetContext(NewContext(TARGET(kHIP), device_, state()));
  op->AttachKernel(kernel.get());
  program_.Add(Instruction(std::move(op), std::move(kernel)));
}

Tensor* HipPredictor::AddFeed(const std::string& name, const std::vector<int64_t>& dims, PrecisionType prec) {
  Tensor* t = Var(name);
  t->Resize(dims);
  const size_t esz = prec == PRECISION(kInt8) || prec == PRECISION(kUInt8) ? 1 : 4;
  t->mutable_data(TARGET(kHost), static_cast<size_t>(t->numel()) * esz);
  t->set_precision(prec);
  // a feed declared again: the kernel objects re-initialise on the next run (repacked weights, private tensors, grown buffers),
  // and none of those addresses is in GraphKey — a recorded launch graph is stale even if every shape comes back to what it was
  graph_stale_ = true;
  return t;
}

void HipPredictor::AddIoCopy(const std::string& in, const std::string& out, bool h2d) {
  auto op = std::make_shared<operators::IoCopyOp>();
  op->mutable_param().x = Var(in);
  op->mutable_param().y = Var(out);
  Emit(op, PickKernel("io_copy", Place(TARGET(kHIP), PRECISION(kAny), DATALAYOUT(kAny)),
                      h2d ? "host_to_device" : "device_to_host"));
}

void HipPredictor::AddCalib(const std::string& in, const std::string& out, float scale, bool f2i) {
  auto op = std::make_shared<operators::CalibOpLite>();
  op->mutable_param().input = Var(in);
  op->mutable_param().output = Var(out);
  op->mutable_param().scale = scale;
  Emit(op, PickKernel("calib", Place(TARGET(kHIP), PRECISION(kInt8)), f2i ? "fp32_to_int8" : "int8_to_fp32"));
}

void HipPredictor::AddImageToTensor(const std::string& in, const std::string& out, int format, const float* means,
                                    const float* scales, float calib_scale) {
  auto op = std::make_shared<operators::ImageToTensorOp>();
  auto& p = op->mutable_param();
  p.x = Var(in);
  p.output = Var(out);
  p.format = format;
  for (int i = 0; i < 3; ++i) {
    p.means[i] = means[i];
    p.scales[i] = scales[i];
  }
  p.int8_out = calib_scale > 0.f;
  p.calib_scale = p.int8_out ? calib_scale : 1.f;
  Emit(op, PickKernel("image_to_tensor", Place(TARGET(kHIP), PRECISION(kAny)), p.int8_out ? "int8" : "fp32"));
}

void HipPredictor::AddImageConvert(const std::string& in, const std::string& out, int src_format, int dst_format) {
  auto op = std::make_shared<operators::ImageConvertOp>();
  auto& p = op->mutable_param();
  p.x = Var(in);
  p.output = Var(out);
  p.src_format = src_format;
  p.dst_format = dst_format;
  Emit(op, PickKernel("image_convert", Place(TARGET(kHIP), PRECISION(kAny)), "def"));
}

void HipPredictor::AddImageResize(const std::string& in, const std::string& out, int frame_format, int out_h, int out_w,
                                  const float* means, const float* scales, float calib_scale) {
  auto op = std::make_shared<operators::ImageResizeOp>();
  auto& p = op->mutable_param();
  p.x = Var(in);
  p.output = Var(out);
  p.format = frame_format;
  p.out_h = out_h;
  p.out_w = out_w;
  p.to_tensor = means != nullptr;
  for (int i = 0; i < 3 && p.to_tensor; ++i) {
    p.means[i] = means[i];
    p.scales[i] = scales[i];
  }
  p.int8_out = p.to_tensor && calib_scale > 0.f;
  p.calib_scale = p.int8_out ? calib_scale : 1.f;
  Emit(op, PickKernel("image_resize", Place(TARGET(kHIP), PRECISION(kAny)), !p.to_tensor ? "uint8" : p.int8_out ? "int8" : "fp32"));
}

void HipPredictor::AddConv(const std::string& op_type, const std::string& in, const std::string& out, const int8_t* w,
                           const std::vector<int64_t>& w_dims, const float* bias, const ConvAttrs& a) {
  auto op = std::make_shared<operators::ConvOpLite>(op_type);
  auto& p = op->mutable_param();
  kernels::hip::HipConvFusion fz;  // this target's graph-level fusion state (lite/kernels/hip/conv_fusion.h)
  const bool fused = !a.calib_out.empty() || !a.residual.empty() || a.pw_w != nullptr || a.in_calib_scale > 0.f;
  p.x = a.image_format >= 0 ? Var(a.image_x) : Var(in);
  p.output = Var(out);
  UploadWeights(w, w_dims, bias, w_dims[0], &p.filter, &p.bias);
  p.strides = a.strides;
  p.paddings = std::make_shared<std::vector<int>>(a.paddings);
  p.dilations = std::make_shared<std::vector<int>>(a.dilations);
  p.groups = a.groups;
  p.enable_int8 = true;
  p.input_scale = a.input_scale;
  p.output_scale = a.output_scale;
  p.weight_scale = a.weight_scale;
  FillActivation(&p.activation_param, a.act, a.act_coef);
  if (a.act == 1) p.fuse_relu = true;
  if (!a.residual.empty()) {
    CHECK(!a.int8_out || (a.pw_tail && !a.pw_int8_out)) << "the fused residual add belongs to the fp32_out kernel";
    p.fuse_residual_connection = true;
    p.residualData = Var(a.residual);
    fz.fuse_residual_relu = a.residual_relu;
  }
  if (!a.calib_out.empty()) {
    CHECK(!a.int8_out || (a.pw_tail && !a.pw_int8_out)) << "the fused calib belongs to the fp32_out kernel";
    const kernels::hip::HipCalibTail t = MakeCalibTail(this, a.calib_out, a.calib_scale, a.drop_fp32);
    fz.calib_output = t.calib_output;  // HipConvFusion keeps the three fields flat (calib_tail.h says why)
    fz.calib_scale = t.calib_scale;
    fz.drop_fp32_output = t.drop_fp32_output;
  }
  if (a.pw_w) {
    CHECK(a.int8_out && op_type == "depthwise_conv2d") << "only a depthwise conv with int8 output takes a 1x1 consumer over";
    UploadWeights(a.pw_w, a.pw_w_dims, a.pw_bias, a.pw_w_dims[0], &fz.pw_filter, &fz.pw_bias);
    op->set_output_channels(a.pw_w_dims[0]);
    fz.pw_weight_scale = a.pw_weight_scale;
    fz.pw_output_scale = a.pw_output_scale;
    fz.pw_int8_out = a.pw_int8_out;
    FillActivation(&fz.pw_activation_param, a.pw_act, a.pw_act_coef);
    p.output->set_precision(a.pw_int8_out ? PRECISION(kInt8) : PRECISION(kFloat));
    fz.pw_tail = a.pw_tail;
    if (a.pw_pool) {
      CHECK(!a.pw_int8_out) << "the fused global average pool reads the 1x1 conv's fp32 output";
      fz.pw_global_avg_pool = true;
      op->set_output_pooled();
    }
  }
  if (a.in_calib_scale > 0.f) fz.calib_input_scale = a.in_calib_scale;
  if (a.image_format >= 0) {  // fusion H1: the conv reads the uint8 image `in`; `x` only carries the NCHW shape made from it
    CHECK(a.in_calib_scale > 0.f) << "an image source needs the calib scale of the int8 stem";
    const Tensor* img = Var(in);
    fz.image_input = img;
    fz.image_format = a.image_format;
    for (int i = 0; i < 3; ++i) {
      fz.image_means[i] = a.image_means[i];
      fz.image_scales[i] = a.image_scales[i];
    }
    op->set_image_input(img, operators::ImageChannels(a.image_format));
  }
  op->set_padding_algorithm(a.padding_algorithm);
  // this target's fusion state goes to the kernel object, not into the reference's ConvParam (conv_fusion.h); every kHIP conv
  // kernel takes one, and one that never receives it is the plain drop-in conv
  kernels::hip::HipFusableKernel* fk;
  auto kernel = PickAs(op_type, Place(TARGET(kHIP), PRECISION(kInt8)), a.int8_out ? "int8_out" : "fp32_out", &fk);
  if (fused) fk->SetFusion(fz);
  Emit(op, std::move(kernel));
}

void HipPredictor::AddConvTranspose(const std::string& in, const std::string& out, const int8_t* w, const std::vector<int64_t>& w_dims,
                                    const float* bias, const ConvAttrs& a) {
  CHECK(a.residual.empty() && a.calib_out.empty() && !a.pw_w && !(a.in_calib_scale > 0.f) && a.image_format < 0)
      << "conv2d_transpose takes no kHIP fusion";
  CHECK_EQ(w_dims.size(), 4UL);
  auto op = std::make_shared<operators::ConvTransposeOpLite>();
  auto& p = op->mutable_param();
  p.x = Var(in);
  p.output = Var(out);
  UploadWeights(w, w_dims, bias, w_dims[1] * a.groups, &p.filter, &p.bias);
  p.strides = a.strides;
  p.paddings = std::make_shared<std::vector<int>>(a.paddings);
  p.dilations = std::make_shared<std::vector<int>>(a.dilations);
  p.groups = a.groups;
  p.output_size = a.output_size;
  p.enable_int8 = true;
  p.input_scale = a.input_scale;
  p.output_scale = a.output_scale;
  p.weight_scale = a.weight_scale;
  FillActivation(&p.activation_param, a.act, a.act_coef);
  if (a.act == 1) p.fuse_relu = true;
  op->set_padding_algorithm(a.padding_algorithm);
  Emit(op, PickKernel("conv2d_transpose", Place(TARGET(kHIP), PRECISION(kInt8)), a.int8_out ? "int8_out" : "fp32_out"));
}

void HipPredictor::AddFc(const std::string& in, const std::string& out, const int8_t* w, int k, int n, const float* bias,
                         float input_scale, const std::vector<float>& weight_scale, float output_scale, bool int8_out,
                         bool relu) {
  auto op = std::make_shared<operators::FcOpLite>();
  auto& p = op->mutable_param();
  p.input = Var(in);
  p.output = Var(out);
  p.w = NewParam(w, static_cast<size_t>(k) * n, {k, n}, PRECISION(kInt8));
  p.bias = bias ? NewParam(bias, static_cast<size_t>(n) * 4, {n}, PRECISION(kFloat)) : nullptr;
  p.in_num_col_dims = 1;
  p.enable_int8 = true;
  p.input_scale = input_scale;
  p.weight_scale = weight_scale;
  p.output_scale = output_scale;
  if (relu) p.activation_type = "relu";
  Emit(op, PickKernel("fc", Place(TARGET(kHIP), PRECISION(kInt8)), int8_out ? "int8out" : "fp32out"));
}

void HipPredictor::AddGlobalAvgPool(const std::string& in, const std::string& out) {
  auto op = std::make_shared<operators::PoolOpLite>();
  auto& p = op->mutable_param();
  p.x = Var(in);
  p.output = Var(out);
  p.pooling_type = "avg";
  p.global_pooling = true;
  p.paddings = std::make_shared<std::vector<int>>(std::vector<int>{0, 0, 0, 0});
  Emit(op, PickKernel("pool2d", Place(TARGET(kHIP), PRECISION(kFloat)), "def"));
}

void HipPredictor::AddPool(const std::string& in, const std::string& out, const std::string& pooling_type,
                           const std::vector<int>& ksize, const std::vector<int>& strides, const std::vector<int>& paddings,
                           bool global_pooling, bool exclusive, bool ceil_mode, bool int8) {
  auto op = std::make_shared<operators::PoolOpLite>();
  auto& p = op->mutable_param();
  p.x = Var(in);
  p.output = Var(out);
  p.pooling_type = pooling_type;
  p.ksize = ksize;
  p.strides = strides;
  p.global_pooling = global_pooling;
  p.exclusive = exclusive;
  p.ceil_mode = ceil_mode;
  p.paddings = std::make_shared<std::vector<int>>(paddings);
  Emit(op, PickKernel("pool2d", Place(TARGET(kHIP), int8 ? PRECISION(kInt8) : PRECISION(kFloat)), "def"));
}

void HipPredictor::AddElementwiseAdd(const std::string& x, const std::string& y, const std::string& out,
                                     const std::string& act_type) {
  if (act_type.empty()) {
    auto op = std::make_shared<operators::ElementwiseOp>("elementwise_add");
    auto& p = op->mutable_param();
    p.X = Var(x);
    p.Y = Var(y);
    p.Out = Var(out);
    Emit(op, PickKernel("elementwise_add", Place(TARGET(kHIP), PRECISION(kFloat)), "def"));
  } else {
    auto op = std::make_shared<operators::FusionElementwiseActivationOp>("fusion_elementwise_add_activation");
    auto& p = op->mutable_param();
    p.X = Var(x);
    p.Y = Var(y);
    p.Out = Var(out);
    p.act_type = act_type;
    Emit(op, PickKernel("fusion_elementwise_add_activation", Place(TARGET(kHIP), PRECISION(kFloat)), "def"));
  }
}

void HipPredictor::AddSoftmax(const std::string& in, const std::string& out) {
  auto op = std::make_shared<operators::SoftmaxOp>();
  op->mutable_param().x = Var(in);
  op->mutable_param().output = Var(out);
  op->mutable_param().axis = -1;
  Emit(op, PickKernel("softmax", Place(TARGET(kHIP), PRECISION(kFloat)), "def"));
}

// the "int8" alias of an fp32 op (registered at tail_precision) with its calib tail attached, or, calib_out == "", the plain "def" kernel
static std::unique_ptr<KernelBase> PickWithCalibTail(HipPredictor* pred, const std::string& op_type, PrecisionType tail_precision,
                                                     const std::string& calib_out, float calib_scale, bool drop_fp32) {
  if (calib_out.empty()) return PickKernel(op_type, Place(TARGET(kHIP), PRECISION(kFloat)), "def");
  kernels::hip::HipCalibTailKernel* tk;
  auto kernel = PickAs(op_type, Place(TARGET(kHIP), tail_precision), "int8", &tk);
  tk->SetCalibTail(MakeCalibTail(pred, calib_out, calib_scale, drop_fp32));
  return kernel;
}

void HipPredictor::AddActivation(const std::string& op_type, const std::string& in, const std::string& out,
                                 const std::string& calib_out, float calib_scale, bool drop_fp32) {
  CHECK(op_type == "hard_swish" || op_type == "hard_sigmoid") << "kHIP has no activation kernel for " << op_type;
  auto op = std::make_shared<operators::ActivationOp>(op_type);
  auto& p = op->mutable_param();
  p.X = Var(in);
  p.Out = Var(out);
  p.has_active = true;
  p.active_type = op_type == "hard_swish" ? lite_api::ActivationType::kHardSwish : lite_api::ActivationType::kHardSigmoid;
  Emit(op, PickWithCalibTail(this, op_type, PRECISION(kFloat), calib_out, calib_scale, drop_fp32));
}

void HipPredictor::AddSeGate(const std::string& in, const std::string& out, float calib_scale, const int8_t* w1,
                             const std::vector<int64_t>& w1_dims, const float* bias1, const ConvAttrs& a1, const int8_t* w2,
                             const std::vector<int64_t>& w2_dims, const float* bias2, const ConvAttrs& a2) {
  auto op = std::make_shared<operators::ActivationOp>("hard_sigmoid");
  auto& p = op->mutable_param();
  p.X = Var(in);
  p.Out = Var(out);
  p.has_active = true;
  p.active_type = lite_api::ActivationType::kHardSigmoid;
  kernels::hip::HipSeGateFusion fz;
  fz.calib_scale = calib_scale;
  auto fill = [this](kernels::hip::HipSeGateConv* c, const int8_t* w, const std::vector<int64_t>& wd, const float* bias, const ConvAttrs& a) {
    UploadWeights(w, wd, bias, wd[0], &c->filter, &c->bias);
    c->weight_scale = a.weight_scale;
    c->input_scale = a.input_scale;
    FillActivation(&c->activation_param, a.act, a.act_coef);
  };
  fill(&fz.reduce, w1, w1_dims, bias1, a1);
  fill(&fz.expand, w2, w2_dims, bias2, a2);
  kernels::hip::HipSeGateKernel* gk;
  auto kernel = PickAs("hard_sigmoid", Place(TARGET(kHIP), PRECISION(kFloat)), "se_gate", &gk);
  gk->SetSeGate(fz);
  Emit(op, std::move(kernel));
}

void HipPredictor::AddElementwiseMul(const std::string& x, const std::string& y, const std::string& out, int axis,
                                     const std::string& calib_out, float calib_scale, bool drop_fp32) {
  auto op = std::make_shared<operators::ElementwiseMulOp>();
  auto& p = op->mutable_param();
  p.X = Var(x);
  p.Y = Var(y);
  p.Out = Var(out);
  p.axis = axis;
  Emit(op, PickWithCalibTail(this, "elementwise_mul", PRECISION(kFloat), calib_out, calib_scale, drop_fp32));
}

void HipPredictor::AddConcat(const std::vector<std::string>& inputs, const std::string& out, int axis) {
  auto op = std::make_shared<operators::ConcatOpLite>();
  auto& p = op->mutable_param();
  for (auto& in : inputs) p.x.push_back(Var(in));
  p.output = Var(out);
  p.axis = axis;
  Emit(op, PickKernel("concat", Place(TARGET(kHIP), PRECISION(kFloat)), "def"));
}

void HipPredictor::AddSplit(const std::string& in, const std::vector<std::string>& outs, int axis, int num,
                            const std::vector<int>& sections) {
  auto op = std::make_shared<operators::SplitOp>();
  auto& p = op->mutable_param();
  p.x = Var(in);
  for (auto& o : outs) p.output.push_back(Var(o));
  p.axis = axis;
  p.num = num;
  p.sections = sections;
  Emit(op, PickKernel("split", Place(TARGET(kHIP), PRECISION(kFloat)), "def"));
}

void HipPredictor::AddShuffleChannel(const std::string& in, const std::string& out, int group) {
  auto op = std::make_shared<operators::ShuffleChannelOpLite>();
  auto& p = op->mutable_param();
  p.X = Var(in);
  p.Out = Var(out);
  p.group = group;
  Emit(op, PickKernel("shuffle_channel", Place(TARGET(kHIP), PRECISION(kFloat)), "def"));
}

void HipPredictor::AddShuffleUnit(const std::string& a, const std::string& b, const std::string& lo, const std::string& hi,
                                  const std::string& calib_out, float calib_scale, bool drop_fp32) {
  const bool unit = !lo.empty();
  CHECK(!hi.empty()) << "AddShuffleUnit: the variable behind the shuffle (or its second half) must be named";
  CHECK(!drop_fp32 || !calib_out.empty()) << "AddShuffleUnit: only a tensor whose int8 image is written can be dropped";
  auto op = std::make_shared<operators::ShuffleChannelOpLite>();
  auto& p = op->mutable_param();
  p.X = Var(a);
  p.Out = Var(unit ? lo : hi);
  p.group = 2;
  if (!unit) op->set_output_channel_factor(2);
  kernels::hip::HipShuffleFusion fz;
  fz.second = Var(b);
  if (unit) fz.hi_output = Var(hi);
  if (!calib_out.empty()) fz.tail = MakeCalibTail(this, calib_out, calib_scale, drop_fp32);
  kernels::hip::HipShuffleFusionKernel* sk;
  auto kernel = PickAs("shuffle_channel", Place(TARGET(kHIP), PRECISION(kFloat)), unit ? "unit" : "int8", &sk);
  sk->SetShuffleFusion(fz);
  Emit(op, std::move(kernel));
}

void HipPredictor::AddConcatCalib(const std::vector<std::string>& inputs, const std::string& out, int axis, const std::string& calib_out,
                                  float calib_scale, bool drop_fp32) {
  CHECK(!calib_out.empty()) << "AddConcatCalib: the int8 tensor must be named";
  auto op = std::make_shared<operators::ConcatOpLite>();
  auto& p = op->mutable_param();
  for (auto& in : inputs) p.x.push_back(Var(in));
  p.output = Var(out);
  p.axis = axis;
  Emit(op, PickWithCalibTail(this, "concat", PRECISION(kAny), calib_out, calib_scale, drop_fp32));
}

static void SetInterpAttrs(operators::InterpolateParam* p, const std::string& op_type, int out_h, int out_w, float scale,
                           bool align_corners, int align_mode) {
  CHECK(op_type == "bilinear_interp" || op_type == "nearest_interp") << "kHIP has no interp kernel for " << op_type;
  p->out_h = out_h;
  p->out_w = out_w;
  p->scale = scale;
  p->align_corners = align_corners;
  p->align_mode = align_mode;
  p->interp_method = op_type == "bilinear_interp" ? "Bilinear" : "Nearest";
}

void HipPredictor::AddInterp(const std::string& op_type, const std::string& in, const std::string& out, int out_h, int out_w, float scale,
                             bool align_corners, int align_mode, const std::string& calib_out, float calib_scale, bool drop_fp32) {
  CHECK(!drop_fp32 || !calib_out.empty()) << "AddInterp: only a tensor whose int8 image is written can be dropped";
  auto op = std::make_shared<operators::InterpolateOp>(op_type);
  auto& p = op->mutable_param();
  SetInterpAttrs(&p, op_type, out_h, out_w, scale, align_corners, align_mode);
  p.X = Var(in);
  p.Out = Var(out);
  Emit(op, PickWithCalibTail(this, op_type, PRECISION(kAny), calib_out, calib_scale, drop_fp32));
}

void HipPredictor::AddArgMax(const std::string& in, const std::string& out, int axis, int dtype, bool keepdims) {
  auto op = std::make_shared<operators::ArgmaxOpLite>();
  auto& p = op->mutable_param();
  p.X = Var(in);
  p.Out = Var(out);
  p.Axis = axis;
  p.dtype = dtype;
  p.keepdims = keepdims;
  Emit(op, PickKernel("arg_max", Place(TARGET(kHIP), PRECISION(kAny)), "def"));
}

void HipPredictor::AddInterpArgMax(const std::string& op_type, const std::string& in, const std::string& out, int out_h, int out_w,
                                   float scale, bool align_corners, int align_mode, int dtype, bool keepdims) {
  kernels::hip::HipInterpArgmaxFusion fz;
  fz.op_type = op_type;
  SetInterpAttrs(&fz.interp, op_type, out_h, out_w, scale, align_corners, align_mode);
  auto op = std::make_shared<operators::ArgmaxOpLite>();
  auto& p = op->mutable_param();
  p.X = Var(in);
  p.Out = Var(out);
  p.Axis = 1;
  p.dtype = dtype;
  p.keepdims = keepdims;
  op->set_interp(fz.interp);
  kernels::hip::HipInterpArgmaxKernel* ak;
  auto kernel = PickAs("arg_max", Place(TARGET(kHIP), PRECISION(kAny)), "interp", &ak);
  ak->SetInterpArgmax(fz);
  Emit(op, std::move(kernel));
}

void HipPredictor::AddTranspose(const std::string& in, const std::string& out, const std::vector<int>& perm) {
  auto op = std::make_shared<operators::TransposeOpLite>("transpose");
  auto& p = op->mutable_param();
  p.x = Var(in);
  p.output = Var(out);
  p.axis = perm;
  Emit(op, PickKernel("transpose", Place(TARGET(kHIP), PRECISION(kFloat)), "def"));
}

void HipPredictor::AddReshape(const std::string& in, const std::string& out, const std::vector<int>& shape) {
  auto op = std::make_shared<operators::ReshapeOpLite>("reshape");
  auto& p = op->mutable_param();
  p.x = Var(in);
  p.output = Var(out);
  p.shape_vct = shape;
  Emit(op, PickKernel("reshape", Place(TARGET(kHIP), PRECISION(kFloat)), "def"));
}

void HipPredictor::AddPriorBox(const std::string& input, const std::string& image, const std::string& boxes, const std::string& variances,
                               const std::vector<float>& min_sizes, const std::vector<float>& max_sizes,
                               const std::vector<float>& aspect_ratios, const std::vector<float>& variance, bool flip, bool clip,
                               float step_w, float step_h, float offset, bool min_max_aspect_ratios_order) {
  auto op = std::make_shared<operators::PriorBoxOpLite>();
  auto& p = op->mutable_param();
  p.input = Var(input);
  p.image = Var(image);
  p.boxes = Var(boxes);
  p.variances = Var(variances);
  p.min_sizes = min_sizes;
  p.max_sizes = max_sizes;
  p.aspect_ratios = aspect_ratios;
  p.variances_ = variance;
  p.flip = flip;
  p.clip = clip;
  p.step_w = step_w;
  p.step_h = step_h;
  p.offset = offset;
  p.min_max_aspect_ratios_order = min_max_aspect_ratios_order;
  p.prior_num = kernels::hip::PriorBoxNum(min_sizes, max_sizes, aspect_ratios, flip);
  Emit(op, PickKernel("prior_box", Place(TARGET(kHIP), PRECISION(kFloat)), "def"));
}

void HipPredictor::AddBoxCoder(const std::string& prior, const std::string& prior_var, const std::string& target, const std::string& out,
                               const std::vector<float>& variance, int axis, bool normalized) {
  auto op = std::make_shared<operators::BoxCoderOpLite>();
  auto& p = op->mutable_param();
  p.prior_box = Var(prior);
  p.prior_box_var = prior_var.empty() ? nullptr : Var(prior_var);
  p.target_box = Var(target);
  p.proposals = Var(out);
  p.code_type = "decode_center_size";
  p.box_normalized = normalized;
  p.axis = axis;
  p.variance = variance;
  Emit(op, PickKernel("box_coder", Place(TARGET(kHIP), PRECISION(kFloat)), "def"));
}

void HipPredictor::AddMulticlassNms(const std::string& boxes, const std::string& scores, const std::string& out, const std::string& index,
                                    int background_label, float score_threshold, int nms_top_k, float nms_threshold, float nms_eta,
                                    int keep_top_k, bool normalized, bool scores_npc) {
  auto op = std::make_shared<operators::MulticlassNmsOpLite>();
  auto& p = op->mutable_param();
  p.bboxes = Var(boxes);
  p.scores = Var(scores);
  p.out = Var(out);
  p.index = index.empty() ? nullptr : Var(index);
  if (p.index) p.index->set_precision(PRECISION(kInt32));
  p.background_label = background_label;
  p.score_threshold = score_threshold;
  p.nms_top_k = nms_top_k;
  p.nms_threshold = nms_threshold;
  p.nms_eta = nms_eta;
  p.keep_top_k = keep_top_k;
  p.normalized = normalized;
  kernels::hip::HipNmsFusion fz;
  fz.count = Var(out + "/count");
  fz.count->set_precision(PRECISION(kInt32));
  fz.scores_npc = scores_npc;
  op->set_count(fz.count);
  op->set_scores_npc(scores_npc);
  kernels::hip::HipNmsFusionKernel* nk;
  auto kernel = PickAs("multiclass_nms", Place(TARGET(kHIP), PRECISION(kFloat)), "def", &nk);
  nk->SetNmsFusion(fz);
  Emit(op, std::move(kernel));
}

void HipPredictor::AddYoloBox(const std::string& x, const std::string& img_size, const std::string& boxes, const std::string& scores,
                              const std::vector<int>& anchors, int class_num, float conf_thresh, int downsample_ratio, bool clip_bbox,
                              float scale_x_y) {
  auto op = std::make_shared<operators::YoloBoxOpLite>();
  auto& p = op->mutable_param();
  p.X = Var(x);
  p.ImgSize = Var(img_size);
  p.Boxes = Var(boxes);
  p.Scores = Var(scores);
  p.anchors = anchors;
  p.class_num = class_num;
  p.conf_thresh = conf_thresh;
  p.downsample_ratio = downsample_ratio;
  p.clip_bbox = clip_bbox;
  p.scale_x_y = scale_x_y;
  Emit(op, PickKernel("yolo_box", Place(TARGET(kHIP), PRECISION(kFloat)), "def"));
}

void HipPredictor::AddYoloHead(const std::vector<std::string>& xs, const std::string& img_size, const std::string& boxes,
                               const std::string& scores, const std::vector<std::vector<int>>& anchors, int class_num, float conf_thresh,
                               const std::vector<int>& downsample_ratios, bool clip_bbox, float scale_x_y) {
  CHECK(!xs.empty() && xs.size() == anchors.size() && xs.size() == downsample_ratios.size()) << "AddYoloHead: one anchor list and one ratio per map";
  auto op = std::make_shared<operators::YoloBoxOpLite>();
  auto& p = op->mutable_param();
  p.X = Var(xs[0]);
  p.ImgSize = Var(img_size);
  p.Boxes = Var(boxes);
  p.Scores = Var(scores);
  p.anchors = anchors[0];
  p.class_num = class_num;
  p.conf_thresh = conf_thresh;
  p.downsample_ratio = downsample_ratios[0];
  p.clip_bbox = clip_bbox;
  p.scale_x_y = scale_x_y;
  op->set_head();
  kernels::hip::HipYoloHead hz;
  for (size_t i = 1; i < xs.size(); ++i) {
    op->add_scale(Var(xs[i]), anchors[i]);
    hz.more.push_back({Var(xs[i]), anchors[i], downsample_ratios[i]});
  }
  kernels::hip::HipYoloHeadKernel* hk;
  auto kernel = PickAs("yolo_box", Place(TARGET(kHIP), PRECISION(kFloat)), "head", &hk);
  hk->SetYoloHead(hz);
  Emit(op, std::move(kernel));
}

void HipPredictor::AddConcatNhwc(const std::vector<std::string>& inputs, const std::string& out, int k) {
  CHECK(k > 0) << "AddConcatNhwc: k " << k;
  auto op = std::make_shared<operators::ConcatOpLite>();
  auto& p = op->mutable_param();
  for (auto& in : inputs) p.x.push_back(Var(in));
  p.output = Var(out);
  p.axis = 1;
  op->set_nhwc_k(k);
  Emit(op, PickKernel("concat", Place(TARGET(kHIP), PRECISION(kFloat), DATALAYOUT(kNHWC)), "nhwc"));
}

std::vector<std::string> HipPredictor::KernelNames() {
  std::vector<std::string> r;
  for (auto& i : program_.instructions())
    r.push_back(i.kernel()->name() + "/" + i.kernel()->alias() + " -> " + i.kernel()->kernel_func_name());
  return r;
}

// Everything a recorded launch graph has baked in: the shape of every variable (grid sizes, strides) and the address of every device
// variable (Buffer::ResetLazy grows only: a feed resized up and back leaves the old shapes at new addresses), the instruction list
// and the workspace arena (its address is a kernel argument; HipExecState::Workspace frees the arena when it grows).
size_t HipPredictor::GraphKey() const {
  size_t h = 1469598103934665603ULL;
  auto mix = [&h](size_t v) { h = (h ^ v) * 1099511628211ULL; };
  mix(const_cast<HipPredictor*>(this)->program_.instructions().size());
  mix(reinterpret_cast<size_t>(state_->workspace_ptr()));
  mix(state_->workspace_bytes());
  for (auto& kv : vars_) {
    const auto d = kv.second->dims();
    mix(d.size());
    for (size_t i = 0; i < d.size(); ++i) mix(static_cast<size_t>(d[i]));
    if (kv.second->target() == TARGET(kHIP)) mix(reinterpret_cast<size_t>(kv.second->raw_data()));
  }
  return h;
}

void HipPredictor::RunGraph() {
  TargetWrapperHip::SetDevice(device_);
  plhip_ctx* ctx = state()->ctx();
  // a feed resized, an instruction added or the arena re-allocated since the recording: the graph is stale (it would read
  // freed memory / use old shapes): drop it and record again
  if (graph_exec_ && (graph_stale_ || graph_key_ != GraphKey())) {
    (void)plhip_graph_destroy(ctx, graph_exec_);
    graph_exec_ = nullptr;
  }
  if (!graph_exec_) {
    // one ordinary run first: PrepareForRun (allocations, weight packing, host syncs) must not happen inside a capture,
    // and it brings the workspace arena to its final size
    program_.Run(/*skip_io_copy=*/true);
    state()->Sync();
    HIP_CALL(ctx, plhip_graph_begin(ctx));
    try {
      program_.Run(/*skip_io_copy=*/true);  // InferShape() + Launch() per instruction, recorded instead of executed
    } catch (...) {
      void* dead = nullptr;  // never leave the stream in capture mode: end it, discard whatever was recorded, re-throw
      if (plhip_graph_end(ctx, &dead) == PLHIP_OK && dead) (void)plhip_graph_destroy(ctx, dead);
      throw;
    }
    HIP_CALL(ctx, plhip_graph_end(ctx, &graph_exec_));
    graph_key_ = GraphKey();
    graph_stale_ = false;
  }
  HIP_CALL(ctx, plhip_graph_launch(ctx, graph_exec_));
}

HipPredictor::~HipPredictor() {
  if (graph_exec_ && state_) (void)plhip_graph_destroy(state_->ctx(), graph_exec_);
}

}  // namespace lite
}  // namespace paddle
