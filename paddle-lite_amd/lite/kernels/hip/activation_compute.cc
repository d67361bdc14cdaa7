// activation_compute.cc — the fp32 ops MobileNetV3 adds to the int8 programs, on kHIP:
//   hard_swish       lite/kernels/arm/activation_compute.cc:150-195 (HardSwishCompute)
//   hard_sigmoid     lite/kernels/arm/activation_compute.cc:319-345 (HardSigmoidCompute)
//   elementwise_mul  lite/kernels/arm/elementwise_compute.cc:30-84 (the fast-broadcast case pre = 1, n = N * C, post = H * W:
//                    the gate of a squeeze-excite block), and same-shape operands
// Alias def: the reference's op.  Alias int8 (hard_swish, elementwise_mul): the product of the graph builder's fusions J1 / J3,
// the op with the calib[fp32_to_int8] behind it in the same launch (calib_tail.h), bit-identical to the two instructions.
// Alias se_gate (hard_sigmoid): fusion J2, the excite chain of a squeeze-excite block in one launch (se_gate_fusion.h).
#include "lite/core/op_registry.h"
#include "lite/kernels/hip/calib_tail.h"
#include "lite/kernels/hip/quant_fold.h"
#include "lite/kernels/hip/se_gate_fusion.h"
#include "lite/operators/op_params.h"
#include "plhip.h"

namespace paddle {
namespace lite {
namespace kernels {
namespace hip {

template <plhip_hard_act_kind Kind>
class HardActCompute : public KernelLite<TARGET(kHIP), PRECISION(kFloat)>, public HipCalibTailKernel {
 public:
  void SetCalibTail(const HipCalibTail& t) override { tail_ = t; }
  void Run() override {
    auto& param = this->Param<operators::ActivationParam>();
    auto& ctx = this->ctx_->As<HIPContext>();
    CHECK(param.X->target() == TARGET(kHIP)) << op_type() << ": X must live on the HIP device";
    const float swish[3] = {param.hard_swish_threshold, param.hard_swish_scale, param.hard_swish_offset};
    const float sigmoid[3] = {param.hard_sigmoid_slope, param.hard_sigmoid_offset, 0.f};
    const TailOutputs o = OutputsOf(tail_, alias() == "int8", param.Out);
    HIP_CALL(ctx.ctx(), plhip_hard_act_f32(ctx.ctx(), Kind, Kind == PLHIP_HARD_SWISH ? swish : sigmoid, param.X->data<float>(),
                                           o.f32, o.i8, o.scale, param.X->numel()));
  }
  void SetProfileRuntimeKernelInfo(profile::OpCharacter* ch) override {
    std::string name = Kind == PLHIP_HARD_SWISH ? "hard_swish" : "hard_sigmoid";
    ch->kernel_func_name = name + TailSuffix(tail_, alias() == "int8") + "_hip";
  }

 private:
  HipCalibTail tail_;
};

// hard_sigmoid that took calib -> conv 1x1 -> conv 1x1 in front of it over (J2): X is the pooled fp32 [N, C, 1, 1]
class SeGateCompute : public KernelLite<TARGET(kHIP), PRECISION(kFloat)>, public HipSeGateKernel {
 public:
  void SetSeGate(const HipSeGateFusion& f) override { fusion_ = f; }
  void PrepareForRun() override {
    CHECK(fusion_.reduce.filter && fusion_.expand.filter) << "hard_sigmoid/se_gate needs the fusion state the graph builder attaches";
    const auto w1 = fusion_.reduce.filter->dims(), w2 = fusion_.expand.filter->dims();
    CHECK(w1.size() == 4UL && w2.size() == 4UL && w1[2] == 1 && w1[3] == 1 && w2[2] == 1 && w2[3] == 1 && w2[1] == w1[0] && w2[0] == w1[1])
        << "se_gate: the two convs must be 1x1, C -> Cr -> C";
    desc_ = plhip_se_gate_desc{};
    desc_.c = static_cast<int>(w1[1]);
    desc_.cr = static_cast<int>(w1[0]);
    desc_.calib_scale = fusion_.calib_scale;
    // folded as two stand-alone conv2d (quant_fold.h): the reduce conv's int8 output scale is the expand conv's input scale
    const auto& r = fusion_.reduce;
    const auto& e = fusion_.expand;
    const QuantFold f1 = FoldLayer(r.weight_scale, desc_.cr, r.input_scale, e.input_scale, true, r.bias, &r.activation_param, false);
    const QuantFold f2 = FoldLayer(e.weight_scale, desc_.c, e.input_scale, 1.f, false, e.bias, &e.activation_param, false);
    desc_.act1 = f1.act; desc_.act1_alpha = f1.alpha;
    desc_.act2 = f2.act; desc_.act2_alpha = f2.alpha;
    has_b1_ = UploadFold(f1, &s1_, &b1_);
    has_b2_ = UploadFold(f2, &s2_, &b2_);
    if (!plhip_se_gate_supported(desc_.c, desc_.cr, desc_.act1, desc_.act2)) LOG(FATAL) << "se_gate: shape outside the fused kernel's envelope";
    auto& ctx = this->ctx_->As<HIPContext>();
    const size_t n1 = static_cast<size_t>(fusion_.reduce.filter->numel()), n2 = static_cast<size_t>(fusion_.expand.filter->numel());
    Tensor raw;
    raw.Resize({static_cast<int64_t>(n1 + n2)});
    int8_t* d = raw.mutable_data<int8_t>(TARGET(kHIP));
    TargetWrapperHip::MemcpySync(d, fusion_.reduce.filter->raw_data(), n1, IoDirection::HtoD);
    TargetWrapperHip::MemcpySync(d + n1, fusion_.expand.filter->raw_data(), n2, IoDirection::HtoD);
    packed_.Resize({static_cast<int64_t>(plhip_se_gate_packed_weight_bytes(desc_.c, desc_.cr))});
    HIP_CALL(ctx.ctx(), plhip_pack_se_gate_weights(ctx.ctx(), desc_.c, desc_.cr, d, d + n1, packed_.mutable_data<int8_t>(TARGET(kHIP))));
    HIP_CALL(ctx.ctx(), plhip_stream_sync(ctx.ctx()));  // `raw` goes away with this scope
  }
  void Run() override {
    auto& param = this->Param<operators::ActivationParam>();
    auto& ctx = this->ctx_->As<HIPContext>();
    const auto d = param.X->dims();
    CHECK(d.size() >= 2UL && d[1] == desc_.c && param.X->numel() == d[0] * d[1]) << "se_gate: X must be the pooled [N, C, 1, 1]";
    desc_.n = static_cast<int>(d[0]);
    desc_.slope = param.hard_sigmoid_slope;
    desc_.offset = param.hard_sigmoid_offset;
    HIP_CALL(ctx.ctx(), plhip_se_gate_int8(ctx.ctx(), &desc_, param.X->data<float>(), packed_.raw_data(), s1_.data<float>(),
                                           has_b1_ ? b1_.data<float>() : nullptr, s2_.data<float>(), has_b2_ ? b2_.data<float>() : nullptr,
                                           param.Out->mutable_data<float>(TARGET(kHIP))));
  }
  void SetProfileRuntimeKernelInfo(profile::OpCharacter* ch) override { ch->kernel_func_name = "se_gate_int8_dot4_hip"; }

 private:
  HipSeGateFusion fusion_;
  plhip_se_gate_desc desc_{};
  Tensor s1_, b1_, s2_, b2_, packed_;
  bool has_b1_{false}, has_b2_{false};
};

class ElementwiseMulCompute : public KernelLite<TARGET(kHIP), PRECISION(kFloat)>, public HipCalibTailKernel {
 public:
  void SetCalibTail(const HipCalibTail& t) override { tail_ = t; }
  // X [N, C, H, W] with Y [N, C, 1, 1] or [N, C] at axis 0 (pre = 1, n = N * C, post = H * W), or equal shapes
  void PrepareForRun() override {
    auto& param = this->Param<operators::ElementwiseParam>();
    const auto x = param.X->dims(), y = param.Y->dims();
    if (x == y) return;
    bool ok = x.size() == 4 && (y.size() == 4 || y.size() == 2) && (param.axis == 0 || (param.axis == -1 && y.size() == 4)) &&
              y[0] == x[0] && y[1] == x[1];
    if (ok && y.size() == 4) ok = y[2] == 1 && y[3] == 1;
    if (!ok) LOG(FATAL) << "kHIP elementwise_mul: unsupported broadcast (Y must be X's shape, or [N, C, 1, 1] / [N, C] at axis 0)";
  }
  void Run() override {
    auto& param = this->Param<operators::ElementwiseParam>();
    auto& ctx = this->ctx_->As<HIPContext>();
    CHECK(param.X->target() == TARGET(kHIP) && param.Y->target() == TARGET(kHIP));
    const auto x = param.X->dims();
    const bool same = x == param.Y->dims();
    const TailOutputs o = OutputsOf(tail_, alias() == "int8", param.Out);
    // equal shapes: every element is its own plane
    const int64_t planes = same ? param.X->numel() : x[0] * x[1];
    CHECK_LT(planes, int64_t{1} << 30) << "kHIP elementwise_mul: tensor too large";
    HIP_CALL(ctx.ctx(), plhip_se_scale_f32(ctx.ctx(), param.X->data<float>(), param.Y->data<float>(), 1, static_cast<int>(planes),
                                           same ? 1 : static_cast<int>(x[2] * x[3]), o.f32, o.i8, o.scale));
  }
  void SetProfileRuntimeKernelInfo(profile::OpCharacter* ch) override {
    ch->kernel_func_name = std::string("se_scale") + TailSuffix(tail_, alias() == "int8") + "_hip";
  }

 private:
  HipCalibTail tail_;
};

}  // namespace hip
}  // namespace kernels
}  // namespace lite
}  // namespace paddle

using HardSwishHip = paddle::lite::kernels::hip::HardActCompute<PLHIP_HARD_SWISH>;
using HardSigmoidHip = paddle::lite::kernels::hip::HardActCompute<PLHIP_HARD_SIGMOID>;
REGISTER_LITE_KERNEL(hard_swish, kHIP, kFloat, kNCHW, HardSwishHip, def)
    .BindInput("X", {LiteType::GetTensorTy(TARGET(kHIP))})
    .BindOutput("Out", {LiteType::GetTensorTy(TARGET(kHIP))})
    .Finalize();
REGISTER_LITE_KERNEL(hard_swish, kHIP, kFloat, kNCHW, HardSwishHip, int8)
    .BindInput("X", {LiteType::GetTensorTy(TARGET(kHIP))})
    .BindOutput("Out", {LiteType::GetTensorTy(TARGET(kHIP))})
    .Finalize();
REGISTER_LITE_KERNEL(hard_sigmoid, kHIP, kFloat, kNCHW, HardSigmoidHip, def)
    .BindInput("X", {LiteType::GetTensorTy(TARGET(kHIP))})
    .BindOutput("Out", {LiteType::GetTensorTy(TARGET(kHIP))})
    .Finalize();
REGISTER_LITE_KERNEL(hard_sigmoid, kHIP, kFloat, kNCHW, paddle::lite::kernels::hip::SeGateCompute, se_gate)
    .BindInput("X", {LiteType::GetTensorTy(TARGET(kHIP))})
    .BindOutput("Out", {LiteType::GetTensorTy(TARGET(kHIP))})
    .Finalize();
REGISTER_LITE_KERNEL(elementwise_mul, kHIP, kFloat, kNCHW, paddle::lite::kernels::hip::ElementwiseMulCompute, def)
    .BindInput("X", {LiteType::GetTensorTy(TARGET(kHIP))})
    .BindInput("Y", {LiteType::GetTensorTy(TARGET(kHIP))})
    .BindOutput("Out", {LiteType::GetTensorTy(TARGET(kHIP))})
    .Finalize();
REGISTER_LITE_KERNEL(elementwise_mul, kHIP, kFloat, kNCHW, paddle::lite::kernels::hip::ElementwiseMulCompute, int8)
    .BindInput("X", {LiteType::GetTensorTy(TARGET(kHIP))})
    .BindInput("Y", {LiteType::GetTensorTy(TARGET(kHIP))})
    .BindOutput("Out", {LiteType::GetTensorTy(TARGET(kHIP))})
    .Finalize();
