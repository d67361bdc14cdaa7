// shuffle_compute.cc — the fp32 ops that join, part and permute tensors along an axis, on kHIP:
//   concat           lite/kernels/arm/concat_compute.cc:37-57 (ConcatCompute)
//   split            lite/kernels/arm/split_compute.cc -> lite/backends/arm/math/split.cc:54-82
//   shuffle_channel  lite/kernels/arm/shuffle_channel_compute.cc -> lite/backends/arm/math/shuffle_channel.cc:24-55
// Alias def: the reference's op.  Aliases int8 / unit (shuffle_channel): the products of the graph builder's fusion K, the
// tail of a ShuffleNetV2 unit in one launch (shuffle_fusion.h), bit-identical to the instructions they replace.
// concat, alias int8: the product of fusion L, concat -> calib[fp32_to_int8] in one launch (calib_tail.h).  It reads fp32 and
// writes int8 (and fp32 where that still has a reader), so it is registered at kAny precision: concat/def stays the one kernel a
// pick at kFloat finds.
// Every class reads its dims in Run: a resized feed needs no new lowering.
#include <vector>

#include "lite/core/op_registry.h"
#include "lite/kernels/hip/calib_tail.h"
#include "lite/kernels/hip/shuffle_fusion.h"
#include "lite/operators/op_params.h"
#include "plhip.h"

namespace paddle {
namespace lite {
namespace kernels {
namespace hip {

// outer = prod(dims[:axis]), inner = prod(dims[axis+1:]) of an op along `axis` (negative: from the back)
struct AxisSplit {
  int axis;
  int64_t outer, inner;
};
static AxisSplit SplitAtAxis(const DDim& d, int axis, const char* who) {
  const int rank = static_cast<int>(d.size());
  AxisSplit s;
  s.axis = axis < 0 ? axis + rank : axis;
  CHECK(s.axis >= 0 && s.axis < rank) << who << ": axis " << axis << " outside the rank " << rank;
  s.outer = d.count(0, s.axis);
  s.inner = d.count(s.axis + 1, rank);
  return s;
}

class ConcatCompute : public KernelLite<TARGET(kHIP), PRECISION(kFloat)> {
 public:
  void Run() override {
    auto& param = this->Param<operators::ConcatParam>();
    auto& ctx = this->ctx_->As<HIPContext>();
    CHECK(!param.x.empty() && param.output) << "concat: inputs / output must be set";
    const AxisSplit s = SplitAtAxis(param.x[0]->dims(), param.axis, "concat");
    std::vector<const float*> xs;
    std::vector<int64_t> extents;
    for (auto* t : param.x) {
      CHECK(t->target() == TARGET(kHIP)) << "concat: every input must live on the HIP device";
      xs.push_back(t->data<float>());
      extents.push_back(t->dims()[s.axis]);
    }
    HIP_CALL(ctx.ctx(), plhip_concat_f32(ctx.ctx(), xs.data(), extents.data(), static_cast<int>(xs.size()), s.outer, s.inner,
                                         param.output->mutable_data<float>(TARGET(kHIP))));
  }
  void SetProfileRuntimeKernelInfo(profile::OpCharacter* ch) override { ch->kernel_func_name = "concat_hip"; }
};

// concat that took the calib[fp32_to_int8] behind it over (fusion L): one launch of plhip_concat_calib_f32 per 8 operands
class ConcatCalibCompute : public KernelLite<TARGET(kHIP), PRECISION(kAny)>, public HipCalibTailKernel {
 public:
  void SetCalibTail(const HipCalibTail& t) override { tail_ = t; }
  void Run() override {
    auto& param = this->Param<operators::ConcatParam>();
    auto& ctx = this->ctx_->As<HIPContext>();
    CHECK(!param.x.empty() && param.output) << "concat/int8: inputs / output must be set";
    CHECK(tail_.calib_output) << "concat/int8 needs the calib tail the graph builder attaches (calib_tail.h)";
    const AxisSplit s = SplitAtAxis(param.x[0]->dims(), param.axis, "concat/int8");
    std::vector<const float*> xs;
    std::vector<int64_t> extents;
    for (auto* t : param.x) {
      CHECK(t->target() == TARGET(kHIP)) << "concat/int8: every input must live on the HIP device";
      xs.push_back(t->data<float>());
      extents.push_back(t->dims()[s.axis]);
    }
    const TailOutputs o = OutputsOf(tail_, true, param.output);
    HIP_CALL(ctx.ctx(), plhip_concat_calib_f32(ctx.ctx(), xs.data(), extents.data(), static_cast<int>(xs.size()), s.outer, s.inner, o.f32,
                                               o.i8, o.scale));
  }
  void SetProfileRuntimeKernelInfo(profile::OpCharacter* ch) override {
    ch->kernel_func_name = std::string("concat") + TailSuffix(tail_, true) + "_hip";
  }

 private:
  HipCalibTail tail_;
};

class SplitCompute : public KernelLite<TARGET(kHIP), PRECISION(kFloat)> {
 public:
  void Run() override {
    auto& param = this->Param<operators::SplitParam>();
    auto& ctx = this->ctx_->As<HIPContext>();
    CHECK(param.x && !param.output.empty()) << "split: x / outputs must be set";
    CHECK(param.x->target() == TARGET(kHIP)) << "split: x must live on the HIP device";
    const AxisSplit s = SplitAtAxis(param.x->dims(), param.axis, "split");
    std::vector<float*> ys;
    std::vector<int64_t> sections;
    for (auto* t : param.output) {  // the dims SplitOp::InferShapeImpl gave them (num or sections)
      sections.push_back(t->dims()[s.axis]);
      ys.push_back(t->mutable_data<float>(TARGET(kHIP)));
    }
    HIP_CALL(ctx.ctx(), plhip_split_f32(ctx.ctx(), param.x->data<float>(), s.outer, param.x->dims()[s.axis], s.inner, 0, sections.data(),
                                        static_cast<int>(ys.size()), ys.data()));
  }
  void SetProfileRuntimeKernelInfo(profile::OpCharacter* ch) override { ch->kernel_func_name = "split_hip"; }
};

// [N, C, hw] of an NCHW (or [N, C]) tensor
static void PlaneDims(const DDim& d, const char* who, int* n, int* c, int* hw) {
  CHECK_GE(d.size(), 2UL) << who << ": X must have at least two dims";
  const int64_t plane = d.count(2, static_cast<int>(d.size()));
  CHECK(d[0] < (int64_t{1} << 30) && d[1] < (int64_t{1} << 30) && plane < (int64_t{1} << 31)) << who << ": tensor too large";
  *n = static_cast<int>(d[0]);
  *c = static_cast<int>(d[1]);
  *hw = static_cast<int>(plane);
}

class ShuffleChannelCompute : public KernelLite<TARGET(kHIP), PRECISION(kFloat)> {
 public:
  void Run() override {
    auto& param = this->Param<operators::ShuffleChannelParam>();
    auto& ctx = this->ctx_->As<HIPContext>();
    CHECK(param.X->target() == TARGET(kHIP)) << "shuffle_channel: X must live on the HIP device";
    int n, c, hw;
    PlaneDims(param.X->dims(), "shuffle_channel", &n, &c, &hw);
    CHECK(param.group >= 1 && c % param.group == 0) << "shuffle_channel: group " << param.group << " does not divide C = " << c;
    HIP_CALL(ctx.ctx(), plhip_shuffle_channel_f32(ctx.ctx(), param.X->data<float>(), n, c, hw, param.group,
                                                  param.Out->mutable_data<float>(TARGET(kHIP)), nullptr, 1.f));
  }
  void SetProfileRuntimeKernelInfo(profile::OpCharacter* ch) override { ch->kernel_func_name = "shuffle_channel_hip"; }
};

// shuffle_channel(group 2) that took the two-input concat in front over, and behind it the calib (alias int8, K2) or the split in
// two halves with the calib of its second output (alias unit, K1): one launch of plhip_shuffle_unit_f32
class ShuffleTailCompute : public KernelLite<TARGET(kHIP), PRECISION(kFloat)>, public HipShuffleFusionKernel {
 public:
  void SetShuffleFusion(const HipShuffleFusion& f) override { fusion_ = f; }
  void Run() override {
    auto& param = this->Param<operators::ShuffleChannelParam>();
    auto& ctx = this->ctx_->As<HIPContext>();
    const bool unit = alias() == "unit";
    CHECK(fusion_.second) << "shuffle_channel/" << alias() << " needs the fusion state the graph builder attaches (shuffle_fusion.h)";
    CHECK(param.group == 2) << "shuffle_channel/" << alias() << ": group 2 only";
    CHECK(param.X->target() == TARGET(kHIP) && fusion_.second->target() == TARGET(kHIP)) << "shuffle_channel: operands must live on the HIP device";
    CHECK(param.X->dims() == fusion_.second->dims()) << "shuffle_channel/" << alias() << ": the two operands must have one shape";
    int n, h, hw;
    PlaneDims(param.X->dims(), "shuffle_channel", &n, &h, &hw);
    float* lo = nullptr;
    lite::Tensor* hi_t = unit ? fusion_.hi_output : param.Out;  // the fp32 tensor the calib read
    if (unit) {
      CHECK(hi_t) << "shuffle_channel/unit: the split's second output must be set";
      hi_t->Resize(param.X->dims());
      lo = param.Out->mutable_data<float>(TARGET(kHIP));
    }
    const TailOutputs o = OutputsOf(fusion_.tail, fusion_.tail.calib_output != nullptr, hi_t);
    HIP_CALL(ctx.ctx(), plhip_shuffle_unit_f32(ctx.ctx(), param.X->data<float>(), fusion_.second->data<float>(), n, h, hw, unit ? h : 0, lo,
                                               o.f32, o.i8, o.scale));
  }
  void SetProfileRuntimeKernelInfo(profile::OpCharacter* ch) override {
    ch->kernel_func_name = std::string(alias() == "unit" ? "shuffle_unit" : "shuffle_concat") +
                           TailSuffix(fusion_.tail, fusion_.tail.calib_output != nullptr) + "_hip";
  }

 private:
  HipShuffleFusion fusion_;
};

}  // namespace hip
}  // namespace kernels
}  // namespace lite
}  // namespace paddle

REGISTER_LITE_KERNEL(concat, kHIP, kFloat, kNCHW, paddle::lite::kernels::hip::ConcatCompute, def)
    .BindInput("X", {LiteType::GetTensorTy(TARGET(kHIP))})
    .BindOutput("Out", {LiteType::GetTensorTy(TARGET(kHIP))})
    .Finalize();
REGISTER_LITE_KERNEL(concat, kHIP, kAny, kNCHW, paddle::lite::kernels::hip::ConcatCalibCompute, int8)
    .BindInput("X", {LiteType::GetTensorTy(TARGET(kHIP))})
    .BindOutput("Out", {LiteType::GetTensorTy(TARGET(kHIP))})
    .Finalize();
REGISTER_LITE_KERNEL(split, kHIP, kFloat, kNCHW, paddle::lite::kernels::hip::SplitCompute, def)
    .BindInput("X", {LiteType::GetTensorTy(TARGET(kHIP))})
    .BindOutput("Out", {LiteType::GetTensorTy(TARGET(kHIP))})
    .Finalize();
REGISTER_LITE_KERNEL(shuffle_channel, kHIP, kFloat, kNCHW, paddle::lite::kernels::hip::ShuffleChannelCompute, def)
    .BindInput("X", {LiteType::GetTensorTy(TARGET(kHIP))})
    .BindOutput("Out", {LiteType::GetTensorTy(TARGET(kHIP))})
    .Finalize();
REGISTER_LITE_KERNEL(shuffle_channel, kHIP, kFloat, kNCHW, paddle::lite::kernels::hip::ShuffleTailCompute, int8)
    .BindInput("X", {LiteType::GetTensorTy(TARGET(kHIP))})
    .BindOutput("Out", {LiteType::GetTensorTy(TARGET(kHIP))})
    .Finalize();
REGISTER_LITE_KERNEL(shuffle_channel, kHIP, kFloat, kNCHW, paddle::lite::kernels::hip::ShuffleTailCompute, unit)
    .BindInput("X", {LiteType::GetTensorTy(TARGET(kHIP))})
    .BindOutput("Out", {LiteType::GetTensorTy(TARGET(kHIP))})
    .Finalize();
