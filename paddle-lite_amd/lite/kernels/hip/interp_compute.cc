// interp_compute.cc — dense prediction on kHIP:
//   bilinear_interp  lite/kernels/arm/interpolate_compute.cc -> lite/backends/arm/math/interpolate.cc:65-463
//   nearest_interp   ... -> interpolate.cc:465-499
//   arg_max          lite/kernels/arm/argmax_compute.cc -> lite/backends/arm/math/argmax.cc:29-61
// Alias def: the reference's op.  bilinear_interp / nearest_interp alias int8: the product of the graph builder's fusion N, the
// calib[fp32_to_int8] behind the interp written in the same launch (calib_tail.h).  It reads fp32 and writes int8 (and fp32
// where that still has a reader), so it is registered at kAny precision: the def alias stays the one kernel a pick at kFloat finds.
// arg_max alias interp: the product of fusion M, interp -> arg_max(axis 1) in one launch (interp_fusion.h); X is the low-resolution tensor.
// The output size comes from the attributes (out_h / out_w, or scale > 0 as int(in * scale)); OutSize, SizeTensor and Scale
// tensors and a layout other than NCHW are fatal in PrepareForRun.  Every class reads its dims in Run: a resized feed needs no
// new lowering.
#include <string>

#include "lite/core/op_registry.h"
#include "lite/kernels/hip/calib_tail.h"
#include "lite/kernels/hip/interp_fusion.h"
#include "lite/operators/op_params.h"
#include "plhip.h"

namespace paddle {
namespace lite {
namespace kernels {
namespace hip {

// what plhip_interp_f32 takes of an interp op, from its type and attributes
struct InterpCall {
  int n, c, in_h, in_w, out_h, out_w, method;
};

static void CheckInterpAttrs(const operators::InterpolateParam& p, const std::string& who) {
  CHECK(p.OutSize == nullptr && p.SizeTensor.empty() && p.Scale == nullptr)
      << who << ": kHIP takes the output size from out_h / out_w / scale; OutSize, SizeTensor and Scale tensors are not supported";
  CHECK(p.data_layout == DATALAYOUT(kNCHW)) << who << ": NCHW only";
  CHECK(p.align_mode == 0 || p.align_mode == 1) << who << ": align_mode " << p.align_mode;
  CHECK((p.out_h > 0 && p.out_w > 0) || p.scale > 0.f) << who << ": neither out_h / out_w nor a scale > 0";
}

static InterpCall MakeInterpCall(const std::string& op_type, const operators::InterpolateParam& p, const DDim& x, const std::string& who) {
  CHECK_EQ(x.size(), 4UL) << who << ": X must be [N, C, H, W]";
  const int64_t cap = int64_t{1} << 15;
  CHECK(x[0] >= 1 && x[1] >= 1 && x[0] < (int64_t{1} << 31) && x[1] <= cap && x[2] >= 1 && x[2] <= cap && x[3] >= 1 && x[3] <= cap)
      << who << ": X dims " << x << " outside what kHIP takes";
  InterpCall k;
  k.n = static_cast<int>(x[0]);
  k.c = static_cast<int>(x[1]);
  k.in_h = static_cast<int>(x[2]);
  k.in_w = static_cast<int>(x[3]);
  if (p.out_h > 0 && p.out_w > 0) {
    k.out_h = p.out_h;
    k.out_w = p.out_w;
  } else {  // interpolate_op.cc:76-77
    k.out_h = static_cast<int>(k.in_h * p.scale);
    k.out_w = static_cast<int>(k.in_w * p.scale);
  }
  k.method = op_type == "bilinear_interp" ? PLHIP_INTERP_BILINEAR : PLHIP_INTERP_NEAREST;
  return k;
}

class InterpCompute : public KernelLite<TARGET(kHIP), PRECISION(kFloat)> {
 public:
  void PrepareForRun() override { CheckInterpAttrs(this->Param<operators::InterpolateParam>(), op_type()); }
  void Run() override {
    auto& param = this->Param<operators::InterpolateParam>();
    auto& ctx = this->ctx_->As<HIPContext>();
    CHECK(param.X && param.Out) << op_type() << ": X / Out must be set";
    CHECK(param.X->target() == TARGET(kHIP)) << op_type() << ": X must live on the HIP device";
    const InterpCall k = MakeInterpCall(op_type(), param, param.X->dims(), op_type());
    HIP_CALL(ctx.ctx(), plhip_interp_f32(ctx.ctx(), param.X->data<float>(), static_cast<int64_t>(k.n) * k.c, k.in_h, k.in_w, k.out_h, k.out_w,
                                         k.method, param.align_corners ? 1 : 0, param.align_mode,
                                         param.Out->mutable_data<float>(TARGET(kHIP)), nullptr, 1.f));
  }
  void SetProfileRuntimeKernelInfo(profile::OpCharacter* ch) override { ch->kernel_func_name = op_type() + "_hip"; }
};

// interp that took the calib[fp32_to_int8] behind it over (fusion N): one launch of plhip_interp_f32 with the int8 output
class InterpCalibCompute : public KernelLite<TARGET(kHIP), PRECISION(kAny)>, public HipCalibTailKernel {
 public:
  void SetCalibTail(const HipCalibTail& t) override { tail_ = t; }
  void PrepareForRun() override { CheckInterpAttrs(this->Param<operators::InterpolateParam>(), op_type() + "/int8"); }
  void Run() override {
    auto& param = this->Param<operators::InterpolateParam>();
    auto& ctx = this->ctx_->As<HIPContext>();
    const std::string who = op_type() + "/int8";
    CHECK(param.X && param.Out) << who << ": X / Out must be set";
    CHECK(tail_.calib_output) << who << " needs the calib tail the graph builder attaches (calib_tail.h)";
    CHECK(param.X->target() == TARGET(kHIP)) << who << ": X must live on the HIP device";
    const InterpCall k = MakeInterpCall(op_type(), param, param.X->dims(), who);
    const TailOutputs o = OutputsOf(tail_, true, param.Out);
    HIP_CALL(ctx.ctx(), plhip_interp_f32(ctx.ctx(), param.X->data<float>(), static_cast<int64_t>(k.n) * k.c, k.in_h, k.in_w, k.out_h, k.out_w,
                                         k.method, param.align_corners ? 1 : 0, param.align_mode, o.f32, o.i8, o.scale));
  }
  void SetProfileRuntimeKernelInfo(profile::OpCharacter* ch) override { ch->kernel_func_name = op_type() + TailSuffix(tail_, true) + "_hip"; }

 private:
  HipCalibTail tail_;
};

static void CheckArgmaxDtype(int dtype, const std::string& who) {
  CHECK(dtype == -1 || dtype == 2 || dtype == 3) << who << ": dtype " << dtype << " is neither int64 (-1, 3) nor int32 (2)";
}

class ArgmaxCompute : public KernelLite<TARGET(kHIP), PRECISION(kAny)> {
 public:
  void PrepareForRun() override { CheckArgmaxDtype(this->Param<operators::ArgmaxParam>().dtype, "arg_max"); }
  void Run() override {
    auto& param = this->Param<operators::ArgmaxParam>();
    auto& ctx = this->ctx_->As<HIPContext>();
    CHECK(param.X && param.Out) << "arg_max: X / Out must be set";
    CHECK(param.X->target() == TARGET(kHIP)) << "arg_max: X must live on the HIP device";
    const DDim& d = param.X->dims();
    const int rank = static_cast<int>(d.size());
    const int axis = param.Axis < 0 ? param.Axis + rank : param.Axis;
    CHECK(axis >= 0 && axis < rank) << "arg_max: axis " << param.Axis << " outside the rank " << rank;
    CHECK(d[axis] >= 1 && d[axis] <= (int64_t{1} << 15)) << "arg_max: the axis has " << d[axis] << " entries";
    void* y = param.dtype == 2 ? static_cast<void*>(param.Out->mutable_data<int32_t>(TARGET(kHIP)))
                               : static_cast<void*>(param.Out->mutable_data<int64_t>(TARGET(kHIP)));
    HIP_CALL(ctx.ctx(), plhip_arg_max_f32(ctx.ctx(), param.X->data<float>(), d.count(0, axis), static_cast<int>(d[axis]),
                                          d.count(axis + 1, rank), y, param.dtype));
  }
  void SetProfileRuntimeKernelInfo(profile::OpCharacter* ch) override { ch->kernel_func_name = "arg_max_hip"; }
};

// arg_max(axis 1) that took the interp in front of it over (fusion M): one launch of plhip_interp_argmax_f32 on the interp's input
class InterpArgmaxCompute : public KernelLite<TARGET(kHIP), PRECISION(kAny)>, public HipInterpArgmaxKernel {
 public:
  void SetInterpArgmax(const HipInterpArgmaxFusion& f) override { fusion_ = f; }
  void PrepareForRun() override {
    CHECK(fusion_.op_type == "bilinear_interp" || fusion_.op_type == "nearest_interp")
        << "arg_max/interp needs the fusion state the graph builder attaches (interp_fusion.h)";
    CheckInterpAttrs(fusion_.interp, "arg_max/interp");
    auto& param = this->Param<operators::ArgmaxParam>();
    CheckArgmaxDtype(param.dtype, "arg_max/interp");
    CHECK(param.Axis == 1 || param.Axis == -3) << "arg_max/interp: axis 1 only";
  }
  void Run() override {
    auto& param = this->Param<operators::ArgmaxParam>();
    auto& ctx = this->ctx_->As<HIPContext>();
    CHECK(param.X && param.Out) << "arg_max/interp: X / Out must be set";
    CHECK(param.X->target() == TARGET(kHIP)) << "arg_max/interp: X must live on the HIP device";
    const InterpCall k = MakeInterpCall(fusion_.op_type, fusion_.interp, param.X->dims(), "arg_max/interp");
    void* y = param.dtype == 2 ? static_cast<void*>(param.Out->mutable_data<int32_t>(TARGET(kHIP)))
                               : static_cast<void*>(param.Out->mutable_data<int64_t>(TARGET(kHIP)));
    HIP_CALL(ctx.ctx(), plhip_interp_argmax_f32(ctx.ctx(), param.X->data<float>(), k.n, k.c, k.in_h, k.in_w, k.out_h, k.out_w, k.method,
                                                fusion_.interp.align_corners ? 1 : 0, fusion_.interp.align_mode, y, param.dtype));
  }
  void SetProfileRuntimeKernelInfo(profile::OpCharacter* ch) override { ch->kernel_func_name = fusion_.op_type + "_arg_max_hip"; }

 private:
  HipInterpArgmaxFusion fusion_;
};

}  // namespace hip
}  // namespace kernels
}  // namespace lite
}  // namespace paddle

REGISTER_LITE_KERNEL(bilinear_interp, kHIP, kFloat, kNCHW, paddle::lite::kernels::hip::InterpCompute, def)
    .BindInput("X", {LiteType::GetTensorTy(TARGET(kHIP))})
    .BindOutput("Out", {LiteType::GetTensorTy(TARGET(kHIP))})
    .Finalize();
REGISTER_LITE_KERNEL(nearest_interp, kHIP, kFloat, kNCHW, paddle::lite::kernels::hip::InterpCompute, def)
    .BindInput("X", {LiteType::GetTensorTy(TARGET(kHIP))})
    .BindOutput("Out", {LiteType::GetTensorTy(TARGET(kHIP))})
    .Finalize();
REGISTER_LITE_KERNEL(bilinear_interp, kHIP, kAny, kNCHW, paddle::lite::kernels::hip::InterpCalibCompute, int8)
    .BindInput("X", {LiteType::GetTensorTy(TARGET(kHIP))})
    .BindOutput("Out", {LiteType::GetTensorTy(TARGET(kHIP))})
    .Finalize();
REGISTER_LITE_KERNEL(nearest_interp, kHIP, kAny, kNCHW, paddle::lite::kernels::hip::InterpCalibCompute, int8)
    .BindInput("X", {LiteType::GetTensorTy(TARGET(kHIP))})
    .BindOutput("Out", {LiteType::GetTensorTy(TARGET(kHIP))})
    .Finalize();
REGISTER_LITE_KERNEL(arg_max, kHIP, kAny, kNCHW, paddle::lite::kernels::hip::ArgmaxCompute, def)
    .BindInput("X", {LiteType::GetTensorTy(TARGET(kHIP))})
    .BindOutput("Out", {LiteType::GetTensorTy(TARGET(kHIP), PRECISION(kAny))})
    .Finalize();
REGISTER_LITE_KERNEL(arg_max, kHIP, kAny, kNCHW, paddle::lite::kernels::hip::InterpArgmaxCompute, interp)
    .BindInput("X", {LiteType::GetTensorTy(TARGET(kHIP))})
    .BindOutput("Out", {LiteType::GetTensorTy(TARGET(kHIP), PRECISION(kAny))})
    .Finalize();
