// detection_compute.cc — detection heads on kHIP:
//   transpose / transpose2   lite/kernels/arm/transpose_compute.cc
//   reshape / reshape2       lite/kernels/host/reshape_compute.cc: the output shares the input's memory, no launch
//   prior_box                lite/kernels/arm/prior_box_compute.cc -> lite/backends/arm/math/prior_box.cc:330-
//   box_coder                lite/kernels/arm/box_coder_compute.cc:92-158 (decode_center_size)
//   multiclass_nms           lite/kernels/host/multiclass_nms_compute.cc:31-322, on the DEVICE: no copy to the host, no
//                            synchronisation, outputs of a fixed size (detection_fusion.h), so that the program can still be
//                            replayed as a launch graph
// prior_box depends on shapes and attributes only: it is computed on the host (prior_box_host.h) when the kernel first runs and
// again when a shape changes, uploaded once, and Run launches nothing otherwise.
// Every class reads its dims in Run: a resized feed needs no new lowering.
#include <string>
#include <vector>

#include "lite/core/op_registry.h"
#include "lite/kernels/hip/detection_fusion.h"
#include "lite/kernels/hip/prior_box_host.h"
#include "lite/operators/op_params.h"
#include "plhip.h"

namespace paddle {
namespace lite {
namespace kernels {
namespace hip {

class TransposeCompute : public KernelLite<TARGET(kHIP), PRECISION(kFloat)> {
 public:
  void Run() override {
    auto& param = this->Param<operators::TransposeParam>();
    auto& ctx = this->ctx_->As<HIPContext>();
    CHECK(param.x && param.output) << op_type() << ": x / output must be set";
    CHECK(param.x->target() == TARGET(kHIP)) << op_type() << ": x must live on the HIP device";
    const auto d = param.x->dims().Vectorize();
    CHECK(d.size() >= 2 && d.size() <= 4 && param.axis.size() == d.size()) << op_type() << ": rank " << d.size() << " with a perm of " << param.axis.size();
    HIP_CALL(ctx.ctx(), plhip_transpose_f32(ctx.ctx(), param.x->data<float>(), d.data(), param.axis.data(), static_cast<int>(d.size()),
                                            param.output->mutable_data<float>(TARGET(kHIP))));
  }
  void SetProfileRuntimeKernelInfo(profile::OpCharacter* ch) override { ch->kernel_func_name = "transpose_hip"; }
};

class ReshapeCompute : public KernelLite<TARGET(kHIP), PRECISION(kFloat)> {
 public:
  void Run() override {
    auto& param = this->Param<operators::ReshapeParam>();
    CHECK(param.x && param.output) << op_type() << ": x / output must be set";
    CHECK(param.shape_tensor_vct.empty() && !param.shape_tensor) << op_type() << ": kHIP takes the shape attribute only";
    const auto out_dims = param.output->dims();  // InferShape's
    param.output->ShareDataWith(*param.x);
    param.output->Resize(out_dims);
  }
  void SetProfileRuntimeKernelInfo(profile::OpCharacter* ch) override { ch->kernel_func_name = "reshape_share"; }
};

class PriorBoxCompute : public KernelLite<TARGET(kHIP), PRECISION(kFloat)> {
 public:
  void PrepareForRun() override { Compute(); }
  void Run() override {
    auto& param = this->Param<operators::PriorBoxParam>();
    if (param.input->dims().Vectorize() != in_dims_ || param.image->dims().Vectorize() != img_dims_) Compute();
  }
  void SetProfileRuntimeKernelInfo(profile::OpCharacter* ch) override { ch->kernel_func_name = "prior_box_host_once"; }

 private:
  void Compute() {
    auto& param = this->Param<operators::PriorBoxParam>();
    auto& ctx = this->ctx_->As<HIPContext>();
    CHECK(param.input && param.image && param.boxes && param.variances) << "prior_box: input / image / boxes / variances must be set";
    in_dims_ = param.input->dims().Vectorize();
    img_dims_ = param.image->dims().Vectorize();
    CHECK(in_dims_.size() == 4 && img_dims_.size() == 4) << "prior_box: Input and Image must be [N, C, H, W]";
    CHECK(!param.min_sizes.empty()) << "prior_box: min_sizes is empty";
    CHECK(param.max_sizes.empty() || param.max_sizes.size() == param.min_sizes.size()) << "prior_box: one max_size per min_size";
    CHECK_EQ(param.variances_.size(), 4UL) << "prior_box: four variances";
    const int img_h = param.img_w == 0 || param.img_h == 0 ? static_cast<int>(img_dims_[2]) : param.img_h;
    const int img_w = param.img_w == 0 || param.img_h == 0 ? static_cast<int>(img_dims_[3]) : param.img_w;
    std::vector<float> boxes, variances;
    PriorBoxHost(static_cast<int>(in_dims_[2]), static_cast<int>(in_dims_[3]), img_h, img_w, param.min_sizes, param.max_sizes,
                 param.aspect_ratios, param.flip, param.clip, param.variances_, param.step_w, param.step_h, param.offset,
                 param.min_max_aspect_ratios_order, &boxes, &variances);
    const int64_t num = static_cast<int64_t>(boxes.size()) / (4 * in_dims_[2] * in_dims_[3]);
    CHECK(param.prior_num == 0 || param.prior_num == num) << "prior_box: prior_num " << param.prior_num << " but the attributes give " << num;
    const std::vector<int64_t> out{in_dims_[2], in_dims_[3], num, 4};
    param.boxes->Resize(out);
    param.variances->Resize(out);
    const size_t bytes = boxes.size() * sizeof(float);
    ctx.MemcpySync(param.boxes->mutable_data<float>(TARGET(kHIP)), boxes.data(), bytes, IoDirection::HtoD);
    ctx.MemcpySync(param.variances->mutable_data<float>(TARGET(kHIP)), variances.data(), bytes, IoDirection::HtoD);
  }
  std::vector<int64_t> in_dims_, img_dims_;
};

class BoxCoderCompute : public KernelLite<TARGET(kHIP), PRECISION(kFloat)> {
 public:
  void PrepareForRun() override {
    auto& param = this->Param<operators::BoxCoderParam>();
    CHECK(param.code_type == "decode_center_size") << "box_coder: kHIP has decode_center_size only, not " << param.code_type;
    CHECK(param.variance.empty() || param.variance.size() == 4) << "box_coder: the variance attribute has " << param.variance.size() << " values";
  }
  void Run() override {
    auto& param = this->Param<operators::BoxCoderParam>();
    auto& ctx = this->ctx_->As<HIPContext>();
    CHECK(param.prior_box && param.target_box && param.proposals) << "box_coder: prior_box / target_box / proposals must be set";
    CHECK(param.prior_box->target() == TARGET(kHIP) && param.target_box->target() == TARGET(kHIP))
        << "box_coder: the inputs must live on the HIP device";
    const DDim& t = param.target_box->dims();
    CHECK(t.size() == 3 && t[2] == 4) << "box_coder: TargetBox must be [rows, cols, 4]";
    CHECK(param.axis == 0 || param.axis == 1) << "box_coder: axis " << param.axis;
    CHECK_EQ(param.prior_box->numel(), 4 * t[1 - param.axis]) << "box_coder: PriorBox does not hold one box per entry of axis " << param.axis;
    if (param.prior_box_var) CHECK_EQ(param.prior_box_var->numel(), param.prior_box->numel()) << "box_coder: PriorBoxVar must have PriorBox's dims";
    HIP_CALL(ctx.ctx(), plhip_box_coder_decode_f32(ctx.ctx(), param.prior_box->data<float>(),
                                                   param.prior_box_var ? param.prior_box_var->data<float>() : nullptr,
                                                   param.variance.empty() ? nullptr : param.variance.data(), param.target_box->data<float>(),
                                                   t[0], t[1], param.axis, param.box_normalized ? 1 : 0,
                                                   param.proposals->mutable_data<float>(TARGET(kHIP))));
  }
  void SetProfileRuntimeKernelInfo(profile::OpCharacter* ch) override { ch->kernel_func_name = "box_coder_decode_hip"; }
};

class MulticlassNmsCompute : public KernelLite<TARGET(kHIP), PRECISION(kFloat)>, public HipNmsFusionKernel {
 public:
  void SetNmsFusion(const HipNmsFusion& f) override { fusion_ = f; }
  void PrepareForRun() override {
    CHECK(fusion_.count) << "multiclass_nms needs the count tensor the predictor attaches (detection_fusion.h)";
  }
  void Run() override {
    auto& param = this->Param<operators::MulticlassNmsParam>();
    auto& ctx = this->ctx_->As<HIPContext>();
    CHECK(param.bboxes && param.scores && param.out) << "multiclass_nms: bboxes / scores / out must be set";
    CHECK(param.bboxes->target() == TARGET(kHIP) && param.scores->target() == TARGET(kHIP)) << "multiclass_nms: the inputs must live on the HIP device";
    const DDim& b = param.bboxes->dims();
    const DDim& s = param.scores->dims();
    CHECK(b.size() == 3 && b[2] == 4 && s.size() == 3) << "multiclass_nms: BBoxes [N, P, 4] and 3-D Scores";
    plhip_nms_desc d;
    d.n = static_cast<int>(b[0]);
    d.p = static_cast<int>(b[1]);
    d.c = static_cast<int>(s[fusion_.scores_npc ? 2 : 1]);
    CHECK(s[0] == b[0] && s[fusion_.scores_npc ? 1 : 2] == b[1]) << "multiclass_nms: BBoxes and Scores disagree in N or P";
    d.score_stride_class = fusion_.scores_npc ? 1 : d.p;
    d.score_stride_prior = fusion_.scores_npc ? d.c : 1;
    d.background_label = param.background_label;
    d.score_threshold = param.score_threshold;
    d.nms_top_k = param.nms_top_k;
    d.nms_threshold = param.nms_threshold;
    d.nms_eta = param.nms_eta;
    d.keep_top_k = param.keep_top_k;
    d.normalized = param.normalized ? 1 : 0;
    CHECK(param.keep_top_k > 0) << "multiclass_nms: keep_top_k " << param.keep_top_k << " must be positive on kHIP (it sizes the output)";
    param.out->Resize(std::vector<int64_t>{b[0], param.keep_top_k, 6});
    fusion_.count->Resize(std::vector<int64_t>{b[0]});
    int* index = nullptr;
    if (param.index) {
      param.index->Resize(std::vector<int64_t>{b[0], param.keep_top_k});
      index = param.index->mutable_data<int32_t>(TARGET(kHIP));
    }
    // 0 bytes: refused; the entry point then says why
    const size_t bytes = plhip_multiclass_nms_workspace_bytes(&d);
    HIP_CALL(ctx.ctx(), plhip_multiclass_nms_f32(ctx.ctx(), param.bboxes->data<float>(), param.scores->data<float>(), &d,
                                                 bytes ? ctx.workspace(bytes) : nullptr, param.out->mutable_data<float>(TARGET(kHIP)), index,
                                                 fusion_.count->mutable_data<int32_t>(TARGET(kHIP))));
  }
  void SetProfileRuntimeKernelInfo(profile::OpCharacter* ch) override {
    ch->kernel_func_name = fusion_.scores_npc ? "multiclass_nms_npc_hip" : "multiclass_nms_hip";
  }

 private:
  HipNmsFusion fusion_;
};

// concat that took the transpose(0,2,3,1) -> reshape([0,-1,k]) chain in front of every operand over (fusion O1): one launch of
// plhip_concat_nhwc_f32 per 8 operands reads the NCHW heads and writes the joined [N, P, k] tensor.  Registered at layout kNHWC
// (what it writes): concat/def stays the one kernel a pick at kNCHW finds.
class ConcatNhwcCompute : public KernelLite<TARGET(kHIP), PRECISION(kFloat), DATALAYOUT(kNHWC)> {
 public:
  void Run() override {
    auto& param = this->Param<operators::ConcatParam>();
    auto& ctx = this->ctx_->As<HIPContext>();
    CHECK(!param.x.empty() && param.output) << "concat/nhwc: inputs / output must be set";
    std::vector<const float*> xs;
    std::vector<int64_t> channels, hw;
    for (auto* t : param.x) {
      CHECK(t->target() == TARGET(kHIP)) << "concat/nhwc: every input must live on the HIP device";
      const DDim& d = t->dims();
      CHECK(d.size() == 4 && d[0] == param.x[0]->dims()[0]) << "concat/nhwc: every input must be [N, C, H, W] of one N";
      xs.push_back(t->data<float>());
      channels.push_back(d[1]);
      hw.push_back(d[2] * d[3]);
    }
    HIP_CALL(ctx.ctx(), plhip_concat_nhwc_f32(ctx.ctx(), xs.data(), channels.data(), hw.data(), static_cast<int>(xs.size()),
                                              param.x[0]->dims()[0], param.output->mutable_data<float>(TARGET(kHIP))));
  }
  void SetProfileRuntimeKernelInfo(profile::OpCharacter* ch) override { ch->kernel_func_name = "concat_nhwc_hip"; }
};

}  // namespace hip
}  // namespace kernels
}  // namespace lite
}  // namespace paddle

REGISTER_LITE_KERNEL(concat, kHIP, kFloat, kNHWC, paddle::lite::kernels::hip::ConcatNhwcCompute, nhwc)
    .BindInput("X", {LiteType::GetTensorTy(TARGET(kHIP))})
    .BindOutput("Out", {LiteType::GetTensorTy(TARGET(kHIP))})
    .Finalize();
REGISTER_LITE_KERNEL(transpose, kHIP, kFloat, kNCHW, paddle::lite::kernels::hip::TransposeCompute, def)
    .BindInput("X", {LiteType::GetTensorTy(TARGET(kHIP))})
    .BindOutput("Out", {LiteType::GetTensorTy(TARGET(kHIP))})
    .Finalize();
REGISTER_LITE_KERNEL(transpose2, kHIP, kFloat, kNCHW, paddle::lite::kernels::hip::TransposeCompute, def)
    .BindInput("X", {LiteType::GetTensorTy(TARGET(kHIP))})
    .BindOutput("Out", {LiteType::GetTensorTy(TARGET(kHIP))})
    .BindOutput("XShape", {LiteType::GetTensorTy(TARGET(kHIP))})
    .Finalize();
REGISTER_LITE_KERNEL(reshape, kHIP, kFloat, kNCHW, paddle::lite::kernels::hip::ReshapeCompute, def)
    .BindInput("X", {LiteType::GetTensorTy(TARGET(kHIP))})
    .BindOutput("Out", {LiteType::GetTensorTy(TARGET(kHIP))})
    .Finalize();
REGISTER_LITE_KERNEL(reshape2, kHIP, kFloat, kNCHW, paddle::lite::kernels::hip::ReshapeCompute, def)
    .BindInput("X", {LiteType::GetTensorTy(TARGET(kHIP))})
    .BindOutput("Out", {LiteType::GetTensorTy(TARGET(kHIP))})
    .BindOutput("XShape", {LiteType::GetTensorTy(TARGET(kHIP))})
    .Finalize();
REGISTER_LITE_KERNEL(prior_box, kHIP, kFloat, kNCHW, paddle::lite::kernels::hip::PriorBoxCompute, def)
    .BindInput("Input", {LiteType::GetTensorTy(TARGET(kHIP))})
    .BindInput("Image", {LiteType::GetTensorTy(TARGET(kHIP))})
    .BindOutput("Boxes", {LiteType::GetTensorTy(TARGET(kHIP))})
    .BindOutput("Variances", {LiteType::GetTensorTy(TARGET(kHIP))})
    .Finalize();
REGISTER_LITE_KERNEL(box_coder, kHIP, kFloat, kNCHW, paddle::lite::kernels::hip::BoxCoderCompute, def)
    .BindInput("PriorBox", {LiteType::GetTensorTy(TARGET(kHIP))})
    .BindInput("PriorBoxVar", {LiteType::GetTensorTy(TARGET(kHIP))})
    .BindInput("TargetBox", {LiteType::GetTensorTy(TARGET(kHIP))})
    .BindOutput("OutputBox", {LiteType::GetTensorTy(TARGET(kHIP))})
    .Finalize();
REGISTER_LITE_KERNEL(multiclass_nms, kHIP, kFloat, kNCHW, paddle::lite::kernels::hip::MulticlassNmsCompute, def)
    .BindInput("BBoxes", {LiteType::GetTensorTy(TARGET(kHIP))})
    .BindInput("Scores", {LiteType::GetTensorTy(TARGET(kHIP))})
    .BindOutput("Out", {LiteType::GetTensorTy(TARGET(kHIP))})
    .BindOutput("Index", {LiteType::GetTensorTy(TARGET(kHIP), PRECISION(kAny))})
    .Finalize();
