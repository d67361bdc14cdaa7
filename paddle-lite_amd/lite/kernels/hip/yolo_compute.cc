// yolo_compute.cc — the kHIP kernel classes of a YOLOv3 head: yolo_box, and the one-launch head of graph-level fusion P.
//
// Replaces (reference, ARM):
//   yolo_box        lite/kernels/arm/yolo_box_compute.cc:25-51 -> lite/backends/arm/math/yolo_box.cc:97-178
//   yolo_box/head   that kernel per feature map -> ConcatCompute (Boxes) -> ConcatCompute (Scores) -> TransposeCompute (0,2,1)
// ImgSize is bound at PRECISION(kInt32): an int32 [N, 2] tensor on the device.  The reference clears Boxes and Scores before the
// call; the device kernels write every element, so nothing is cleared here.  A missing or refused device kernel is fatal.
#include <vector>

#include "lite/core/kernel.h"
#include "lite/core/op_registry.h"
#include "lite/kernels/hip/yolo_fusion.h"
#include "lite/operators/op_params.h"
#include "plhip.h"

namespace paddle {
namespace lite {
namespace kernels {
namespace hip {

namespace {

void CheckOperands(const operators::YoloBoxParam& param, const char* who) {
  CHECK(param.X && param.ImgSize && param.Boxes && param.Scores) << who << ": X / ImgSize / Boxes / Scores must be set";
  CHECK(param.X->target() == TARGET(kHIP) && param.ImgSize->target() == TARGET(kHIP)) << who << ": the inputs must live on the HIP device";
  CHECK(param.ImgSize->precision() == PRECISION(kInt32)) << who << ": ImgSize must be an int32 tensor";
  CHECK(param.X->dims().size() == 4) << who << ": X must be [N, C, H, W]";
}

}  // namespace

class YoloBoxCompute : public KernelLite<TARGET(kHIP), PRECISION(kFloat)> {
 public:
  void Run() override {
    auto& param = this->Param<operators::YoloBoxParam>();
    auto& ctx = this->ctx_->As<HIPContext>();
    CheckOperands(param, "yolo_box");
    const DDim& d = param.X->dims();
    CHECK(param.anchors.size() >= 2 && param.anchors.size() % 2 == 0) << "yolo_box: anchors must hold (width, height) pairs";
    const int an = static_cast<int>(param.anchors.size() / 2);
    CHECK_EQ(d[1], static_cast<int64_t>(an) * (5 + param.class_num)) << "yolo_box: X's channels are not an * (5 + class_num)";
    HIP_CALL(ctx.ctx(), plhip_yolo_box_f32(ctx.ctx(), param.X->data<float>(), param.ImgSize->data<int>(), static_cast<int>(d[0]), an,
                                           param.class_num, static_cast<int>(d[2]), static_cast<int>(d[3]), param.anchors.data(),
                                           param.conf_thresh, param.downsample_ratio, param.clip_bbox ? 1 : 0, param.scale_x_y,
                                           param.Boxes->mutable_data<float>(TARGET(kHIP)), param.Scores->mutable_data<float>(TARGET(kHIP))));
  }
  void SetProfileRuntimeKernelInfo(profile::OpCharacter* ch) override { ch->kernel_func_name = "yolo_box_hip"; }
};

// fusion P: Param().X with its anchors and downsample_ratio is the first feature map, head_.more the ones behind it
class YoloHeadCompute : public KernelLite<TARGET(kHIP), PRECISION(kFloat)>, public HipYoloHeadKernel {
 public:
  void SetYoloHead(const HipYoloHead& h) override { head_ = h; }
  void Run() override {
    auto& param = this->Param<operators::YoloBoxParam>();
    auto& ctx = this->ctx_->As<HIPContext>();
    CheckOperands(param, "yolo_box/head");
    std::vector<const float*> xs{param.X->data<float>()};
    std::vector<int> hs{static_cast<int>(param.X->dims()[2])}, ws{static_cast<int>(param.X->dims()[3])};
    std::vector<const int*> anchors{param.anchors.data()};
    std::vector<int> lens{static_cast<int>(param.anchors.size())}, ratios{param.downsample_ratio};
    for (auto& m : head_.more) {
      CHECK(m.x && m.x->target() == TARGET(kHIP) && m.x->dims().size() == 4 && m.x->dims()[0] == param.X->dims()[0])
          << "yolo_box/head: every feature map must be [N, C, H, W] of the first one's N on the HIP device";
      xs.push_back(m.x->data<float>());
      hs.push_back(static_cast<int>(m.x->dims()[2]));
      ws.push_back(static_cast<int>(m.x->dims()[3]));
      anchors.push_back(m.anchors.data());
      lens.push_back(static_cast<int>(m.anchors.size()));
      ratios.push_back(m.downsample_ratio);
    }
    HIP_CALL(ctx.ctx(), plhip_yolo_head_f32(ctx.ctx(), xs.data(), hs.data(), ws.data(), anchors.data(), lens.data(), ratios.data(),
                                            static_cast<int>(xs.size()), param.ImgSize->data<int>(), static_cast<int>(param.X->dims()[0]),
                                            param.class_num, param.conf_thresh, param.clip_bbox ? 1 : 0, param.scale_x_y,
                                            param.Boxes->mutable_data<float>(TARGET(kHIP)), param.Scores->mutable_data<float>(TARGET(kHIP))));
  }
  void SetProfileRuntimeKernelInfo(profile::OpCharacter* ch) override { ch->kernel_func_name = "yolo_head_hip"; }

 private:
  HipYoloHead head_;
};

}  // namespace hip
}  // namespace kernels
}  // namespace lite
}  // namespace paddle

REGISTER_LITE_KERNEL(yolo_box, kHIP, kFloat, kNCHW, paddle::lite::kernels::hip::YoloBoxCompute, def)
    .BindInput("X", {LiteType::GetTensorTy(TARGET(kHIP))})
    .BindInput("ImgSize", {LiteType::GetTensorTy(TARGET(kHIP), PRECISION(kInt32))})
    .BindOutput("Boxes", {LiteType::GetTensorTy(TARGET(kHIP))})
    .BindOutput("Scores", {LiteType::GetTensorTy(TARGET(kHIP))})
    .Finalize();
REGISTER_LITE_KERNEL(yolo_box, kHIP, kFloat, kNCHW, paddle::lite::kernels::hip::YoloHeadCompute, head)
    .BindInput("X", {LiteType::GetTensorTy(TARGET(kHIP))})
    .BindInput("ImgSize", {LiteType::GetTensorTy(TARGET(kHIP), PRECISION(kInt32))})
    .BindOutput("Boxes", {LiteType::GetTensorTy(TARGET(kHIP))})
    .BindOutput("Scores", {LiteType::GetTensorTy(TARGET(kHIP))})
    .Finalize();
