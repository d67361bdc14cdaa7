// conv_compute.h — ConvCompute<PRECISION(kInt8), OutType> for TARGET(kHIP): the drop-in for
// lite/kernels/arm/conv_compute.h:27-58 (+ conv_gemmlike / conv_depthwise / conv_direct / conv_winograd,
// which collapse into two device paths here: MFMA GEMM and depthwise).
#pragma once
#include <memory>
#include <string>
#include <vector>

#include "lite/core/kernel.h"
#include "lite/kernels/hip/conv_fusion.h"
#include "lite/operators/op_params.h"
#include "plhip.h"

namespace paddle {
namespace lite {
namespace kernels {
namespace hip {

// One conv as a launch takes it: the descriptor (desc.act / desc.act_alpha = the folded activation, quant_fold.h), the weights
// (packed for the GEMM path, raw OIHW for the depthwise path; the process-wide shared copy where packed_weight_cache.h shares
// them) and the folded per-channel scale and bias, all on the device.
struct FoldedConv {
  plhip_conv_desc desc{};
  std::shared_ptr<Tensor> weights;
  Tensor scale, bias;
  bool has_bias{false};
  const float* sc() const { return scale.data<float>(); }
  const float* bi() const { return has_bias ? bias.data<float>() : nullptr; }
};

template <PrecisionType Ptype, PrecisionType OutType>
class ConvCompute : public KernelLite<TARGET(kHIP), Ptype>, public HipFusableKernel {
 public:
  using param_t = operators::ConvParam;
  void PrepareForRun() override;
  void ReInitWhenNeeded() override;
  void Run() override;
  void SetFusion(const HipConvFusion& f) override { fusion_ = f; }  // before the first Launch (conv_fusion.h)
  void SetProfileRuntimeKernelInfo(profile::OpCharacter* ch) override { ch->kernel_func_name = kernel_func_name_; }
  ~ConvCompute() override = default;

 private:
  // What Run launches for the current input shape; ReInitWhenNeeded decides it (ResolveRoute), KernelFuncName names it.
  enum class Route {
    kImageStem,        // fusion H1: image_to_tensor + calib + conv in one launch
    kCalibStem,        // fusion F: calib + conv in one launch
    kConvTail,         // conv [fp32_out] with its residual add / calib copy
    kDwConv1x1Fused,   // fusion G: depthwise + 1x1 conv with that conv's tail, one launch
    kDwConv1x1Split,   //           ... the shape is outside the fused kernel: two launches through mid_
    kDwPwFused,        // fusions D / E: depthwise + 1x1 conv (+ global average pool), one launch
    kDwPwSplit,        //           ... two (three) launches through mid_ (mid2_)
    kDepthwise,
    kConv,
  };
  struct Tail {  // the graph tail of an fp32 conv output: residual operand, int8 copy
    const float* residual{nullptr};
    int8_t* calib_out{nullptr};
  };
  void BuildDesc();
  void PackWeights();
  void PreparePointwise();
  Route ResolveRoute();
  std::string KernelFuncName() const;
  const int8_t* Int8Input();
  void* Output(bool int8, bool drop = false);
  Tail GatherTail(bool f32);
  const int8_t* DepthwiseIntoMid(const int8_t* x);
  void RunStem();
  void RunConvTail(const int8_t* x);
  void RunDwConv1x1(const int8_t* x);
  void RunDwPw(const int8_t* x);

  HipConvFusion fusion_;  // default-constructed = the plain conv of the reference
  FoldedConv conv_;       // the op's own conv
  FoldedConv pw_;         // the 1x1 consumer a depthwise conv took over (HipConvFusion::pw_filter), its input plane from conv_.desc
  bool is_depthwise_{false};
  DDim last_shape_;
  std::string packed_impl_;  // the implementation conv_.weights are packed for, and their size: checked on every reshape
  size_t packed_bytes_{0};
  size_t workspace_bytes_{0};
  Route route_{Route::kConv};
  std::string kernel_func_name_{"NotImplForConv"};
  Tensor mid_, mid2_;              // the split routes' depthwise result (and the 1x1 conv's plane in front of the pool)
  Tensor xq_;                      // the int8 input of a conv that took its calib (or image) over, on a shape without the one-launch form
  plhip_image_desc image_desc_{};  // HipConvFusion::image_input: the image, [n, h, w] from the descriptor
};

}  // namespace hip
}  // namespace kernels
}  // namespace lite
}  // namespace paddle
