// interp_fusion.h — the kHIP-side state of graph-level fusions M and N (lite/api/graph_builder.h):
//   N  bilinear_interp | nearest_interp -> calib[fp32_to_int8]                            => ONE launch (plhip_interp_f32 with y_i8)
//   M  bilinear_interp | nearest_interp -> arg_max(axis 1)                                => ONE launch (plhip_interp_argmax_f32)
// The InterpolateParam / ArgmaxParam stay the reference's (lite/operators/op_params.h:154-168, 821-827).  Like concat_fusion.h:
// what the reference's structs have no field for is attached to the kernel object after SetParam.
//   N: the interp kernel (alias int8) gets the calib's tensor and scale, and whether its own fp32 output still has a reader.
//   M: the arg_max kernel (alias interp) reads the LOW-resolution tensor as its X and gets the attributes of the interp taken
//      over; the resampled tensor never exists.
#pragma once
#include "lite/core/tensor.h"
#include "lite/operators/op_params.h"

namespace paddle {
namespace lite {
namespace kernels {
namespace hip {

struct HipInterpFusion {
  lite::Tensor* calib_output{nullptr};  // the int8 tensor of the calib taken over, Out's shape
  float calib_scale{1.f};
  bool drop_fp32_output{false};         // Out has no reader left: it only carries the shape
};

class HipInterpFusionKernel {
 public:
  virtual void SetInterpFusion(const HipInterpFusion& f) = 0;
  virtual ~HipInterpFusionKernel() = default;
};

struct HipInterpArgmaxFusion {
  std::string op_type;                   // bilinear_interp | nearest_interp
  operators::InterpolateParam interp;    // the attributes of the interp taken over (its tensors are not read)
};

class HipInterpArgmaxKernel {
 public:
  virtual void SetInterpArgmax(const HipInterpArgmaxFusion& f) = 0;
  virtual ~HipInterpArgmaxKernel() = default;
};

}  // namespace hip
}  // namespace kernels
}  // namespace lite
}  // namespace paddle
