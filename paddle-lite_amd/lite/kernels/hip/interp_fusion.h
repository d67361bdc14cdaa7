// interp_fusion.h — the kHIP-side state of graph-level fusion M (lite/api/graph_builder.h):
//   M  bilinear_interp | nearest_interp -> arg_max(axis 1)                                => ONE launch (plhip_interp_argmax_f32)
// The ArgmaxParam stays the reference's (lite/operators/op_params.h:821-827).  What the reference's struct has no field for is
// attached to the kernel object after SetParam: the arg_max kernel (alias interp) reads the LOW-resolution tensor as its X and gets
// the attributes of the interp taken over; the resampled tensor never exists.
// Fusion N (interp -> calib[fp32_to_int8], the interp's alias int8) is a calib tail: calib_tail.h.
#pragma once
#include "lite/core/tensor.h"
#include "lite/operators/op_params.h"

namespace paddle {
namespace lite {
namespace kernels {
namespace hip {

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
