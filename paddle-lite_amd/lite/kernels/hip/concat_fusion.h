// concat_fusion.h — the kHIP-side state of graph-level fusion L (lite/api/graph_builder.h): a concat that took the
// calib[fp32_to_int8] behind it over,
//   concat -> calib                                                                                         => ONE launch
// (plhip_concat_calib_f32).  The ConcatParam stays the reference's (lite/operators/op_params.h:369-386): `x` the operands, `output`
// the fp32 tensor, `axis`.  Like shuffle_fusion.h: what the reference's struct has no field for is attached to the kernel object
// through HipConcatFusionKernel::SetConcatFusion, after SetParam.
#pragma once
#include "lite/core/tensor.h"

namespace paddle {
namespace lite {
namespace kernels {
namespace hip {

struct HipConcatFusion {
  lite::Tensor* calib_output{nullptr};  // the int8 tensor of the calib taken over, output's shape
  float calib_scale{1.f};
  bool drop_fp32_output{false};         // `output` has no reader left: it only carries the shape
};

class HipConcatFusionKernel {
 public:
  virtual void SetConcatFusion(const HipConcatFusion& f) = 0;
  virtual ~HipConcatFusionKernel() = default;
};

}  // namespace hip
}  // namespace kernels
}  // namespace lite
}  // namespace paddle
