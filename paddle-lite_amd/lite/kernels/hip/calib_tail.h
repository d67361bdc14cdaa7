// calib_tail.h — the kHIP-side state of the graph-level fusions J1 / J3 (lite/api/graph_builder.h): an fp32 op
// (hard_swish, elementwise_mul) that took the calib[fp32_to_int8] behind it over.
//
// NOT part of operators::ActivationParam / ElementwiseParam: those stay field-for-field subsets of the reference's structs
// (lite/operators/op_params.h:395-419, 643-651), as conv_fusion.h explains for ConvParam.  The graph builder attaches the
// state to the picked kernel object (alias "int8") through HipCalibTailKernel::SetCalibTail, after SetParam.
#pragma once
#include "lite/core/tensor.h"

namespace paddle {
namespace lite {
namespace kernels {
namespace hip {

struct HipCalibTail {
  lite::Tensor* calib_output{nullptr};  // the int8 tensor the calib[fp32_to_int8] with calib_scale behind `Out` would produce
  float calib_scale{1.f};
  bool drop_fp32_output{false};  // `Out` has no other reader: it only carries the shape and is never allocated
};

class HipCalibTailKernel {
 public:
  virtual void SetCalibTail(const HipCalibTail& t) = 0;
  virtual ~HipCalibTailKernel() = default;
};

}  // namespace hip
}  // namespace kernels
}  // namespace lite
}  // namespace paddle
