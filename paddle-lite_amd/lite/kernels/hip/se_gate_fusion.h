// se_gate_fusion.h — the kHIP-side state of graph-level fusion J2 (lite/api/graph_builder.h): the hard_sigmoid of a
// squeeze-excite block that took the excite chain in front of it over,
//   calib[fp32_to_int8] -> conv2d 1x1 C -> Cr [int8_out] -> conv2d 1x1 Cr -> C [fp32_out] -> hard_sigmoid   => ONE launch
// (plhip_se_gate_int8).  `X` of the ActivationParam is then the pooled fp32 tensor [N, C, 1, 1] the calib read.  Like
// conv_fusion.h: not part of the reference's parameter structs; attached to the kernel object (hard_sigmoid, alias se_gate)
// through HipSeGateKernel::SetSeGate, after SetParam.
#pragma once
#include <vector>

#include "lite/core/tensor.h"
#include "lite/operators/op_params.h"

namespace paddle {
namespace lite {
namespace kernels {
namespace hip {

struct HipSeGateConv {  // one of the two 1x1 convs, as its ConvParam had it
  lite::Tensor* filter{nullptr};  // [out, in, 1, 1] int8
  lite::Tensor* bias{nullptr};
  std::vector<float> weight_scale{};
  float input_scale{1.f};
  operators::ActivationParam activation_param;
};

struct HipSeGateFusion {
  float calib_scale{1.f};  // of the calib taken over == reduce.input_scale
  HipSeGateConv reduce;    // C -> Cr, int8 output with expand.input_scale as its output scale
  HipSeGateConv expand;    // Cr -> C, fp32 output
};

class HipSeGateKernel {
 public:
  virtual void SetSeGate(const HipSeGateFusion& f) = 0;
  virtual ~HipSeGateKernel() = default;
};

}  // namespace hip
}  // namespace kernels
}  // namespace lite
}  // namespace paddle
