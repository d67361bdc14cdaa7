// shuffle_fusion.h — the kHIP-side state of graph-level fusion K (lite/api/graph_builder.h): a shuffle_channel(group 2) that took
// the two-input concat in front of it over, together with
//   K2 (alias int8): the calib[fp32_to_int8] behind it:  concat -> shuffle_channel -> calib                 => ONE launch
//   K1 (alias unit): the split in two halves behind it and the calib behind the split's second output:
//                    concat -> shuffle_channel -> split -> calib                                            => ONE launch
// (plhip_shuffle_unit_f32).  `X` of the ShuffleChannelParam is then the concat's first operand [N, h, H, W]; `Out` is the shuffled
// tensor [N, 2 h, H, W] (int8) or the split's first output [N, h, H, W] (unit).  Like conv_fusion.h / se_gate_fusion.h: not part of
// the reference's parameter struct (lite/operators/op_params.h:258-263); attached to the kernel object through
// HipShuffleFusionKernel::SetShuffleFusion, after SetParam.
#pragma once
#include "lite/core/tensor.h"
#include "lite/kernels/hip/calib_tail.h"

namespace paddle {
namespace lite {
namespace kernels {
namespace hip {

struct HipShuffleFusion {
  const lite::Tensor* second{nullptr};  // the concat's second operand, X's shape
  lite::Tensor* hi_output{nullptr};     // unit: the split's second output (fp32), written unless the tail drops it
  HipCalibTail tail;                    // the calib taken over (calib_output == nullptr: none): of Out (int8) or of hi_output (unit)
};

class HipShuffleFusionKernel {
 public:
  virtual void SetShuffleFusion(const HipShuffleFusion& f) = 0;
  virtual ~HipShuffleFusionKernel() = default;
};

}  // namespace hip
}  // namespace kernels
}  // namespace lite
}  // namespace paddle
