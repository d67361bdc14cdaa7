// detection_fusion.h — the kHIP-side state of multiclass_nms and of graph-level fusion O (lite/api/graph_builder.h).
// The MulticlassNmsParam stays the reference's (lite/operators/op_params.h:910-922).  The reference's host kernel writes an
// output whose length is the number of detections; the kHIP kernel writes out [N, keep_top_k, 6] (rows past an image's count
// filled with -1) and the per-image counts into a tensor the struct has no field for.  Like interp_fusion.h / calib_tail.h:
// what the reference's struct lacks is attached to the kernel object after SetParam.
//   count            the int32 [N] tensor of the per-image counts; its variable is "<out>/count"
//   scores_npc       fusion O2: the transpose(0,2,1) in front of the scores operand was folded away, `scores` is [N, P, C] and the
//                    kernel reads it through its strides
#pragma once
#include "lite/core/tensor.h"

namespace paddle {
namespace lite {
namespace kernels {
namespace hip {

struct HipNmsFusion {
  lite::Tensor* count{nullptr};
  bool scores_npc{false};
};

class HipNmsFusionKernel {
 public:
  virtual void SetNmsFusion(const HipNmsFusion& f) = 0;
  virtual ~HipNmsFusionKernel() = default;
};

}  // namespace hip
}  // namespace kernels
}  // namespace lite
}  // namespace paddle
