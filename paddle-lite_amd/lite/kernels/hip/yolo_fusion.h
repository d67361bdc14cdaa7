// yolo_fusion.h — the kHIP-side state of graph-level fusion P (lite/api/graph_builder.h): one yolo_box/head instruction for the
// yolo_box ops of a YOLOv3 head, the two concats behind them and the transpose(0,2,1) in front of multiclass_nms.
// The YoloBoxParam stays the reference's (lite/operators/op_params.h:266-278) and describes the FIRST feature map: X, anchors and
// downsample_ratio are its own, ImgSize, class_num, conf_thresh, clip_bbox and scale_x_y are shared by all, Boxes is the joined
// [N, P, 4] tensor and Scores the [N, class_num, P] tensor the NMS reads.  Like detection_fusion.h / interp_fusion.h: what the
// reference's struct lacks is attached to the kernel object after SetParam.
//   more             the feature maps behind the first, in the order of the concats, each with its anchors and downsample_ratio
#pragma once
#include <vector>

#include "lite/core/tensor.h"

namespace paddle {
namespace lite {
namespace kernels {
namespace hip {

struct HipYoloScale {
  const lite::Tensor* x{nullptr};
  std::vector<int> anchors;
  int downsample_ratio{0};
};

struct HipYoloHead {
  std::vector<HipYoloScale> more;
};

class HipYoloHeadKernel {
 public:
  virtual void SetYoloHead(const HipYoloHead& h) = 0;
  virtual ~HipYoloHeadKernel() = default;
};

}  // namespace hip
}  // namespace kernels
}  // namespace lite
}  // namespace paddle
