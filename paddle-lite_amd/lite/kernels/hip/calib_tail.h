// calib_tail.h — the one declaration of a calib tail: an fp32 op that took the calib[fp32_to_int8] behind it over.  The kHIP-side
// state of the graph-level fusions J1 / J3 (hard_swish, elementwise_mul), L (concat), N (bilinear_interp / nearest_interp) and,
// as a member of HipShuffleFusion (shuffle_fusion.h), K (the tail of a ShuffleNetV2 unit); lite/api/graph_builder.h has the letters.
//
// NOT part of the reference's parameter structs (lite/operators/op_params.h: ActivationParam, ElementwiseParam, ConcatParam,
// InterpolateParam): those stay field-for-field subsets of the reference's, as conv_fusion.h explains for ConvParam.  The graph
// builder attaches the state to the picked kernel object (alias "int8") through HipCalibTailKernel::SetCalibTail, after SetParam.
//
// Out of scope here: HipConvFusion (conv_fusion.h) keeps its own flat calib_output / calib_scale / drop_fp32_output fields.
// patches/0006 and tools/make_khip_patches.py carry those names into a Paddle-Lite tree, and tests/test_patches.py pins them.
#pragma once
#include "lite/core/tensor.h"
#include "lite/utils/logging.h"

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

// what every kernel class does with a calib tail: the output pointers of one launch
struct TailOutputs {
  float* f32{nullptr};
  int8_t* i8{nullptr};
  float scale{1.f};
};
// `on`: this launch writes the int8 image (the alias that carries the tail; for shuffle_channel, a tail was attached).  `out` is the
// fp32 tensor the calib read: the int8 image copies its shape, and it is allocated unless the tail drops it.
inline TailOutputs OutputsOf(const HipCalibTail& t, bool on, lite::Tensor* out) {
  TailOutputs o;
  if (on) {
    CHECK(t.calib_output) << "the int8 form needs the calib tail the graph builder attaches (calib_tail.h)";
    t.calib_output->Resize(out->dims());
    o.i8 = t.calib_output->mutable_data<int8_t>(TARGET(kHIP));
    o.scale = t.calib_scale;
  }
  if (!on || !t.drop_fp32_output) o.f32 = out->mutable_data<float>(TARGET(kHIP));
  return o;
}
// the part of the profile name between the op's and "_hip"
inline const char* TailSuffix(const HipCalibTail& t, bool on) { return !on ? "" : t.drop_fp32_output ? "_int8" : "_fp32_int8"; }

}  // namespace hip
}  // namespace kernels
}  // namespace lite
}  // namespace paddle
