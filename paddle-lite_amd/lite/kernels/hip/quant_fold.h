// quant_fold.h — the scale / bias / activation fold of an int8 conv or fc, as the reference's GEMM-like conv does it
// (conv_gemmlike.cc:208-263, conv_depthwise.cc:146-158,242-271), once for every kHIP kernel class:
//   scale_j = ws_j * in_scale / out_scale (int8 output) | ws_j * in_scale (fp32 output), one weight scale broadcast to oc;
//   bias_j  = b_j / out_scale (int8 output);   relu6's clip = coef / out_scale (int8 output).
// fp32, one operation at a time in exactly this order: the int8 results of every kernel are bit-exact against the oracle
// only as long as `ws * in_scale / out_scale` is evaluated left to right (never ws * (in_scale / out_scale)).
// FoldQuant is pure host code (tests/test_quant_fold.py compiles and checks it alone).  FoldLayer, what the kernel classes call,
// is FoldQuant behind the one step that needs the runtime: it checks the bias tensor's size (that CHECK lives there, not in the
// tested FoldQuant) and brings it to the host.  UploadFold puts the result on the device.
#pragma once
#include <vector>

#include "lite/core/tensor.h"
#include "lite/operators/op_params.h"
#include "plhip.h"

namespace paddle {
namespace lite {
namespace kernels {
namespace hip {

struct QuantFold {
  std::vector<float> scale;  // oc folded scales
  std::vector<float> bias;   // oc folded biases; empty = no bias
  int act{PLHIP_ACT_NONE};   // PLHIP_ACT_*
  float alpha{0.f};          // relu6 clip (folded) / leaky slope
};

// bias: oc floats on the host, or nullptr.  act: the op's ActivationParam, or nullptr (fc); fuse_relu: the legacy flag, read
// only when `act` names no activation (conv_gemmlike.cc:325-345).
inline QuantFold FoldQuant(const std::vector<float>& weight_scale, int oc, float in_scale, float out_scale, bool int8_out,
                           const float* bias, const operators::ActivationParam* act, bool fuse_relu) {
  QuantFold f;
  f.scale = weight_scale;
  if (f.scale.size() != 1 && f.scale.size() != static_cast<size_t>(oc)) LOG(FATAL) << "weights scale size must equal to filter size";
  if (f.scale.size() == 1) f.scale.resize(oc, f.scale[0]);
  for (auto& ws : f.scale) ws = int8_out ? ws * in_scale / out_scale : ws * in_scale;
  if (bias) {
    f.bias.assign(bias, bias + oc);
    if (int8_out)
      for (auto& b : f.bias) b = b / out_scale;
  }
  if (act && act->has_active) {
    switch (act->active_type) {
      case lite_api::ActivationType::kRelu: f.act = PLHIP_ACT_RELU; break;
      case lite_api::ActivationType::kRelu6: f.act = PLHIP_ACT_RELU6; f.alpha = act->Relu_clipped_coef; break;
      case lite_api::ActivationType::kLeakyRelu: f.act = PLHIP_ACT_LEAKY_RELU; f.alpha = act->Leaky_relu_alpha; break;
      default: LOG(FATAL) << "this act_type: " << static_cast<int>(act->active_type) << " fuse not support";
    }
  } else if (fuse_relu) {
    f.act = PLHIP_ACT_RELU;
  }
  if (int8_out && f.act == PLHIP_ACT_RELU6) f.alpha = f.alpha / out_scale;  // conv_gemmlike.cc:259-263
  return f;
}

// FoldQuant of a layer whose bias is a tensor (on the host or the device, or nullptr): the shape of every call site.
inline QuantFold FoldLayer(const std::vector<float>& weight_scale, int oc, float in_scale, float out_scale, bool int8_out,
                           const Tensor* bias, const operators::ActivationParam* act, bool fuse_relu) {
  std::vector<float> b;
  if (bias) {
    CHECK_EQ(bias->numel(), oc) << "bias size must equal to filter number";
    b.resize(oc);
    TargetCopy(TARGET(kHost), bias->target(), b.data(), bias->raw_data(), oc * sizeof(float));
  }
  return FoldQuant(weight_scale, oc, in_scale, out_scale, int8_out, bias ? b.data() : nullptr, act, fuse_relu);
}

// Folded scale (and bias, if any) to the device; returns whether there is a bias.
inline bool UploadFold(const QuantFold& f, Tensor* scale, Tensor* bias) {
  auto upload = [](const std::vector<float>& v, Tensor* t) {
    t->Resize({static_cast<int64_t>(v.size())});
    TargetWrapperHip::MemcpySync(t->mutable_data<float>(TARGET(kHIP)), v.data(), v.size() * sizeof(float), IoDirection::HtoD);
  };
  upload(f.scale, scale);
  if (!f.bias.empty()) upload(f.bias, bias);
  return !f.bias.empty();
}

}  // namespace hip
}  // namespace kernels
}  // namespace lite
}  // namespace paddle
