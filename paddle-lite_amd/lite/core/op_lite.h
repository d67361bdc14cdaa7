// op_lite.h — OpLite (lite/core/op_lite.h:54-) reduced to what Instruction::Run needs (program.cc:436-467):
// CheckShape() once, InferShape() before every launch, AttachKernel() to hand the op's parameter struct to the
// picked kernel.  The ops below restate the shape inference of lite/operators/{conv_op.cc:25-111, fc_op.cc,
// calib_op.cc, io_copy_op.cc, pool_op.cc, softmax_op.cc, concat_op.cc, split_op.cc, shuffle_channel_op.cc}; attributes are set on the param struct directly, as the
// reference's math tests do (conv_int8_compute_test.cc:90-117), because there is no model parser in this build.
#pragma once
#include <algorithm>
#include <memory>
#include <string>

#include "lite/core/kernel.h"
#include "lite/operators/op_params.h"

namespace paddle {
namespace lite {

class OpLite {
 public:
  explicit OpLite(const std::string& type) : op_type_(type) {}
  virtual ~OpLite() = default;
  virtual bool CheckShape() const { return true; }
  virtual bool InferShape() { return InferShapeImpl(); }
  virtual bool InferShapeImpl() const { return true; }
  virtual void AttachKernel(KernelBase* kernel) = 0;
  const std::string& Type() const { return op_type_; }

 protected:
  std::string op_type_;
};

namespace operators {

// conv_op.cc:25-52
inline int ConvOutputSize(int input_size, int filter_size, int dilation, int pad_left, int pad_right, int stride) {
  const int dkernel = dilation * (filter_size - 1) + 1;
  return (input_size + (pad_left + pad_right) - dkernel) / stride + 1;
}

// conv_op.cc:55-81
inline void UpdatePaddingAndDilation(std::vector<int>* paddings, std::vector<int>* dilations,
                                     const std::vector<int>& strides, const std::string& padding_algorithm,
                                     const DDim& data_dims, const DDim& ksize) {
  if (padding_algorithm == "SAME") {
    for (size_t i = 0; i < strides.size(); ++i) {
      const int out_size = static_cast<int>((data_dims[i + 2] + strides[i] - 1) / strides[i]);
      const int pad_sum = static_cast<int>(
          std::max<int64_t>((out_size - 1) * strides[i] + ksize[i + 2] - data_dims[i + 2], 0));
      const int pad_0 = pad_sum / 2;
      (*paddings)[i * 2] = pad_0;
      (*paddings)[i * 2 + 1] = pad_sum - pad_0;
      (*dilations)[i] = 1;
    }
  } else if (padding_algorithm == "VALID") {
    for (auto& p : *paddings) p = 0;
  }
}

class ConvOpLite : public OpLite {
 public:
  explicit ConvOpLite(const std::string& type = "conv2d") : OpLite(type) {}
  ConvParam& mutable_param() { return param_; }
  void set_padding_algorithm(const std::string& a) { padding_algorithm_ = a; }
  void set_output_channels(int64_t c) { out_channels_override_ = c; }  // kHIP fusions only (lite/kernels/hip/conv_fusion.h)
  void set_output_pooled() { out_pooled_ = true; }                     // ... with the global average pool behind it: [n, c, 1, 1]
  // kHIP fusion H1 (conv_fusion.h image_input): `x` takes the NCHW shape [n, channels, h, w] of the uint8 image [n, h, w, cs]
  void set_image_input(const Tensor* img, int channels) {
    image_ = img;
    image_channels_ = channels;
  }
  bool CheckShape() const override {
    CHECK(param_.x && param_.filter && param_.output) << "conv: x / filter / output must be set";
    ImageShape();
    const auto in = param_.x->dims(), f = param_.filter->dims();
    CHECK_EQ(in.size(), 4UL) << "conv input must be NCHW";
    CHECK_EQ(f.size(), 4UL);
    CHECK_EQ(in[1], f[1] * param_.groups) << "input channel must equal filter channel * groups";
    CHECK_EQ(f[0] % param_.groups, 0) << "filter number must be divisible by groups";
    // conv_op.h:149-161: 2-element paddings are expanded to {top, bottom, left, right}
    CHECK(param_.paddings && param_.dilations);
    if (param_.paddings->size() == 2UL) {
      const int ph = (*param_.paddings)[0], pw = (*param_.paddings)[1];
      *param_.paddings = {ph, ph, pw, pw};
    }
    CHECK_EQ(param_.paddings->size(), 4UL) << "paddings must have 2 or 4 entries";
    return true;
  }
  bool InferShapeImpl() const override {
    ImageShape();
    const auto in = param_.x->dims(), f = param_.filter->dims();
    UpdatePaddingAndDilation(param_.paddings.get(), param_.dilations.get(), param_.strides, padding_algorithm_, in, f);
    // kHIP dw -> pw fusion (opt-in): a depthwise conv that took its 1x1 consumer over writes THAT conv's output
    std::vector<int64_t> out{in[0], out_channels_override_ > 0 ? out_channels_override_ : f[0]};
    for (size_t i = 0; i < param_.strides.size(); ++i)
      out.push_back(ConvOutputSize(static_cast<int>(in[i + 2]), static_cast<int>(f[i + 2]), (*param_.dilations)[i],
                                   (*param_.paddings)[i * 2], (*param_.paddings)[i * 2 + 1], param_.strides[i]));
    if (out_pooled_)
      for (size_t i = 2; i < out.size(); ++i) out[i] = 1;
    param_.output->Resize(out);
    return true;
  }
  void AttachKernel(KernelBase* k) override { k->SetParam<ConvParam>(param_); }

 private:
  void ImageShape() const {
    if (!image_) return;
    const auto d = image_->dims();
    CHECK_EQ(d.size(), 4UL) << "conv: the image source must be [n, h, w, cs]";
    param_.x->Resize(std::vector<int64_t>{d[0], image_channels_, d[1], d[2]});
  }
  mutable ConvParam param_;
  std::string padding_algorithm_{""};
  int64_t out_channels_override_{0};
  bool out_pooled_{false};
  const Tensor* image_{nullptr};
  int64_t image_channels_{0};
};

// conv_transpose_op.cc:43-53: (in - 1) * stride - pads + the dilated kernel extent
inline int ConvTransposeOutputSize(int input_size, int filter_size, int dilation, int pad_left, int pad_right, int stride) {
  return (input_size - 1) * stride - pad_left - pad_right + dilation * (filter_size - 1) + 1;
}

// conv2d_transpose (conv_transpose_op.cc:25-96): ConvParam with the filter [cin][cout / groups][kh][kw]; output_size, where
// given, replaces the computed extent and must lie in [extent, extent + stride)
class ConvTransposeOpLite : public OpLite {
 public:
  ConvTransposeOpLite() : OpLite("conv2d_transpose") {}
  ConvParam& mutable_param() { return param_; }
  void set_padding_algorithm(const std::string& a) { padding_algorithm_ = a; }
  bool CheckShape() const override {
    CHECK(param_.x && param_.filter && param_.output) << "conv2d_transpose: x / filter / output must be set";
    const auto in = param_.x->dims(), f = param_.filter->dims();
    CHECK_EQ(in.size(), 4UL) << "conv2d_transpose input must be NCHW";
    CHECK_EQ(f.size(), 4UL);
    CHECK_EQ(param_.strides.size(), 2UL);
    CHECK_EQ(in[1] % param_.groups, 0) << "input channels must be divisible by groups";
    CHECK_EQ(in[1], f[0]) << "input channels must equal the filter's first extent";
    CHECK(param_.paddings && param_.dilations);
    if (param_.paddings->size() == 2UL) {  // 2-element paddings mean {top = bottom, left = right}
      const int ph = (*param_.paddings)[0], pw = (*param_.paddings)[1];
      *param_.paddings = {ph, ph, pw, pw};
    }
    CHECK_EQ(param_.paddings->size(), 4UL) << "paddings must have 2 or 4 entries";
    CHECK(param_.output_size.empty() || param_.output_size.size() == 2UL) << "output_size must have 0 or 2 entries";
    return true;
  }
  bool InferShapeImpl() const override {
    const auto in = param_.x->dims(), f = param_.filter->dims();
    UpdatePaddingAndDilation(param_.paddings.get(), param_.dilations.get(), param_.strides, padding_algorithm_, in, f);
    std::vector<int64_t> out{in[0], f[1] * param_.groups};
    for (size_t i = 0; i < param_.strides.size(); ++i)
      out.push_back(ConvTransposeOutputSize(static_cast<int>(in[i + 2]), static_cast<int>(f[i + 2]), (*param_.dilations)[i],
                                            (*param_.paddings)[i * 2], (*param_.paddings)[i * 2 + 1], param_.strides[i]));
    for (size_t i = 0; i < param_.output_size.size(); ++i) {
      CHECK_LT(param_.output_size[i], out[i + 2] + param_.strides[i]) << "conv2d_transpose: output_size must be below " << out[i + 2] + param_.strides[i];
      CHECK_GE(param_.output_size[i], out[i + 2]) << "conv2d_transpose: output_size must be at least " << out[i + 2];
      out[i + 2] = param_.output_size[i];
    }
    param_.output->Resize(out);
    return true;
  }
  void AttachKernel(KernelBase* k) override { k->SetParam<ConvParam>(param_); }

 private:
  mutable ConvParam param_;
  std::string padding_algorithm_{""};
};

class FcOpLite : public OpLite {
 public:
  FcOpLite() : OpLite("fc") {}
  FcParam& mutable_param() { return param_; }
  bool CheckShape() const override {
    CHECK(param_.input && param_.w && param_.output);
    CHECK_EQ(param_.w->dims().size(), 2UL);
    const auto in = param_.input->dims();
    CHECK_GT(static_cast<int>(in.size()), param_.in_num_col_dims);
    CHECK_EQ(in.count(param_.in_num_col_dims, static_cast<int>(in.size())), param_.w->dims()[0])
        << "fc: flattened input width must equal w.dims[0]";
    return true;
  }
  bool InferShapeImpl() const override {  // fc_op.cc: out = in.dims[:ncol] + {w.dims[1]}
    const auto in = param_.input->dims();
    std::vector<int64_t> out;
    for (int i = 0; i < param_.in_num_col_dims; ++i) out.push_back(in[i]);
    out.push_back(param_.w->dims()[1]);
    param_.output->Resize(out);
    return true;
  }
  void AttachKernel(KernelBase* k) override { k->SetParam<FcParam>(param_); }

 private:
  mutable FcParam param_;
};

class CalibOpLite : public OpLite {
 public:
  CalibOpLite() : OpLite("calib") {}
  CalibParam& mutable_param() { return param_; }
  bool InferShapeImpl() const override {
    param_.output->Resize(param_.input->dims());
    return true;
  }
  void AttachKernel(KernelBase* k) override { k->SetParam<CalibParam>(param_); }

 private:
  mutable CalibParam param_;
};

class IoCopyOp : public OpLite {
 public:
  IoCopyOp() : OpLite("io_copy") {}
  IoCopyParam& mutable_param() { return param_; }
  bool InferShapeImpl() const override {
    param_.y->Resize(param_.x->dims());
    return true;
  }
  void AttachKernel(KernelBase* k) override { k->SetParam<IoCopyParam>(param_); }

 private:
  mutable IoCopyParam param_;
};

// pool_op.cc:44-61
inline int PoolOutputSize(int input_size, int filter_size, int pad_left, int pad_right, int stride, bool ceil_mode) {
  if (!ceil_mode) return (input_size - filter_size + pad_left + pad_right) / stride + 1;
  return (input_size - filter_size + pad_left + pad_right + stride - 1) / stride + 1;
}

// pool_op.h:119-150
inline void UpdatePoolPadding(std::vector<int>* paddings, bool global_pooling, bool adaptive,
                              const std::string& padding_algorithm, const DDim& data_dims,
                              const std::vector<int>& strides, const std::vector<int>& ksize) {
  if (padding_algorithm == "SAME") {
    for (size_t i = 0; i < strides.size(); ++i) {
      const int out_size = static_cast<int>((data_dims[i + 2] + strides[i] - 1) / strides[i]);
      const int pad_sum =
          static_cast<int>(std::max<int64_t>((out_size - 1) * strides[i] + ksize[i] - data_dims[i + 2], 0));
      (*paddings)[i * 2] = pad_sum / 2;
      (*paddings)[i * 2 + 1] = pad_sum - pad_sum / 2;
    }
  } else if (padding_algorithm == "VALID") {
    for (auto& p : *paddings) p = 0;
  }
  if (global_pooling || adaptive)
    for (auto& p : *paddings) p = 0;
}

class PoolOpLite : public OpLite {
 public:
  PoolOpLite() : OpLite("pool2d") {}
  PoolParam& mutable_param() { return param_; }
  void set_padding_algorithm(const std::string& a) { padding_algorithm_ = a; }
  bool CheckShape() const override {
    CHECK(param_.x && param_.output && param_.paddings);
    CHECK_EQ(param_.x->dims().size(), 4UL) << "pool2d input must be NCHW";
    if (param_.paddings->size() == 2UL) {  // pool_op.h AttachKernel: 2-element paddings -> {top, bottom, left, right}
      const int ph = (*param_.paddings)[0], pw = (*param_.paddings)[1];
      *param_.paddings = {ph, ph, pw, pw};
    }
    CHECK_EQ(param_.paddings->size(), 4UL);
    if (!param_.global_pooling) {
      CHECK_EQ(param_.ksize.size(), 2UL);
      CHECK_EQ(param_.strides.size(), 2UL);
    }
    return true;
  }
  bool InferShapeImpl() const override {  // pool_op.cc:63-98
    const auto in = param_.x->dims();
    UpdatePoolPadding(param_.paddings.get(), param_.global_pooling, param_.adaptive, padding_algorithm_, in,
                      param_.strides, param_.ksize);
    if (param_.global_pooling) {
      param_.ksize.resize(2);
      param_.ksize[0] = static_cast<int>(in[2]);
      param_.ksize[1] = static_cast<int>(in[3]);
    }
    CHECK(!param_.adaptive) << "adaptive pooling is not on the int8 hot path";
    std::vector<int64_t> out{in[0], in[1]};
    for (size_t i = 0; i < 2; ++i)
      out.push_back(PoolOutputSize(static_cast<int>(in[i + 2]), param_.ksize[i], (*param_.paddings)[2 * i],
                                   (*param_.paddings)[2 * i + 1], param_.strides[i], param_.ceil_mode));
    param_.output->Resize(out);
    return true;
  }
  void AttachKernel(KernelBase* k) override { k->SetParam<PoolParam>(param_); }

 private:
  mutable PoolParam param_;
  std::string padding_algorithm_{""};
};

// elementwise_ops.cc: Out takes X's dims (same-shape operands on this path; Y broadcast along `axis` is not needed
// by the residual adds of ResNet50 / MobileNetV2)
class ElementwiseOp : public OpLite {
 public:
  explicit ElementwiseOp(const std::string& type = "elementwise_add") : OpLite(type) {}
  ElementwiseParam& mutable_param() { return param_; }
  bool CheckShape() const override {
    CHECK(param_.X && param_.Y && param_.Out);
    return true;
  }
  bool InferShapeImpl() const override {
    CHECK(param_.X->dims() == param_.Y->dims()) << op_type_ << ": operands must have the same shape on kHIP";
    param_.Out->Resize(param_.X->dims());
    return true;
  }
  void AttachKernel(KernelBase* k) override { k->SetParam<ElementwiseParam>(param_); }

 private:
  mutable ElementwiseParam param_;
};

// elementwise_ops.cc for elementwise_mul: Out takes X's dims.  Y is X's shape, or the per-(image, channel) operand of a
// squeeze-excite block ([N, C, 1, 1] or [N, C] along axis 0); the kernel refuses every other broadcast (PrepareForRun).
class ElementwiseMulOp : public OpLite {
 public:
  ElementwiseMulOp() : OpLite("elementwise_mul") {}
  ElementwiseParam& mutable_param() { return param_; }
  bool CheckShape() const override {
    CHECK(param_.X && param_.Y && param_.Out);
    return true;
  }
  bool InferShapeImpl() const override {
    CHECK_GE(param_.X->dims().size(), param_.Y->dims().size()) << "elementwise_mul: Y must not have more dims than X";
    param_.Out->Resize(param_.X->dims());
    return true;
  }
  void AttachKernel(KernelBase* k) override { k->SetParam<ElementwiseParam>(param_); }

 private:
  mutable ElementwiseParam param_;
};

// activation_ops.cc: Out takes X's dims.  hard_swish / hard_sigmoid read the ActivationParam fields of their names.
class ActivationOp : public OpLite {
 public:
  explicit ActivationOp(const std::string& type) : OpLite(type) {}
  ActivationParam& mutable_param() { return param_; }
  bool CheckShape() const override {
    CHECK(param_.X && param_.Out) << op_type_ << ": X / Out must be set";
    return true;
  }
  bool InferShapeImpl() const override {
    param_.Out->Resize(param_.X->dims());
    return true;
  }
  void AttachKernel(KernelBase* k) override { k->SetParam<ActivationParam>(param_); }

 private:
  mutable ActivationParam param_;
};

// fusion_elementwise_activation_ops.cc
class FusionElementwiseActivationOp : public OpLite {
 public:
  explicit FusionElementwiseActivationOp(const std::string& type = "fusion_elementwise_add_activation") : OpLite(type) {}
  FusionElementwiseActivationParam& mutable_param() { return param_; }
  bool CheckShape() const override {
    CHECK(param_.X && param_.Y && param_.Out);
    return true;
  }
  bool InferShapeImpl() const override {
    CHECK(param_.X->dims() == param_.Y->dims()) << op_type_ << ": operands must have the same shape on kHIP";
    param_.Out->Resize(param_.X->dims());
    return true;
  }
  void AttachKernel(KernelBase* k) override { k->SetParam<FusionElementwiseActivationParam>(param_); }

 private:
  mutable FusionElementwiseActivationParam param_;
};

// concat_op.cc:22-62: every input has the first one's dims outside `axis` (negative: from the back); Out sums the axis.
// kHIP alias nhwc (fusion O1, lite/kernels/hip/detection_fusion.h): the inputs are the NCHW tensors in front of the
// transpose(0,2,3,1) -> reshape([0,-1,k]) chains taken over, Out is [N, sum(C * H * W) / k, k].
class ConcatOpLite : public OpLite {
 public:
  ConcatOpLite() : OpLite("concat") {}
  ConcatParam& mutable_param() { return param_; }
  void set_nhwc_k(int k) { nhwc_k_ = k; }  // kHIP fusion O1 only
  bool CheckShape() const override {
    CHECK_GE(param_.x.size(), 1UL) << "concat: at least one input";
    CHECK(param_.output) << "concat: output must be set";
    return true;
  }
  bool InferShapeImpl() const override {
    CHECK(param_.axis_tensor == nullptr) << "concat: kHIP takes the axis attribute only";
    if (nhwc_k_ > 0) {
      int64_t rows = 0;
      for (size_t i = 0; i < param_.x.size(); ++i) {
        const auto d = param_.x[i]->dims();
        CHECK(d.size() == 4 && d[0] == param_.x[0]->dims()[0]) << "concat/nhwc: input " << i << " is not [N, C, H, W] of input 0's N";
        CHECK(d[1] % nhwc_k_ == 0) << "concat/nhwc: " << nhwc_k_ << " does not divide the " << d[1] << " channels of input " << i;
        rows += d[1] / nhwc_k_ * d[2] * d[3];
      }
      param_.output->Resize(std::vector<int64_t>{param_.x[0]->dims()[0], rows, nhwc_k_});
      return true;
    }
    auto out = param_.x[0]->dims().Vectorize();
    const int rank = static_cast<int>(out.size());
    const int axis = param_.axis < 0 ? param_.axis + rank : param_.axis;
    CHECK(axis >= 0 && axis < rank) << "concat: axis " << param_.axis << " outside the rank " << rank;
    for (size_t i = 1; i < param_.x.size(); ++i) {
      const auto d = param_.x[i]->dims();
      CHECK_EQ(static_cast<int>(d.size()), rank) << "concat: input " << i << " has another rank";
      for (int j = 0; j < rank; ++j) {
        if (j == axis) out[j] += d[j];
        else CHECK_EQ(out[j], d[j]) << "concat: input " << i << " differs from input 0 in dim " << j;
      }
    }
    param_.output->Resize(out);
    return true;
  }
  void AttachKernel(KernelBase* k) override { k->SetParam<ConcatParam>(param_); }

 private:
  mutable ConcatParam param_;
  int nhwc_k_{0};
};

// split_op.cc:32-75: num > 0: `num` equal parts of the axis; else sections[i] along it
class SplitOp : public OpLite {
 public:
  SplitOp() : OpLite("split") {}
  SplitParam& mutable_param() { return param_; }
  bool CheckShape() const override {
    CHECK(param_.x) << "split: x must be set";
    CHECK_GT(param_.output.size(), 0UL) << "split: at least one output";
    const int rank = static_cast<int>(param_.x->dims().size());
    CHECK(param_.axis >= -rank && param_.axis < rank) << "split: axis " << param_.axis << " outside the rank " << rank;
    return true;
  }
  bool InferShapeImpl() const override {
    CHECK(param_.axis_tensor == nullptr && param_.sections_tensor_list.empty()) << "split: kHIP takes the attributes only";
    const auto in = param_.x->dims().Vectorize();
    const int axis = param_.axis < 0 ? param_.axis + static_cast<int>(in.size()) : param_.axis;
    const size_t n = param_.output.size();
    if (param_.num > 0) {
      CHECK(static_cast<size_t>(param_.num) == n && in[axis] % param_.num == 0)
          << "split: num " << param_.num << " must equal the number of outputs and divide the axis (" << in[axis] << ")";
    } else {
      CHECK_EQ(param_.sections.size(), n) << "split: one section per output";
      int64_t sum = 0;
      for (int v : param_.sections) sum += v;
      CHECK_EQ(sum, in[axis]) << "split: the sections do not add up to the axis";
    }
    for (size_t i = 0; i < n; ++i) {
      auto d = in;
      d[axis] = param_.num > 0 ? in[axis] / param_.num : param_.sections[i];
      param_.output[i]->Resize(d);
    }
    return true;
  }
  void AttachKernel(KernelBase* k) override { k->SetParam<SplitParam>(param_); }

 private:
  mutable SplitParam param_;
};

// shuffle_channel_op.cc:23-31: Out takes X's dims.  kHIP fusion K2 (lite/kernels/hip/shuffle_fusion.h): X is the first of the two
// operands of the concat taken over, Out the shuffled tensor of twice its channels.
class ShuffleChannelOpLite : public OpLite {
 public:
  ShuffleChannelOpLite() : OpLite("shuffle_channel") {}
  ShuffleChannelParam& mutable_param() { return param_; }
  void set_output_channel_factor(int f) { channel_factor_ = f; }  // kHIP fusion K2 only
  bool CheckShape() const override {
    CHECK(param_.X && param_.Out) << "shuffle_channel: X / Out must be set";
    return true;
  }
  bool InferShapeImpl() const override {
    auto d = param_.X->dims().Vectorize();
    if (channel_factor_ != 1) {
      CHECK_GE(d.size(), 2UL);
      d[1] *= channel_factor_;
    }
    param_.Out->Resize(d);
    return true;
  }
  void AttachKernel(KernelBase* k) override { k->SetParam<ShuffleChannelParam>(param_); }

 private:
  mutable ShuffleChannelParam param_;
  int channel_factor_{1};
};

// interpolate_op.cc:34-82 with the size from the attributes: out_h / out_w where both are > 0, else int(in * scale) with
// scale > 0.  kHIP: NCHW, and no OutSize / SizeTensor / Scale tensor (the kernel's PrepareForRun is fatal on them too).
class InterpolateOp : public OpLite {
 public:
  explicit InterpolateOp(const std::string& type) : OpLite(type) {}
  InterpolateParam& mutable_param() { return param_; }
  // the output size the attributes give for an input of in_h x in_w
  static void OutputSize(const InterpolateParam& p, int64_t in_h, int64_t in_w, int64_t* out_h, int64_t* out_w) {
    if (p.out_h > 0 && p.out_w > 0) {
      *out_h = p.out_h;
      *out_w = p.out_w;
    } else {
      CHECK(p.scale > 0.f) << "interp: neither out_h / out_w nor a scale > 0";
      *out_h = static_cast<int>(in_h * p.scale);
      *out_w = static_cast<int>(in_w * p.scale);
    }
    CHECK(*out_h >= 1 && *out_w >= 1) << "interp: the output size " << *out_h << " x " << *out_w << " is empty";
  }
  bool CheckShape() const override {
    CHECK(param_.X && param_.Out) << op_type_ << ": X / Out must be set";
    CHECK_EQ(param_.X->dims().size(), 4UL) << op_type_ << ": X must be [N, C, H, W]";
    return true;
  }
  bool InferShapeImpl() const override {
    CHECK(!param_.OutSize && param_.SizeTensor.empty() && !param_.Scale) << op_type_ << ": kHIP takes the size attributes only";
    CHECK(param_.data_layout == DATALAYOUT(kNCHW)) << op_type_ << ": NCHW only";
    const auto d = param_.X->dims();
    int64_t oh, ow;
    OutputSize(param_, d[2], d[3], &oh, &ow);
    param_.Out->Resize(std::vector<int64_t>{d[0], d[1], oh, ow});
    return true;
  }
  void AttachKernel(KernelBase* k) override { k->SetParam<InterpolateParam>(param_); }

 private:
  mutable InterpolateParam param_;
};

// argmax_op.cc:29-60: Out drops (keepdims: keeps as 1) the axis.  kHIP alias interp (lite/kernels/hip/interp_fusion.h): X is the
// low-resolution tensor of the interp taken over, and the spatial dims of Out come from that interp's attributes.
class ArgmaxOpLite : public OpLite {
 public:
  ArgmaxOpLite() : OpLite("arg_max") {}
  ArgmaxParam& mutable_param() { return param_; }
  void set_interp(const InterpolateParam& p) {  // kHIP fusion M only
    interp_ = p;
    has_interp_ = true;
  }
  bool CheckShape() const override {
    CHECK(param_.X && param_.Out) << "arg_max: X / Out must be set";
    const int rank = static_cast<int>(param_.X->dims().size());
    CHECK(param_.Axis >= -rank && param_.Axis < rank) << "arg_max: axis " << param_.Axis << " outside the rank " << rank;
    return true;
  }
  bool InferShapeImpl() const override {
    auto in = param_.X->dims().Vectorize();
    if (has_interp_) {
      CHECK_EQ(in.size(), 4UL) << "arg_max/interp: X must be [N, C, H, W]";
      InterpolateOp::OutputSize(interp_, in[2], in[3], &in[2], &in[3]);
    }
    const int rank = static_cast<int>(in.size());
    const int axis = param_.Axis < 0 ? param_.Axis + rank : param_.Axis;
    std::vector<int64_t> out;
    for (int i = 0; i < rank; ++i) {
      if (i != axis) out.push_back(in[i]);
      else if (param_.keepdims) out.push_back(1);
    }
    param_.Out->Resize(out);
    return true;
  }
  void AttachKernel(KernelBase* k) override { k->SetParam<ArgmaxParam>(param_); }

 private:
  mutable ArgmaxParam param_;
  InterpolateParam interp_;
  bool has_interp_{false};
};

// transpose_op.cc: Out axis k is X axis perm[k]; rank 2 to 4 on kHIP.  transpose2's XShape is not written.
class TransposeOpLite : public OpLite {
 public:
  explicit TransposeOpLite(const std::string& type) : OpLite(type) {}
  TransposeParam& mutable_param() { return param_; }
  // fatal unless perm is a permutation of 0 .. rank - 1
  static void CheckPerm(const std::vector<int>& perm, size_t rank, const std::string& who) {
    CHECK(rank >= 2 && rank <= 4) << who << ": rank " << rank << " outside 2 .. 4";
    CHECK_EQ(perm.size(), rank) << who << ": the perm has " << perm.size() << " entries for rank " << rank;
    unsigned seen = 0;
    for (int a : perm) {
      CHECK(a >= 0 && a < static_cast<int>(rank) && !(seen & (1u << a))) << who << ": the perm is not a permutation of the axes";
      seen |= 1u << a;
    }
  }
  bool CheckShape() const override {
    CHECK(param_.x && param_.output) << op_type_ << ": x / output must be set";
    return true;
  }
  bool InferShapeImpl() const override {
    const auto in = param_.x->dims().Vectorize();
    CheckPerm(param_.axis, in.size(), op_type_);
    std::vector<int64_t> out(in.size());
    for (size_t k = 0; k < in.size(); ++k) out[k] = in[param_.axis[k]];
    param_.output->Resize(out);
    return true;
  }
  void AttachKernel(KernelBase* k) override { k->SetParam<TransposeParam>(param_); }

 private:
  mutable TransposeParam param_;
};

// reshape_op.cc ValidateShape for shape_vct: 0 copies the input's dim at that place, one -1 is inferred
class ReshapeOpLite : public OpLite {
 public:
  explicit ReshapeOpLite(const std::string& type) : OpLite(type) {}
  ReshapeParam& mutable_param() { return param_; }
  static std::vector<int64_t> OutputDims(const std::vector<int64_t>& in, const std::vector<int>& shape, const std::string& who) {
    int64_t total = 1, rest = 1;
    for (auto d : in) total *= d;
    int unknown = -1;
    std::vector<int64_t> out(shape.size());
    CHECK(!shape.empty()) << who << ": empty shape";
    for (size_t i = 0; i < shape.size(); ++i) {
      if (shape[i] == -1) {
        CHECK(unknown < 0) << who << ": more than one -1 in the shape";
        unknown = static_cast<int>(i);
        continue;
      }
      if (shape[i] == 0) {
        CHECK(i < in.size()) << who << ": 0 at place " << i << " beyond the input's rank";
        out[i] = in[i];
      } else {
        CHECK(shape[i] > 0) << who << ": dim " << shape[i] << " in the shape";
        out[i] = shape[i];
      }
      rest *= out[i];
    }
    if (unknown >= 0) {
      CHECK(rest > 0 && total % rest == 0) << who << ": the shape does not divide the input's " << total << " elements";
      out[unknown] = total / rest;
      rest *= out[unknown];
    }
    CHECK_EQ(rest, total) << who << ": the shape holds another count than the input";
    return out;
  }
  bool CheckShape() const override {
    CHECK(param_.x && param_.output) << op_type_ << ": x / output must be set";
    return true;
  }
  bool InferShapeImpl() const override {
    CHECK(param_.shape_tensor_vct.empty() && !param_.shape_tensor) << op_type_ << ": kHIP takes the shape attribute only";
    param_.output->Resize(OutputDims(param_.x->dims().Vectorize(), param_.shape_vct, op_type_));
    return true;
  }
  void AttachKernel(KernelBase* k) override { k->SetParam<ReshapeParam>(param_); }

 private:
  mutable ReshapeParam param_;
};

// prior_box_op.cc: Boxes and Variances [H, W, prior_num, 4] of the input feature map; prior_num is set by the caller
class PriorBoxOpLite : public OpLite {
 public:
  PriorBoxOpLite() : OpLite("prior_box") {}
  PriorBoxParam& mutable_param() { return param_; }
  bool CheckShape() const override {
    CHECK(param_.input && param_.image && param_.boxes && param_.variances) << "prior_box: input / image / boxes / variances must be set";
    CHECK_EQ(param_.input->dims().size(), 4UL) << "prior_box: Input must be [N, C, H, W]";
    CHECK_EQ(param_.image->dims().size(), 4UL) << "prior_box: Image must be [N, C, H, W]";
    return true;
  }
  bool InferShapeImpl() const override {
    CHECK(param_.prior_num > 0) << "prior_box: prior_num " << param_.prior_num;
    const auto d = param_.input->dims();
    const std::vector<int64_t> out{d[2], d[3], param_.prior_num, 4};
    param_.boxes->Resize(out);
    param_.variances->Resize(out);
    return true;
  }
  void AttachKernel(KernelBase* k) override { k->SetParam<PriorBoxParam>(param_); }

 private:
  mutable PriorBoxParam param_;
};

// box_coder_op.cc, decode_center_size: proposals take TargetBox's dims [rows, cols, 4]; PriorBox is [cols, 4] (axis 0) / [rows, 4]
class BoxCoderOpLite : public OpLite {
 public:
  BoxCoderOpLite() : OpLite("box_coder") {}
  BoxCoderParam& mutable_param() { return param_; }
  static void CheckDims(const std::vector<int64_t>& prior, const std::vector<int64_t>* prior_var, const std::vector<int64_t>& target, int axis) {
    CHECK(target.size() == 3 && target[2] == 4) << "box_coder: TargetBox must be [rows, cols, 4]";
    CHECK(axis == 0 || axis == 1) << "box_coder: axis " << axis;
    CHECK(prior.size() == 2 && prior[1] == 4 && prior[0] == target[1 - axis])
        << "box_coder: PriorBox must be [" << target[1 - axis] << ", 4] for axis " << axis;
    if (prior_var) CHECK(*prior_var == prior) << "box_coder: PriorBoxVar must have PriorBox's dims";
  }
  bool CheckShape() const override {
    CHECK(param_.prior_box && param_.target_box && param_.proposals) << "box_coder: prior_box / target_box / proposals must be set";
    return true;
  }
  bool InferShapeImpl() const override {
    CHECK(param_.code_type == "decode_center_size") << "box_coder: kHIP has decode_center_size only, not " << param_.code_type;
    CHECK(param_.variance.empty() || param_.variance.size() == 4) << "box_coder: the variance attribute has " << param_.variance.size() << " values";
    // a prior_box output [H, W, A, 4] is read as [H * W * A, 4]
    auto flat = [](const lite::Tensor* t) {
      auto d = t->dims().Vectorize();
      if (d.size() == 4) d = {d[0] * d[1] * d[2], d[3]};
      return d;
    };
    const auto pv = param_.prior_box_var ? flat(param_.prior_box_var) : std::vector<int64_t>{};
    CheckDims(flat(param_.prior_box), param_.prior_box_var ? &pv : nullptr, param_.target_box->dims().Vectorize(), param_.axis);
    param_.proposals->Resize(param_.target_box->dims());
    return true;
  }
  void AttachKernel(KernelBase* k) override { k->SetParam<BoxCoderParam>(param_); }

 private:
  mutable BoxCoderParam param_;
};

// yolo_box_op.cc:25-60: X [N, an * (5 + class_num), H, W], ImgSize int32 [N, 2]; Boxes [N, an * H * W, 4], Scores [N, an * H * W,
// class_num].  kHIP alias head (fusion P, lite/kernels/hip/yolo_fusion.h): further feature maps behind X; Boxes is [N, P, 4] and
// Scores [N, class_num, P] with P the sum over all maps.
class YoloBoxOpLite : public OpLite {
 public:
  YoloBoxOpLite() : OpLite("yolo_box") {}
  YoloBoxParam& mutable_param() { return param_; }
  struct Scale {
    const lite::Tensor* x;
    std::vector<int> anchors;
  };
  // kHIP fusion P only: Scores is [N, class_num, P]; a further feature map behind X
  void set_head() { head_ = true; }
  void add_scale(const lite::Tensor* x, const std::vector<int>& anchors) { more_.push_back({x, anchors}); }
  // YoloBoxOp::CheckShape on the operands' dims; returns the boxes of one image
  static int64_t CheckDims(const std::vector<int64_t>& x, const std::vector<int64_t>& img, const std::vector<int>& anchors, int class_num,
                           const std::string& who) {
    CHECK(x.size() == 4) << who << ": X must be [N, C, H, W], has rank " << x.size();
    CHECK(!anchors.empty() && anchors.size() % 2 == 0) << who << ": anchors must hold (width, height) pairs, has " << anchors.size() << " values";
    CHECK(class_num > 0) << who << ": class_num " << class_num << " must be positive";
    const int64_t an = static_cast<int64_t>(anchors.size() / 2);
    CHECK(x[1] == an * (5 + class_num)) << who << ": X has " << x[1] << " channels, " << an << " anchors of " << class_num << " classes need "
                                        << an * (5 + class_num);
    CHECK(img.size() == 2 && img[0] == x[0] && img[1] == 2) << who << ": ImgSize must be [" << x[0] << ", 2]";
    return an * x[2] * x[3];
  }
  bool CheckShape() const override {
    CHECK(param_.X && param_.ImgSize && param_.Boxes && param_.Scores) << "yolo_box: X / ImgSize / Boxes / Scores must be set";
    return true;
  }
  bool InferShapeImpl() const override {
    const auto img = param_.ImgSize->dims().Vectorize();
    const auto x = param_.X->dims().Vectorize();
    int64_t p = CheckDims(x, img, param_.anchors, param_.class_num, "yolo_box");
    for (auto& m : more_) p += CheckDims(m.x->dims().Vectorize(), img, m.anchors, param_.class_num, "yolo_box/head");
    param_.Boxes->Resize(std::vector<int64_t>{x[0], p, 4});
    if (head_) param_.Scores->Resize(std::vector<int64_t>{x[0], param_.class_num, p});
    else param_.Scores->Resize(std::vector<int64_t>{x[0], p, param_.class_num});
    return true;
  }
  void AttachKernel(KernelBase* k) override { k->SetParam<YoloBoxParam>(param_); }

 private:
  mutable YoloBoxParam param_;
  std::vector<Scale> more_;
  bool head_{false};
};

// multiclass_nms_op.cc, the 3-D score form.  kHIP: Out is [N, keep_top_k, 6] padded with -1, Index [N, keep_top_k], and the counts
// [N] go to the tensor set_count names (lite/kernels/hip/detection_fusion.h); scores_npc: the scores are [N, P, C] (fusion O2)
class MulticlassNmsOpLite : public OpLite {
 public:
  MulticlassNmsOpLite() : OpLite("multiclass_nms") {}
  MulticlassNmsParam& mutable_param() { return param_; }
  void set_count(lite::Tensor* t) { count_ = t; }
  void set_scores_npc(bool v) { scores_npc_ = v; }
  // fatal on what the kernel refuses; boxes [N, P, 4], scores [N, C, P] ([N, P, C] with npc)
  static void CheckCall(const std::vector<int64_t>& boxes, const std::vector<int64_t>& scores, bool npc, const MulticlassNmsParam& p) {
    CHECK(boxes.size() == 3 && boxes[2] == 4) << "multiclass_nms: BBoxes must be [N, P, 4]";
    CHECK(scores.size() == 3) << "multiclass_nms: kHIP takes the 3-D score form [N, C, P] only";
    const int64_t c = scores[npc ? 2 : 1], pr = scores[npc ? 1 : 2];
    CHECK(scores[0] == boxes[0] && pr == boxes[1]) << "multiclass_nms: BBoxes and Scores disagree in N or P";
    CHECK(p.keep_top_k > 0) << "multiclass_nms: keep_top_k " << p.keep_top_k << " must be positive on kHIP (it sizes the output)";
    CHECK(p.nms_eta >= 1.f) << "multiclass_nms: nms_eta < 1 (adaptive threshold) is outside the device kernel";
    const int64_t kmax = p.nms_top_k < 0 || p.nms_top_k > pr ? pr : p.nms_top_k;
    const int64_t cap = kmax < p.keep_top_k ? kmax : p.keep_top_k;
    const int64_t nact = c - (p.background_label >= 0 && p.background_label < c ? 1 : 0);
    CHECK(pr <= 16384 && kmax <= 4096 && nact * cap <= 16384 && boxes[0] <= 65535)
        << "multiclass_nms: N " << boxes[0] << " C " << c << " P " << pr << " nms_top_k " << p.nms_top_k << " keep_top_k " << p.keep_top_k
        << " is outside the device kernel's envelope (P <= 16384, min(nms_top_k, P) <= 4096, classes * min(nms_top_k, keep_top_k, P) <= 16384)";
  }
  bool CheckShape() const override {
    CHECK(param_.bboxes && param_.scores && param_.out) << "multiclass_nms: bboxes / scores / out must be set";
    return true;
  }
  bool InferShapeImpl() const override {
    const auto b = param_.bboxes->dims().Vectorize();
    CheckCall(b, param_.scores->dims().Vectorize(), scores_npc_, param_);
    param_.out->Resize(std::vector<int64_t>{b[0], param_.keep_top_k, 6});
    if (param_.index) param_.index->Resize(std::vector<int64_t>{b[0], param_.keep_top_k});
    if (count_) count_->Resize(std::vector<int64_t>{b[0]});
    return true;
  }
  void AttachKernel(KernelBase* k) override { k->SetParam<MulticlassNmsParam>(param_); }

 private:
  mutable MulticlassNmsParam param_;
  lite::Tensor* count_{nullptr};
  bool scores_npc_{false};
};

class SoftmaxOp : public OpLite {
 public:
  SoftmaxOp() : OpLite("softmax") {}
  SoftmaxParam& mutable_param() { return param_; }
  bool InferShapeImpl() const override {
    param_.output->Resize(param_.x->dims());
    return true;
  }
  void AttachKernel(KernelBase* k) override { k->SetParam<SoftmaxParam>(param_); }

 private:
  mutable SoftmaxParam param_;
};

}  // namespace operators
}  // namespace lite
}  // namespace paddle
