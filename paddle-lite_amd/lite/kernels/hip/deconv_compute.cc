// deconv_compute.cc — TARGET(kHIP) / PRECISION(kInt8) conv2d_transpose kernels, int8_out and fp32_out as conv2d has them.
//
// The reference's ARM kernel (lite/kernels/arm/conv_transpose_compute.cc) is fp32 only; the int8 semantics are its test oracle's
// deconv_basic<int8_t, int> (lite/tests/utils/naive_math_impl.h:538-635) with the GEMM-like conv's scale / bias / activation fold
// (quant_fold.h), indexed by output channel.  Reads ConvParam fields only (output_size among them, op_params.h): the file compiles
// against the reference's own struct text.  The weights are packed in PrepareForRun for the route plhip picks on the first shape
// (plhip_deconv_impl_name) and again when a resized feed changes the route.
#include <string>

#include "lite/core/kernel.h"
#include "lite/core/op_registry.h"
#include "lite/kernels/hip/conv_compute.h"
#include "lite/kernels/hip/packed_weight_cache.h"
#include "lite/kernels/hip/quant_fold.h"
#include "lite/operators/op_params.h"
#include "plhip.h"

namespace paddle {
namespace lite {
namespace kernels {
namespace hip {

template <PrecisionType OutType>
class ConvTransposeCompute : public KernelLite<TARGET(kHIP), PRECISION(kInt8)> {
 public:
  using param_t = operators::ConvParam;
  void PrepareForRun() override {
    auto& param = this->template Param<param_t>();
    CHECK(this->ctx_) << "SetContext must precede PrepareForRun";
    CHECK(!param.fuse_residual_connection) << "kHIP: conv2d_transpose has no fused tail";
    BuildDesc();
    const QuantFold f = FoldLayer(param.weight_scale, desc_.conv.cout, param.input_scale, param.output_scale, OutType == PRECISION(kInt8),
                                  param.bias, &param.activation_param, param.fuse_relu);
    desc_.conv.act = f.act;
    desc_.conv.act_alpha = f.alpha;
    folded_.has_bias = UploadFold(f, &folded_.scale, &folded_.bias);
    PackWeights();
    last_shape_ = param.x->dims();
  }
  void ReInitWhenNeeded() override {
    auto& param = this->template Param<param_t>();
    if (last_shape_ == param.x->dims()) return;
    BuildDesc();
    // the packed bytes belong to ONE route: a resized feed that changes it packs again (through the shared cache)
    if (packed_impl_ != plhip_deconv_impl_name(&desc_) || packed_bytes_ != plhip_deconv_packed_weight_bytes(&desc_)) PackWeights();
    last_shape_ = param.x->dims();
  }
  void Run() override {
    auto& param = this->template Param<param_t>();
    auto& ctx = this->ctx_->template As<HIPContext>();
    CHECK(param.x->target() == TARGET(kHIP)) << "conv2d_transpose input must live on the HIP device (io_copy missing?)";
    constexpr bool kInt8Out = OutType == PRECISION(kInt8);
    void* y = kInt8Out ? static_cast<void*>(param.output->template mutable_data<int8_t>(TARGET(kHIP)))
                       : static_cast<void*>(param.output->template mutable_data<float>(TARGET(kHIP)));
    HIP_CALL(ctx.ctx(), plhip_conv2d_transpose_int8(ctx.ctx(), &desc_, param.x->template data<int8_t>(), folded_.weights->raw_data(), folded_.sc(),
                                                    folded_.bi(), y, kInt8Out ? PLHIP_OUT_I8 : PLHIP_OUT_F32));
  }
  void SetProfileRuntimeKernelInfo(profile::OpCharacter* ch) override { ch->kernel_func_name = packed_impl_; }

 private:
  void BuildDesc() {  // the shape part of desc_; its activation is the fold's (PrepareForRun)
    auto& param = this->template Param<param_t>();
    const auto x = param.x->dims(), w = param.filter->dims();
    CHECK_EQ(x.size(), 4UL);
    CHECK_EQ(w.size(), 4UL);
    CHECK(param.paddings && param.paddings->size() == 4UL) << "paddings must be {top, bottom, left, right}";
    CHECK(param.dilations && param.dilations->size() == 2UL);
    CHECK(param.output_size.empty() || param.output_size.size() == 2UL) << "output_size must have 0 or 2 entries";
    auto& d = desc_.conv;
    d.n = static_cast<int>(x[0]);
    d.cin = static_cast<int>(x[1]);
    d.h = static_cast<int>(x[2]);
    d.w = static_cast<int>(x[3]);
    d.cout = static_cast<int>(w[1]) * param.groups;  // filter [cin][cout / groups][kh][kw]
    d.kh = static_cast<int>(w[2]);
    d.kw = static_cast<int>(w[3]);
    for (int i = 0; i < 4; ++i) d.pad[i] = (*param.paddings)[i];
    d.stride[0] = param.strides[0];
    d.stride[1] = param.strides[1];
    d.dil[0] = (*param.dilations)[0];
    d.dil[1] = (*param.dilations)[1];
    d.groups = param.groups;
    desc_.out_h = param.output_size.empty() ? 0 : param.output_size[0];
    desc_.out_w = param.output_size.empty() ? 0 : param.output_size[1];
    int oh = 0, ow = 0;
    CHECK(plhip_deconv_out_dims(&desc_, &oh, &ow) == PLHIP_OK) << "invalid conv2d_transpose configuration: " << plhip_last_error(nullptr);
  }
  void PackWeights() {
    auto& param = this->template Param<param_t>();
    packed_impl_ = plhip_deconv_impl_name(&desc_);
    packed_bytes_ = plhip_deconv_packed_weight_bytes(&desc_);
    CHECK_GT(packed_bytes_, 0UL) << "invalid conv2d_transpose configuration";
    std::string layout = packed_impl_;
    const auto wd = param.filter->dims();
    for (size_t i = 0; i < wd.size(); ++i) layout += "_" + std::to_string(wd[i]);
    layout += "_g" + std::to_string(desc_.conv.groups);
    auto* ctx = &this->ctx_->template As<HIPContext>();
    folded_.weights = PackThroughCache(ctx, param.filter, layout, packed_bytes_, [&](const int8_t* w_dev, void* d) {
      HIP_CALL(ctx->ctx(), plhip_pack_deconv_weights(ctx->ctx(), &desc_, w_dev, d));
    });
  }

  plhip_deconv_desc desc_{};
  FoldedConv folded_;  // the weights, folded scale and bias on the device (its own desc is not used: desc_ carries the shape)
  DDim last_shape_;
  std::string packed_impl_{"NotImplForConvTranspose"};
  size_t packed_bytes_{0};
};

}  // namespace hip
}  // namespace kernels
}  // namespace lite
}  // namespace paddle

typedef paddle::lite::kernels::hip::ConvTransposeCompute<PRECISION(kInt8)> ConvTransposeInt8_Int8;
typedef paddle::lite::kernels::hip::ConvTransposeCompute<PRECISION(kFloat)> ConvTransposeInt8_Fp32;

REGISTER_LITE_KERNEL(conv2d_transpose, kHIP, kInt8, kNCHW, ConvTransposeInt8_Int8, int8_out)
    .BindInput("Input", {LiteType::GetTensorTy(TARGET(kHIP), PRECISION(kInt8))})
    .BindInput("Bias", {LiteType::GetTensorTy(TARGET(kHIP), PRECISION(kFloat))})
    .BindInput("Filter", {LiteType::GetTensorTy(TARGET(kHIP), PRECISION(kInt8))})
    .BindOutput("Output", {LiteType::GetTensorTy(TARGET(kHIP), PRECISION(kInt8))})
    .Finalize();

REGISTER_LITE_KERNEL(conv2d_transpose, kHIP, kInt8, kNCHW, ConvTransposeInt8_Fp32, fp32_out)
    .BindInput("Input", {LiteType::GetTensorTy(TARGET(kHIP), PRECISION(kInt8))})
    .BindInput("Bias", {LiteType::GetTensorTy(TARGET(kHIP), PRECISION(kFloat))})
    .BindInput("Filter", {LiteType::GetTensorTy(TARGET(kHIP), PRECISION(kInt8))})
    .BindOutput("Output", {LiteType::GetTensorTy(TARGET(kHIP), PRECISION(kFloat))})
    .Finalize();
