// image_to_tensor.h — the kHIP instruction that turns the caller's decoded uint8 image into the program's input tensor on the
// device: ImagePreprocess::image_to_tensor (lite/utils/cv/paddle_image_preprocess.h:217-244, .cc:143-172 -> image2tensor.cc) run
// as the first instruction after the io_copy of the image's bytes, instead of on the host in front of the feed.
//
// Its parameter struct lives here and NOT in lite/operators/op_params.h, which stays a field-for-field subset of the reference's:
// the reference has no such op (its image step is a host utility, not an instruction).  The graph builder emits it for an image
// feed (GraphBuilder::FeedImage); with the graph fusions on, the calib[fp32_to_int8] behind it folds in (the int8 form, fusion H2),
// or both fold into the 3x3 stem conv that reads the image itself (HipConvFusion::image_input, fusion H1).
#pragma once
#include <vector>

#include "lite/core/op_lite.h"
#include "plhip.h"

namespace paddle {
namespace lite {
namespace operators {

struct ImageToTensorParam {
  const lite::Tensor* x{nullptr};  // uint8 [n, h, w, cs], device
  lite::Tensor* output{nullptr};   // fp32 NCHW [n, c, h, w], or int8 with int8_out
  int format{PLHIP_IMG_BGR};       // plhip_image_format == cv::ImageFormat
  float means[3]{0.f, 0.f, 0.f};   // indexed by the source byte of a pixel (image2tensor.cc:279-284)
  float scales[3]{1.f, 1.f, 1.f};
  bool int8_out{false};            // the calib[fp32_to_int8] behind it folded in (its scale below)
  float calib_scale{1.f};
};

inline int ImagePixelBytes(int format) { return format == PLHIP_IMG_GRAY ? 1 : (format == PLHIP_IMG_RGB || format == PLHIP_IMG_BGR) ? 3 : 4; }
inline int ImageChannels(int format) { return format == PLHIP_IMG_GRAY ? 1 : 3; }
inline const char* ImageFormatName(int format) {
  static const char* names[] = {"RGBA", "BGRA", "RGB", "BGR", "GRAY"};
  return format >= 0 && format <= 4 ? names[format] : "?";
}
// the NCHW shape of the tensor made from an image of dims [n, h, w, cs]
inline std::vector<int64_t> ImageTensorDims(const DDim& img, int format) { return {img[0], ImageChannels(format), img[1], img[2]}; }

class ImageToTensorOp : public OpLite {
 public:
  ImageToTensorOp() : OpLite("image_to_tensor") {}
  ImageToTensorParam& mutable_param() { return param_; }
  bool CheckShape() const override {
    CHECK(param_.x && param_.output) << "image_to_tensor: x / output must be set";
    CHECK(param_.format >= PLHIP_IMG_RGBA && param_.format <= PLHIP_IMG_GRAY) << "image_to_tensor: unsupported image format " << param_.format;
    CHECK_EQ(param_.x->dims().size(), 4UL) << "image_to_tensor: the image must be [n, h, w, cs]";
    CHECK_EQ(param_.x->dims()[3], ImagePixelBytes(param_.format)) << "image_to_tensor: bytes per pixel do not match the format";
    return true;
  }
  bool InferShapeImpl() const override {
    param_.output->Resize(ImageTensorDims(param_.x->dims(), param_.format));
    return true;
  }
  void AttachKernel(KernelBase* k) override { k->SetParam<ImageToTensorParam>(param_); }

 private:
  mutable ImageToTensorParam param_;
};

}  // namespace operators
}  // namespace lite
}  // namespace paddle
