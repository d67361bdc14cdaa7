// image_frame.h — the two kHIP instructions in front of image_to_tensor when the caller feeds a decoder's or camera's FRAME (its own
// size, NV12 / NV21 or an interleaved format) instead of the network-sized image: ImagePreprocess::imageConvert and imageResize
// (lite/utils/cv/paddle_image_preprocess.cc:44-98 -> image_convert.cc, image_resize.cc) as instructions behind the io_copy of the
// frame's bytes.  Like image_to_tensor.h, the parameter structs live here and not in lite/operators/op_params.h: the reference has
// no such ops.  The graph builder emits them for a frame feed (GraphBuilder::FeedFrame); with the graph fusions on, image_resize
// takes the image_to_tensor behind it, the calib behind that and the image_convert in front over (fusion I, one launch).
#pragma once
#include <vector>

#include "lite/kernels/hip/image_to_tensor.h"

namespace paddle {
namespace lite {
namespace operators {

inline bool FrameIsNV(int format) { return format == PLHIP_IMG_NV12 || format == PLHIP_IMG_NV21; }
inline const char* FrameFormatName(int format) {
  return format == PLHIP_IMG_NV12 ? "NV12" : format == PLHIP_IMG_NV21 ? "NV21" : ImageFormatName(format);
}
// dims of the host / device variable that holds a frame: NV [n, h * 3 / 2, w], interleaved [n, h, w, cs]
inline std::vector<int64_t> FrameDims(int n, int h, int w, int format) {
  if (FrameIsNV(format)) return {n, h / 2 * 3, w};
  return {n, h, w, ImagePixelBytes(format)};
}

struct ImageConvertParam {
  const lite::Tensor* x{nullptr};  // uint8 NV12 / NV21 frame [n, h * 3 / 2, w], device
  lite::Tensor* output{nullptr};   // uint8 [n, h, w, 3 | 4]
  int src_format{PLHIP_IMG_NV12};
  int dst_format{PLHIP_IMG_BGR};   // BGR, or BGRA (4th byte 255)
};

class ImageConvertOp : public OpLite {
 public:
  ImageConvertOp() : OpLite("image_convert") {}
  ImageConvertParam& mutable_param() { return param_; }
  bool CheckShape() const override {
    CHECK(param_.x && param_.output) << "image_convert: x / output must be set";
    CHECK(FrameIsNV(param_.src_format)) << "image_convert: the source must be NV12 / NV21";
    CHECK(param_.dst_format == PLHIP_IMG_BGR || param_.dst_format == PLHIP_IMG_BGRA) << "image_convert: an NV frame converts to BGR / BGRA only";
    CHECK_EQ(param_.x->dims().size(), 3UL) << "image_convert: the frame must be [n, h * 3 / 2, w]";
    CHECK(param_.x->dims()[1] % 3 == 0 && param_.x->dims()[2] % 2 == 0) << "image_convert: an NV frame needs even w and h";
    return true;
  }
  bool InferShapeImpl() const override {
    const auto d = param_.x->dims();
    param_.output->Resize(std::vector<int64_t>{d[0], d[1] / 3 * 2, d[2], ImagePixelBytes(param_.dst_format)});
    return true;
  }
  void AttachKernel(KernelBase* k) override { k->SetParam<ImageConvertParam>(param_); }

 private:
  mutable ImageConvertParam param_;
};

struct ImageResizeParam {
  const lite::Tensor* x{nullptr};  // uint8 frame (FrameDims), device
  lite::Tensor* output{nullptr};   // uint8 [n, out_h, out_w, cs]; with to_tensor: fp32 NCHW [n, c, out_h, out_w], or int8 with int8_out
  int format{PLHIP_IMG_BGR};       // the frame's: an interleaved plhip_image_format, or NV12 / NV21 (converted tap by tap, resized as BGR)
  int out_h{0}, out_w{0};
  bool to_tensor{false};           // the image_to_tensor behind it folded in (means / scales below) ...
  float means[3]{0.f, 0.f, 0.f};
  float scales[3]{1.f, 1.f, 1.f};
  bool int8_out{false};            // ... and the calib[fp32_to_int8] behind that (its scale below)
  float calib_scale{1.f};
};

class ImageResizeOp : public OpLite {
 public:
  ImageResizeOp() : OpLite("image_resize") {}
  ImageResizeParam& mutable_param() { return param_; }
  bool CheckShape() const override {
    CHECK(param_.x && param_.output) << "image_resize: x / output must be set";
    const bool nv = FrameIsNV(param_.format);
    CHECK(nv || (param_.format >= PLHIP_IMG_RGBA && param_.format <= PLHIP_IMG_GRAY)) << "image_resize: unsupported frame format " << param_.format;
    CHECK_EQ(param_.x->dims().size(), nv ? 3UL : 4UL) << "image_resize: the frame must be [n, h, w, cs] ([n, h * 3 / 2, w] for NV12 / NV21)";
    CHECK(param_.out_h > 0 && param_.out_w > 0) << "image_resize: bad output size";
    CHECK(!param_.int8_out || param_.to_tensor) << "image_resize: int8_out needs to_tensor";
    return true;
  }
  bool InferShapeImpl() const override {
    const int fmt = FrameIsNV(param_.format) ? static_cast<int>(PLHIP_IMG_BGR) : param_.format;
    const int64_t n = param_.x->dims()[0];
    if (param_.to_tensor) param_.output->Resize(std::vector<int64_t>{n, ImageChannels(fmt), param_.out_h, param_.out_w});
    else param_.output->Resize(std::vector<int64_t>{n, param_.out_h, param_.out_w, ImagePixelBytes(fmt)});
    return true;
  }
  void AttachKernel(KernelBase* k) override { k->SetParam<ImageResizeParam>(param_); }

 private:
  mutable ImageResizeParam param_;
};

}  // namespace operators
}  // namespace lite
}  // namespace paddle
