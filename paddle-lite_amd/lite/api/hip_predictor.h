// hip_predictor.h — a mini CxxPredictor for the kHIP target: a name->Tensor scope plus a RuntimeProgram of
// {OpLite, KernelBase} instructions built in code (the model parser and MIR optimiser of the reference are out of
// scope — SURVEY.md §2).  What it does restate from the reference's build pipeline:
//   * kernel choice by (op_type, Place{kHIP, precision, layout}, alias) through KernelFactory, with the
//     static_kernel_pick rule for enable_int8 ops: alias int8_out iff the consumer is int8, else fp32_out
//     (lite/core/mir/static_kernel_pick_pass.cc:92-165) — the caller states which;
//   * io_copy between host and device tensors (type_target_cast_pass) and calib on precision edges
//     (type_precision_cast_pass);
//   * one KernelContext per instruction from NewContext(target) (runtime_context_assign_pass);
//   * Run() = for inst: InferShape(); Launch()   (program.cc:265-315, 436-467).
#pragma once
#include <map>
#include <memory>
#include <string>
#include <vector>

#include "lite/core/op_registry.h"
#include "lite/core/program.h"

namespace paddle {
namespace lite {

std::unique_ptr<KernelBase> PickKernel(const std::string& op_type, const Place& place, const std::string& alias);

struct ConvAttrs {
  std::vector<int> strides{1, 1}, paddings{0, 0, 0, 0}, dilations{1, 1};
  int groups{1};
  int act{0};            // lite_api::ActivationType value: 0, 1 relu, 2 relu6, 4 leaky
  float act_coef{0.f};   // Relu_clipped_coef or Leaky_relu_alpha
  float input_scale{1.f}, output_scale{1.f};
  std::vector<float> weight_scale;
  bool int8_out{true};
  std::string padding_algorithm{""};
  std::vector<int> output_size;  // conv2d_transpose only (ConvParam::output_size): empty, or {h, w}
  // kHIP fused tail of an fp32_out conv (op_params.h ConvParam, graph_builder.h): variable names, "" = none
  std::string residual, calib_out;
  bool residual_relu{false}, drop_fp32{false};
  float calib_scale{1.f};
  // kHIP fused 1x1 consumer of a depthwise conv (ConvParam::pw_*): `out` of AddConv is then the pointwise conv's output
  const int8_t* pw_w{nullptr};
  std::vector<int64_t> pw_w_dims;
  const float* pw_bias{nullptr};
  std::vector<float> pw_weight_scale;
  float pw_output_scale{1.f};
  bool pw_int8_out{true};
  int pw_act{0};
  float pw_act_coef{0.f};
  bool pw_pool{false};  // ... and the global average pool2d behind it: `out` is the pool's output, [n, cout, 1, 1] fp32
  bool pw_tail{false};  // fusion G: residual / calib_out / drop_fp32 above are the 1x1 conv's tail (its fp32 output)
  float in_calib_scale{0.f};  // kHIP: the calib[fp32_to_int8] in front taken over: `in` of AddConv is the calib's fp32 input (0 = none)
  // ... and the image_to_tensor in front of it (fusion H1): `in` of AddConv is then the uint8 image on the device, image_x the name
  // of the (never allocated) NCHW variable that carries its shape; format < 0 = none
  int image_format{-1};
  float image_means[3]{0.f, 0.f, 0.f}, image_scales[3]{1.f, 1.f, 1.f};
  std::string image_x;
};

class HipPredictor {
 public:
  explicit HipPredictor(int device_id) : device_(device_id) { TargetWrapperHip::SetDevice(device_id); }
  Tensor* Var(const std::string& name);
  bool HasVar(const std::string& name) const { return vars_.count(name) != 0; }

  // host tensor that the caller fills (feed) — fp32 or int8
  Tensor* AddFeed(const std::string& name, const std::vector<int64_t>& dims, PrecisionType prec);
  void AddIoCopy(const std::string& in, const std::string& out, bool host_to_device);
  void AddCalib(const std::string& in, const std::string& out, float scale, bool fp32_to_int8);
  // image_to_tensor (lite/kernels/hip/image_to_tensor.h): uint8 image [n, h, w, cs] on the device -> fp32 NCHW, or int8 with the
  // calib[fp32_to_int8](calib_scale) behind it folded in (calib_scale > 0)
  void AddImageToTensor(const std::string& in, const std::string& out, int format, const float* means, const float* scales,
                        float calib_scale);
  // image_convert / image_resize (lite/kernels/hip/image_frame.h): the frame feed's instructions.  AddImageResize: frame_format may be
  // NV12 / NV21 (converted in the same launch); means != nullptr folds the image_to_tensor behind it in, calib_scale > 0 the calib too
  void AddImageConvert(const std::string& in, const std::string& out, int src_format, int dst_format);
  void AddImageResize(const std::string& in, const std::string& out, int frame_format, int out_h, int out_w, const float* means,
                      const float* scales, float calib_scale);
  void AddConv(const std::string& op_type, const std::string& in, const std::string& out, const int8_t* w,
               const std::vector<int64_t>& w_dims, const float* bias, const ConvAttrs& attrs);
  // conv2d_transpose: w [cin][cout / groups][kh][kw], bias per output channel (cout = w_dims[1] * groups); of `attrs` the conv's
  // own fields and output_size are read, there is no fused form
  void AddConvTranspose(const std::string& in, const std::string& out, const int8_t* w, const std::vector<int64_t>& w_dims,
                        const float* bias, const ConvAttrs& attrs);
  void AddFc(const std::string& in, const std::string& out, const int8_t* w, int k, int n, const float* bias,
             float input_scale, const std::vector<float>& weight_scale, float output_scale, bool int8_out, bool relu);
  void AddGlobalAvgPool(const std::string& in, const std::string& out);
  void AddPool(const std::string& in, const std::string& out, const std::string& pooling_type, const std::vector<int>& ksize,
               const std::vector<int>& strides, const std::vector<int>& paddings, bool global_pooling, bool exclusive,
               bool ceil_mode, bool int8 = false);
  // act_type "" -> elementwise_add, "relu" -> fusion_elementwise_add_activation
  void AddElementwiseAdd(const std::string& x, const std::string& y, const std::string& out, const std::string& act_type);
  void AddSoftmax(const std::string& in, const std::string& out);
  // hard_swish / hard_sigmoid with the reference's default parameters (lite/operators/op_params.h:406-412), and
  // elementwise_mul (y: x's shape, or [N, C, 1, 1] / [N, C] at axis 0).  calib_out != "": the calib[fp32_to_int8](calib_scale)
  // behind the op runs in the same launch and writes that variable (fusions J1 / J3, lite/kernels/hip/calib_tail.h);
  // drop_fp32: `out` has no reader left and is not written.
  void AddActivation(const std::string& op_type, const std::string& in, const std::string& out, const std::string& calib_out = "",
                     float calib_scale = 1.f, bool drop_fp32 = false);
  // fusion J2: hard_sigmoid that took calib(calib_scale) -> conv 1x1 (w1 [cr, c, 1, 1], a1; int8 out at a2.input_scale) -> conv 1x1
  // (w2 [c, cr, 1, 1], a2; fp32 out) in front of it over: `in` is the pooled fp32 [N, C, 1, 1], `out` the gate
  void AddSeGate(const std::string& in, const std::string& out, float calib_scale, const int8_t* w1, const std::vector<int64_t>& w1_dims,
                 const float* bias1, const ConvAttrs& a1, const int8_t* w2, const std::vector<int64_t>& w2_dims, const float* bias2,
                 const ConvAttrs& a2);
  void AddElementwiseMul(const std::string& x, const std::string& y, const std::string& out, int axis, const std::string& calib_out = "",
                         float calib_scale = 1.f, bool drop_fp32 = false);
  // concat / split / shuffle_channel, fp32 ops with the reference's attributes (lite/operators/op_params.h:369-386, 590-608,
  // 258-263).  AddSplit: num > 0 = equal parts, else `sections`, one per output.
  void AddConcat(const std::vector<std::string>& inputs, const std::string& out, int axis);
  // fusion L (lite/kernels/hip/calib_tail.h): concat -> calib[fp32_to_int8](calib_scale) in ONE launch, concat/int8.  `out` names
  // the fp32 tensor, calib_out its int8 image; drop_fp32: `out` has no reader left and is not written (it carries the shape).
  void AddConcatCalib(const std::vector<std::string>& inputs, const std::string& out, int axis, const std::string& calib_out,
                      float calib_scale, bool drop_fp32);
  void AddSplit(const std::string& in, const std::vector<std::string>& outs, int axis, int num, const std::vector<int>& sections);
  void AddShuffleChannel(const std::string& in, const std::string& out, int group);
  // fusion K (lite/kernels/hip/shuffle_fusion.h): concat([a, b], axis 1) -> shuffle_channel(2) and what follows, ONE launch.
  // lo == "": K2, shuffle_channel/int8: `hi` names the shuffled fp32 tensor, calib_out its int8 image.  lo != "": K1,
  // shuffle_channel/unit: `lo` / `hi` name the two halves of the split behind the shuffle, calib_out the int8 image of `hi`.
  // drop_fp32: `hi` has no reader left and is not written.
  void AddShuffleUnit(const std::string& a, const std::string& b, const std::string& lo, const std::string& hi,
                      const std::string& calib_out, float calib_scale, bool drop_fp32);
  // bilinear_interp / nearest_interp and arg_max with the reference's attributes (lite/operators/op_params.h:154-168, 821-827); the
  // output size is out_h x out_w where both are > 0, else int(in * scale).  calib_out != "": fusion N (lite/kernels/hip/
  // calib_tail.h), the calib[fp32_to_int8](calib_scale) behind the interp runs in the same launch and writes that variable;
  // drop_fp32: `out` has no reader left and is not written (it carries the shape).
  void AddInterp(const std::string& op_type, const std::string& in, const std::string& out, int out_h, int out_w, float scale,
                 bool align_corners, int align_mode, const std::string& calib_out = "", float calib_scale = 1.f, bool drop_fp32 = false);
  void AddArgMax(const std::string& in, const std::string& out, int axis, int dtype, bool keepdims);
  // fusion M: interp -> arg_max(axis 1) in ONE launch, arg_max/interp.  `in` is the interp's low-resolution input, `out` the labels;
  // the resampled tensor is no variable of the program.
  void AddInterpArgMax(const std::string& op_type, const std::string& in, const std::string& out, int out_h, int out_w, float scale,
                       bool align_corners, int align_mode, int dtype, bool keepdims);

  // detection heads (lite/kernels/hip/detection_compute.cc) with the reference's attributes (lite/operators/op_params.h:342, 617, 880,
  // 910, 941).  AddReshape launches nothing: `out` shares `in`'s memory.  AddPriorBox computes on the host once per shape.
  void AddTranspose(const std::string& in, const std::string& out, const std::vector<int>& perm);
  void AddReshape(const std::string& in, const std::string& out, const std::vector<int>& shape);
  void AddPriorBox(const std::string& input, const std::string& image, const std::string& boxes, const std::string& variances,
                   const std::vector<float>& min_sizes, const std::vector<float>& max_sizes, const std::vector<float>& aspect_ratios,
                   const std::vector<float>& variance, bool flip, bool clip, float step_w, float step_h, float offset,
                   bool min_max_aspect_ratios_order);
  // decode_center_size; prior_var "" = none: then `variance` (4 values, or empty = none)
  void AddBoxCoder(const std::string& prior, const std::string& prior_var, const std::string& target, const std::string& out,
                   const std::vector<float>& variance, int axis, bool normalized);
  // out [N, keep_top_k, 6] padded with -1; the per-image counts go to the int32 variable "<out>/count"; index "" = none, else
  // [N, keep_top_k] int32.  scores_npc: `scores` is [N, P, C] (fusion O2: the transpose in front of it folded away)
  // yolo_box: x [N, an * (5 + class_num), H, W], img_size an int32 [N, 2] variable; boxes [N, an * H * W, 4], scores [N, an * H * W, class_num]
  void AddYoloBox(const std::string& x, const std::string& img_size, const std::string& boxes, const std::string& scores,
                  const std::vector<int>& anchors, int class_num, float conf_thresh, int downsample_ratio, bool clip_bbox, float scale_x_y);
  // fusion P, yolo_box/head: the feature maps xs[i] with anchors[i] and downsample_ratios[i] in one launch; boxes [N, P, 4], scores
  // [N, class_num, P], P the sum over the maps
  void AddYoloHead(const std::vector<std::string>& xs, const std::string& img_size, const std::string& boxes, const std::string& scores,
                   const std::vector<std::vector<int>>& anchors, int class_num, float conf_thresh, const std::vector<int>& downsample_ratios,
                   bool clip_bbox, float scale_x_y);
  void AddMulticlassNms(const std::string& boxes, const std::string& scores, const std::string& out, const std::string& index,
                        int background_label, float score_threshold, int nms_top_k, float nms_threshold, float nms_eta, int keep_top_k,
                        bool normalized, bool scores_npc = false);
  // fusion O1 (lite/kernels/hip/detection_fusion.h): transpose(0,2,3,1) -> reshape([0,-1,k]) -> concat(axis 1) of NCHW heads in ONE launch
  void AddConcatNhwc(const std::vector<std::string>& inputs, const std::string& out, int k);

  void Run(bool skip_io_copy = false) {
    TargetWrapperHip::SetDevice(device_);
    program_.Run(skip_io_copy);
  }
  // Replays the device part of the program (everything but the io_copy instructions) as ONE launch graph: recorded on
  // the first call (the program must have run once before: PrepareForRun, workspace), replayed afterwards.  Feeds and
  // fetches keep their device addresses, so new input is a plain copy into the feed's device tensor before the call.
  void RunGraph();
  ~HipPredictor();
  // The predictor's execution state (device stream + workspace): the creating thread's default state at the first
  // instruction (after pllite_adopt_stream: the adopted stream), kept for life — Run() from any thread uses it.
  const std::shared_ptr<HipExecState>& state();
  void Sync() { state()->Sync(); }
  RuntimeProgram& program() { return program_; }
  std::vector<std::string> KernelNames();

 private:
  void Emit(std::shared_ptr<OpLite> op, std::unique_ptr<KernelBase> kernel);
  Tensor* NewParam(const void* host, size_t bytes, const std::vector<int64_t>& dims, PrecisionType prec);
  // the int8 filter `w` and, bias != nullptr, the `cout` fp32 bias values of a conv as persistable host tensors
  void UploadWeights(const int8_t* w, const std::vector<int64_t>& w_dims, const float* bias, int64_t cout, Tensor** filter, Tensor** bias_out);
  int device_;
  std::shared_ptr<HipExecState> state_;
  void* graph_exec_{nullptr};  // plhip launch graph of the program (RunGraph)
  size_t graph_key_{0};        // what the recorded graph depends on: shapes of every variable, instruction count, workspace arena
  bool graph_stale_{false};    // AddFeed since the recording: addresses GraphKey does not see may have changed (RunGraph records again)
  size_t GraphKey() const;
  std::map<std::string, std::unique_ptr<Tensor>> vars_;
  std::vector<std::unique_ptr<Tensor>> params_;
  RuntimeProgram program_;
};

}  // namespace lite
}  // namespace paddle
