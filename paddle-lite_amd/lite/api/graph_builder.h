// graph_builder.h — from an op list "as the optimiser sees it after the fusion passes" to the kHIP RuntimeProgram.
//
// The reference builds its program with ~60 MIR passes; the model parser and the generic optimiser are
// out of scope.  What decides WHICH int8 kernels run and WHERE precision casts sit is restated here, in the order the
// reference applies it (lite/api/cxx_api.cc / lite/core/optimizer.h pass list):
//   1. static_kernel_pick_pass (lite/core/mir/static_kernel_pick_pass.cc:92-165): an enable_int8 op takes the
//      int8-output kernel iff EVERY consumer of its output is enable_int8, and then inherits the first consumer's
//      input scale as its output scale; otherwise the fp32-output kernel.
//   2. type_target_cast_pass: io_copy host->device behind every feed, device->host in front of every fetch.
//   3. type_precision_cast_pass (lite/core/mir/type_precision_cast_pass.cc:60-100, 130-260): where a consumer's declared
//      input precision differs from the tensor's, a calib op is inserted; one calib per source tensor, shared by later
//      consumers (`cast_nodes`); its scale is the consumer's input scale (fp32->int8) or the producer's output scale
//      (int8->fp32); its output is named "<var>/precision_trans".
// Ops arrive in topological order with the conv+bn, conv+activation, fc and elementwise_add+activation fusions already
// applied (the model loader, lite/model_parser of this repo, does the weight-side part of those).
#pragma once
#include <map>
#include <memory>
#include <string>
#include <vector>

#include "lite/api/hip_predictor.h"

namespace paddle {
namespace lite {

struct GraphOp {
  std::string type;  // conv2d | depthwise_conv2d | conv2d_transpose (w [cin][cout / groups][kh][kw], conv.output_size) | fc | pool2d | elementwise_add | fusion_elementwise_add_activation | softmax |
                     // hard_swish | hard_sigmoid | elementwise_mul (fp32 ops like pool2d; the reference's default parameters) |
                     // concat (N inputs) | split | shuffle_channel (fp32 ops like pool2d) |
                     // bilinear_interp | nearest_interp | arg_max (fp32 ops like pool2d; arg_max writes int64 / int32 labels) |
                     // transpose | reshape | prior_box | box_coder | multiclass_nms (fp32 ops like pool2d) |
                     // yolo_box (an fp32 op like box_coder whose second operand is an int32 feed)
  std::vector<std::string> inputs;
  std::string output;                // the first output
  std::vector<std::string> outputs;  // split: all outputs, outputs[0] == output; prior_box: {Boxes, Variances}; multiclass_nms:
                                     // {Out, "<Out>/count"[, Index]}; yolo_box: {Boxes, Scores}; empty for every other type
  bool enable_int8{false};
  // conv2d / depthwise_conv2d / fc
  std::vector<int8_t> w;
  std::vector<int64_t> w_dims;
  std::vector<float> bias;
  bool has_bias{false};
  ConvAttrs conv;  // input_scale, weight_scale, act, strides ...; output_scale / int8_out are set by Lower()
  bool fc_relu{false};
  // pool2d
  std::string pooling_type{"max"};
  std::vector<int> ksize{1, 1}, pool_strides{1, 1}, pool_paddings{0, 0, 0, 0};
  bool global_pooling{false}, exclusive{true}, ceil_mode{false};
  // fusion_elementwise_add_activation
  std::string act_type;
  // elementwise_mul: inputs {X [N, C, H, W], Y [N, C, 1, 1] | [N, C] | X's shape}; concat / split: the axis (negative: from the back)
  int axis{-1};
  // split: num > 0 = equal parts, else sections (one per output): lite/operators/split_op.cc:32-75
  int num{0};
  std::vector<int> sections;
  // shuffle_channel
  int group{1};
  // bilinear_interp / nearest_interp (InterpolateParam): the output is out_h x out_w where both are > 0, else int(in * interp_scale)
  int out_h{-1}, out_w{-1};
  float interp_scale{0.f};
  bool align_corners{true};
  int align_mode{1};
  // arg_max (ArgmaxParam): along `axis`; dtype -1 / 3 int64 labels, 2 int32
  int dtype{-1};
  bool keepdims{false};
  // transpose: axis k of the output is axis perm[k] of the input; reshape: the shape attribute (0 copies a dim, one -1 is inferred)
  std::vector<int> perm, shape;
  // prior_box (PriorBoxParam): inputs {Input, Image}, outputs {Boxes, Variances}, each [H, W, prior_num, 4]
  std::vector<float> min_sizes, max_sizes, aspect_ratios, variances;
  bool flip{true}, clip{false}, min_max_aspect_ratios_order{false};
  float step_w{0.f}, step_h{0.f}, offset{0.5f};
  // box_coder, decode_center_size (BoxCoderParam): inputs {PriorBox, TargetBox} or {PriorBox, PriorBoxVar, TargetBox}; without a
  // PriorBoxVar the 4 values of `variances` (or none); along `axis` (0 | 1)
  bool box_normalized{true};
  // multiclass_nms (MulticlassNmsParam): inputs {BBoxes [N, P, 4], Scores [N, C, P]}
  int background_label{0}, nms_top_k{-1}, keep_top_k{-1};
  float score_threshold{0.f}, nms_threshold{0.3f}, nms_eta{1.f};
  bool nms_normalized{true};
  // yolo_box (YoloBoxParam): inputs {X [N, an * (5 + class_num), H, W], ImgSize int32 [N, 2]}, outputs {Boxes [N, an * H * W, 4],
  // Scores [N, an * H * W, class_num]}
  std::vector<int> anchors;
  int class_num{0}, downsample_ratio{0};
  float conf_thresh{0.f}, scale_x_y{1.f};
  bool clip_bbox{true};
};

class GraphBuilder {
 public:
  void Feed(const std::string& name, const std::vector<int64_t>& dims, PrecisionType prec);
  // A feed the caller fills with a decoded uint8 image [n, h, w, cs] (format: plhip_image_format == cv::ImageFormat; means / scales
  // indexed by the source byte of a pixel) instead of the normalised tensor: ImagePreprocess::image_to_tensor
  // (lite/utils/cv/paddle_image_preprocess.h:217-244) moves onto the device.  The ops name `name` as the fp32 NCHW tensor
  // [n, c, h, w] (c = 1 for GRAY, else 3); lowering emits io_copy of the bytes, then image_to_tensor ("<name>/tensor").  With
  // set_fuse(true): (H1) image_to_tensor -> its only reader calib[fp32_to_int8] -> a 3x3 stride-2 stem plhip_conv2d_image_supported
  // takes  => ONE conv instruction reading the image (plhip_conv2d_image_int8); (H2) otherwise image_to_tensor and its only-reader
  // calib => one image_to_tensor/int8 instruction.
  void FeedImage(const std::string& name, int n, int h, int w, int format, const float* means, const float* scales);
  // A feed the caller fills with a decoder's or camera's FRAME: n frames of src_h x src_w in src_format, an interleaved
  // plhip_image_format ([n, src_h, src_w, cs] bytes) or PLHIP_IMG_NV12 / NV21 ([n, src_h * 3 / 2, src_w] bytes, even sizes), brought
  // to the network's dst_h x dst_w on the device: ImagePreprocess::imageConvert -> imageResize -> image_to_tensor
  // (lite/utils/cv/paddle_image_preprocess.cc:44-172).  The ops name `name` as the fp32 NCHW tensor [n, c, dst_h, dst_w] exactly as
  // with FeedImage (means / scales indexed by the byte of the image that is normalised: b, g, r for an NV frame).  Lowering:
  // io_copy -> image_convert "<name>/bgr" (NV only) -> image_resize "<name>/image" (omitted when the sizes are equal) ->
  // image_to_tensor "<name>/tensor".  With set_fuse(true), (I), in front of H: image_resize takes the image_to_tensor behind it, the
  // image_convert in front and, where it is the only reader (H2's condition), the calib[fp32_to_int8] over => ONE instruction, one
  // launch; H1 does not apply to a resized feed (the stem reads the int8 tensor).  Equal sizes and an interleaved format: FeedImage.
  void FeedFrame(const std::string& name, int n, int src_h, int src_w, int src_format, int dst_h, int dst_w, const float* means,
                 const float* scales);
  void Fetch(const std::string& name) { fetches_.push_back(name); }
  // Graph-level fusions of the kHIP target on top of the reference's program (default on; results are bit-identical to
  // the unfused program, every fused value is rounded as the separate instructions round it):
  //   conv2d[fp32_out] -> elementwise_add | fusion_elementwise_add_activation(relu) -> calib   => ONE conv launch
  //   conv2d[fp32_out] -> pool2d(max) -> calib                                  => conv + fused calib, int8 max pool
  void set_fuse(bool on) { fuse_ = on; }
  //   depthwise_conv2d[int8_out] -> conv2d 1x1 (stride 1, no padding, groups 1, no fused tail), sole consumer  => ONE instruction
  // Default (mode 2): only the pairs the fused kernel takes (plhip_dwpw_fused_supported on the shapes propagated from the
  // feeds: one launch, the int8 tensor between the two convs never leaves the CU — DESIGN.md 8); set_fuse_dwpw(true) = mode 1
  // takes every eligible pair over (shapes outside the kernel run as two launches inside the one instruction), false = off.
  void set_fuse_dwpw(bool on) { fuse_dwpw_ = on ? 1 : 0; }
  void set_fuse_dwpw_mode(int mode) { fuse_dwpw_ = mode; }
  //   (G) depthwise_conv2d[int8_out] -> conv2d 1x1 (stride 1, no padding, groups 1) WITH the 1x1 conv's fused tail (residual add,
  // calib copy, dropped fp32 output), sole consumer  => ONE instruction, one launch of plhip_dw_conv1x1_fused_int8.  Opt-in
  // (default off): runs with set_fuse(true) only, after D / E / F, on the pairs D left alone, where
  // plhip_dw_conv1x1_fused_supported takes the shapes propagated from the feeds.  MobileNetV2's 17 block pairs.
  void set_fuse_dwconv(bool on) { fuse_dwconv_ = on; }
  //   (J1) hard_swish -> calib[fp32_to_int8]      => ONE hard_swish/int8 instruction (plhip_hard_act_f32, both outputs when the
  //        fp32 value has other readers: the pool and the multiply of a squeeze-excite block)
  //   (J2) pool2d(avg, global) -> calib -> conv2d 1x1 [int8_out] -> conv2d 1x1 [fp32_out] -> hard_sigmoid, each the only reader
  //        of the one before, where plhip_se_gate_supported takes C, Cr and the activations
  //        => pool2d + ONE hard_sigmoid/se_gate instruction (plhip_se_gate_int8); otherwise the separate instructions stay
  //   (J3) elementwise_mul -> calib[fp32_to_int8] => ONE elementwise_mul/int8 instruction (plhip_se_scale_f32); the fp32 product
  //        is not written when the calib was its only reader
  // With set_fuse(true) only; bit-identical to the instructions they replace (the quantiser is calib's own).  DEFAULT OFF: none of
  // the three has been measured against the launches it replaces, as 8.5 keeps fusion G off.
  void set_fuse_hard_act(bool on) { fuse_hard_act_ = on; }
  //   (K1) concat(axis 1, two inputs of equal channels h) -> shuffle_channel(group 2) -> split(axis 1, two equal parts), each the
  //        only reader of the one before, where a calib[fp32_to_int8] reads the split's second output
  //        => ONE shuffle_channel/unit instruction (plhip_shuffle_unit_f32): the first half fp32, the second half int8 and, only
  //        where it has another reader, fp32
  //   (K2) the same concat -> shuffle_channel(group 2), whose output a calib[fp32_to_int8] reads
  //        => ONE shuffle_channel/int8 instruction; the fp32 tensor is not written when the calib was its only reader
  // Anything else (three inputs, unequal channels, another group, unequal sections, an intermediate that is fetched or read
  // elsewhere) keeps the separate instructions.  With set_fuse(true) only; bit-identical to the instructions they replace (values
  // are moved, the quantiser is calib's own).  DEFAULT ON: measured faster than the separate instructions by far more than the
  // run-to-run spread; no program without a concat changes.
  void set_fuse_shuffle(bool on) { fuse_shuffle_ = on; }
  //   (L) a concat (any axis, any number of inputs) that K did not take.  D: the calib[fp32_to_int8] that reads its output (at most
  //       one per variable).  P: every pool2d(max, not global) reader of that output whose own output only a calib[fp32_to_int8]
  //       reads (so it is not fetched).
  //   (L1) D exists => the concat step becomes ONE concat/int8 instruction (plhip_concat_calib_f32) that writes D's tensor at D's
  //        scale; D disappears.
  //   (L2) a pool of P whose calib has bitwise D's scale becomes an int8 max pool that reads the int8 copy and writes its calib's
  //        tensor (max commutes with the monotonic quantiser, as in C); that calib disappears.  Without D, where every pool of P
  //        shares one scale, the int8 copy is made at that scale as "<concat>/precision_trans".  Pools of another scale stay fp32
  //        readers.
  // The fp32 concat output is written only where a reader or a fetch is left.  An average pool, a global pool, a pool that is
  // fetched or has a second reader, a concat that only fp32 ops read: the separate instructions stay.  With set_fuse(true) only,
  // after K; bit-identical to the instructions it replaces (values are moved, the quantiser is calib's own).  No program without a
  // concat that a calib or a max pool reads changes.  DEFAULT ON: measured faster than the separate instructions by far more than
  // the run-to-run spread.
  void set_fuse_concat(bool on) { fuse_concat_ = on; }
  //   (M) a bilinear_interp / nearest_interp whose only reader is an arg_max along axis 1 and which is not fetched
  //       => ONE arg_max/interp instruction (plhip_interp_argmax_f32) that reads the low-resolution tensor and writes the labels; the
  //       resampled tensor is no variable of the program any more.
  //   (N) a bilinear_interp / nearest_interp (that M did not take) whose output a calib[fp32_to_int8] reads
  //       => ONE bilinear_interp/int8 | nearest_interp/int8 instruction (plhip_interp_f32 with y_i8) that writes the calib's tensor at
  //       its scale; the fp32 tensor is written only where a reader or a fetch is left.
  // Anything else (an arg_max along another axis, a second reader of the resampled tensor in front of an arg_max, an interp only
  // fp32 ops read) keeps the separate instructions.  With set_fuse(true) only, after L; bit-identical to the instructions they
  // replace (the resampled values come from one device function, the comparison and the quantiser are arg_max's and calib's own).
  // No program without an interp changes.  DEFAULT ON, each with a switch of its own: each was measured faster than the separate
  // instructions by far more than the run-to-run spread.
  void set_fuse_interp_argmax(bool on) { fuse_interp_argmax_ = on; }
  void set_fuse_interp_calib(bool on) { fuse_interp_calib_ = on; }
  //   (O1) a concat along axis 1 ALL of whose operands are chains transpose(0,2,3,1) -> reshape([0,-1,k]) of one k on 4-D tensors,
  //        each link the only reader of the one before and none fetched
  //        => ONE concat/nhwc instruction (plhip_concat_nhwc_f32) that reads the NCHW tensors and writes the joined [N, P, k] tensor;
  //        the transposed and reshaped tensors are no variables of the program any more.  SSD's six-map head: 13 instructions become 1.
  //   (O2) a transpose(0,2,1) that is not fetched and whose only reader is the Scores operand of a multiclass_nms
  //        => it disappears: the multiclass_nms instruction reads [N, P, C] through its strides.
  // Anything else (a second reader or a fetch of a link, another perm, another shape, a concat with one plain operand) keeps the
  // separate instructions.  With set_fuse(true) only, after N; bit-identical to the instructions it replaces (values are moved; the
  // NMS reads the same scores).  No program without a transpose changes.  DEFAULT ON: the whole step of ssd_mini_net was measured
  // faster than the separate instructions in every round, by more than the run-to-run spread.
  void set_fuse_detection_head(bool on) { fuse_detection_head_ = on; }
  //   (P) a multiclass_nms whose BBoxes operand is concat(axis 1) of the Boxes of k yolo_box ops (1 <= k <= 8) and whose Scores
  //       operand is transpose(0,2,1) of concat(axis 1) of the Scores of the SAME ops in the SAME order, all of them sharing ImgSize,
  //       class_num, conf_thresh, clip_bbox and scale_x_y, every link the only reader of the one before it and none fetched; k = 1:
  //       one yolo_box without concats whose Scores go through the transpose
  //       => ONE yolo_box/head instruction (plhip_yolo_head_f32) that reads the k feature maps and writes the boxes concat's
  //       variable [N, P, 4] and the transpose's output variable [N, C, P]; the multiclass_nms is unchanged.  2 k + 3 instructions
  //       (k = 3: 6 launches and, in the reference, 3 clearing passes) become 1.
  // Anything else (a fetched link, a second reader, differing attributes, scores concatenated in another order, more than 16
  // anchors in a map) keeps the separate instructions; with P off, O2 still folds the transpose.  With set_fuse(true) only, in
  // front of O; bit-identical to the instructions it replaces (the per-cell arithmetic is one device function, the rest are
  // moves).  No program without a yolo_box changes.  DEFAULT ON: the whole step of yolov3_mini_net was measured faster than the
  // separate instructions in every round, by more than the run-to-run spread.
  void set_fuse_yolo_head(bool on) { fuse_yolo_head_ = on; }
  GraphOp& Add(const std::string& type, const std::vector<std::string>& inputs, const std::string& output);
  // Emits the program into `pred`; returns the host-side names of the fetched variables ("<name>/host").
  std::vector<std::string> Lower(HipPredictor* pred);
  // The decisions of passes 1-3 as text, one instruction per line (CPU-testable without a device):
  //   "conv2d/int8_out in=a out=b oscale=0.031496"   "calib/fp32_to_int8 in=x out=x/precision_trans scale=..."
  std::vector<std::string> Plan();
  const std::vector<GraphOp>& ops() const { return ops_; }

 private:
  enum class StepKind { kOp, kIoCopyH2D, kIoCopyD2H, kCalibF2I, kCalibI2F, kImageToTensor, kImageConvert, kImageResize, kSeGate };
  // Which instruction a kOp step lowers to: its op's own (kPlain, with the modifiers further down), or the ONE fused instruction a
  // rewrite of FuseSteps made of it.  `via` then holds the names that are no longer written.
  enum class Form {
    kPlain,
    kShuffleInt8,   // (K2) a concat step that took shuffle_channel(2) and the calib behind it over: shuffle_channel/int8, `out` the
                    // shuffled tensor; calib_out / calib_scale / drop_f32 belong to the tensor the calib read
    kShuffleUnit,   // (K1) ... and the split behind the shuffle: shuffle_channel/unit, `out` the split's first half, `hi` its second
    kConcatInt8,    // (L) a concat step that took the calib behind it over: concat/int8, calib_out / calib_scale / drop_f32
    kConcatNhwc,    // (O1) a concat step that took the transpose -> reshape chains of its operands over: concat/nhwc, op_inputs the
                    // NCHW tensors, nhwc_k the chains' k
    kArgmaxInterp,  // (M) an interp step that took the arg_max(axis 1) behind it over: arg_max/interp, argmax_op that op's index in
                    // ops_, `out` the labels
    kYoloHead,      // (P) a yolo_box step that became the yolo_box/head instruction: yolo_ops the ops_ indices of the k yolo_box ops in
                    // the concats' order; op_inputs {X_0, ImgSize, X_1 ..}, outs {boxes [N, P, 4], scores [N, C, P]}
  };
  struct Step {
    int op{-1};              // index into ops_, or -1 for an inserted instruction
    StepKind kind{StepKind::kOp};
    std::string in, out;
    float scale{0.f};
    bool int8_out{false};
    float out_scale{1.f};
    std::vector<std::string> op_inputs;  // op inputs after cast renaming
    std::vector<std::string> outs;       // split: every output (outs[0] == out)
    Form form{Form::kPlain};
    std::string hi;             // kShuffleUnit
    int argmax_op{-1};          // kArgmaxInterp
    int nhwc_k{0};              // kConcatNhwc
    std::vector<int> yolo_ops;  // kYoloHead
    bool scores_npc{false};   // (O2) a multiclass_nms step whose Scores operand is the [N, P, C] input of the transpose taken over (`via`)
    // kHIP fusions (FuseSteps): tail taken over by an fp32_out conv or (J1 / J3 / N) by a hard_swish, an elementwise_mul or an interp,
    // int8 max pool behind a fused calib
    std::string res;          // residual operand of the fused elementwise_add ("" = none)
    bool res_relu{false};
    std::string calib_out;    // int8 tensor of the fused calib ("" = none)
    float calib_scale{1.f};
    bool drop_f32{false};     // the fp32 output has no consumer left
    bool pool_int8{false};    // pool2d(max) moved behind the calib: max commutes with the monotonic quantiser
    int pw_op{-1};            // depthwise conv that took its 1x1 consumer over: index of that conv in ops_
    bool pw_int8_out{true};
    float pw_out_scale{1.f};
    std::string via;          // name the depthwise result would have had
    bool pw_pool{false};      // ... and that conv's sole consumer, a global average pool2d, too (E): `out` is the pool's output
    std::string via_pw;       // name the 1x1 conv's result would have had
    bool pw_tail{false};      // fusion G: pw_op is the 1x1 consumer with its tail (res / calib_out / drop_f32 are then its own)
    float in_calib_scale{0.f};  // conv that took the calib[fp32_to_int8] in front of it over (F): its input is the calib's fp32 input
    std::string via_in;       // name the calib's int8 result would have had
    int image_feed{-1};       // image_to_tensor of feeds_[image_feed]; on a conv: it took that image_to_tensor over too (H1)
    bool image_int8{false};   // image_to_tensor that took the calib behind it over (H2): int8 output, `scale` the calib's
    bool resize_tensor{false};  // image_resize that took the image_to_tensor behind it over (I); image_int8: and the calib behind that
    bool resize_nv{false};      // ... and the image_convert in front: its source is the NV frame itself
    // kind kSeGate (J2): `in` the pooled tensor, `out` the gate, `scale` the calib's; op / pw_op the two convs in ops_, `via` the
    // names of the three tensors that are no longer written
  };
  struct Fuser;  // graph_builder.cc: the state the rewrites of FuseSteps share, one member function per rewrite
  void FeedSteps(std::vector<Step>* steps) const;
  void PickKernels(std::vector<bool>* int8_out, std::vector<float>* out_scale) const;  // pass 1, after checking the graph's names
  // The shape of every variable that follows from the feeds (an op type it does not know passes none on); CHECKs what concat,
  // split and shuffle_channel require of their operands' shapes.  Program() runs it once and hands the result to the rewrites.
  std::map<std::string, std::vector<int64_t>> InferShapes() const;
  std::vector<Step> Schedule();
  void FuseSteps(std::vector<Step>* steps, const std::map<std::string, std::vector<int64_t>>& shapes);
  std::vector<Step> Program();  // Schedule(), then FuseSteps() unless set_fuse(false): what Plan() prints and Lower() emits
  std::string OpLine(const Step& s) const;
  ConvAttrs LoweredConvAttrs(const Step& s) const;
  void LowerOp(const Step& s, HipPredictor* pred);
  struct FeedDesc {
    std::string name;
    std::vector<int64_t> dims;
    PrecisionType prec;
    int image_format{-1};              // FeedImage: the host variable is the uint8 image, `dims` the NCHW tensor made from it
    std::vector<int64_t> image_dims;   // [n, h, w, cs]
    float means[3]{0.f, 0.f, 0.f}, scales[3]{1.f, 1.f, 1.f};
    int frame_format{-1};              // FeedFrame: the host variable is the frame (image_dims = its dims), image_format what is normalised
    int frame_h{0}, frame_w{0};
  };
  bool fuse_{true};
  int fuse_dwpw_{2};
  bool fuse_dwconv_{false};
  bool fuse_hard_act_{false};
  bool fuse_shuffle_{true};
  bool fuse_concat_{true};
  bool fuse_interp_argmax_{true};
  bool fuse_interp_calib_{true};
  bool fuse_detection_head_{true};
  bool fuse_yolo_head_{true};
  std::vector<FeedDesc> feeds_;
  std::vector<std::string> fetches_;
  std::vector<GraphOp> ops_;
};

}  // namespace lite
}  // namespace paddle
