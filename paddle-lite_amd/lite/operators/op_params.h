// op_params.h — the parameter structs the hot-path kernels receive, field-for-field compatible (names, types,
// defaults) with the subset of lite/operators/op_params.h the ARM int8 kernels read:
//   WITH_INT8_CONFIG :49-54, IoCopyParam :70, CalibParam :82, FcParam :115-143, SoftmaxParam :319,
//   ActivationParam :395-419, ConvParam :446-502, PoolParam :539-, ElementwiseParam :643-651,
//   FusionElementwiseActivationParam :678-680, ShuffleChannelParam :258-263, ConcatParam :369-386, SplitParam :590-608,
//   InterpolateParam :154-168, ArgmaxParam :821-827, ReshapeParam :342-, TransposeParam :617-, BoxCoderParam :880-,
//   MulticlassNmsParam :910-922, PriorBoxParam :941-, YoloBoxParam :266-278.
// Tensors are NOT owned: params hold raw lite::Tensor* into the caller's scope (conv_op.h:72-74); bias may be null;
// paddings / dilations are shared_ptrs the op may mutate (UpdatePaddingAndDilation, conv_op.cc:55-81).
#pragma once
#include <memory>
#include <string>
#include <vector>

#include "lite/api/paddle_place.h"
#include "lite/core/tensor.h"

namespace paddle {
namespace lite {
namespace operators {

struct ParamBase {
  virtual ~ParamBase() = default;
};

#define WITH_INT8_CONFIG             \
  bool enable_int8{false};           \
  float input_scale{1.0f};           \
  std::vector<float> weight_scale{}; \
  float output_scale{1.0f};          \
  int bit_length{8};

struct IoCopyParam : ParamBase {
  const lite::Tensor* x{};
  lite::Tensor* y{};
  int process_type{0};
};

struct CalibParam : ParamBase {
  const lite::Tensor* input{};
  lite::Tensor* output{};
  float scale;
};

struct FcParam : ParamBase {
  lite::Tensor* input{nullptr};
  lite::Tensor* w{nullptr};
  lite::Tensor* bias{nullptr};
  lite::Tensor* output{nullptr};
  lite::DDim in_mat_dims;
  lite::DDim w_dims;
  int in_num_col_dims{1};
  std::string activation_type{""};
  bool padding_weights{false};
  WITH_INT8_CONFIG
};

struct SoftmaxParam : ParamBase {
  lite::Tensor* x{};
  lite::Tensor* output{};
  int axis{-1};
  bool use_cudnn{true};
};

struct ActivationParam : ParamBase {
  const lite::Tensor* X{};
  lite::Tensor* Out{};
  lite_api::ActivationType active_type{lite_api::ActivationType::kIndentity};
  bool has_active{false};
  float Leaky_relu_alpha{0};
  float Relu_clipped_coef{6};
  float hard_sigmoid_slope{0.2f};
  float hard_sigmoid_offset{0.5f};
  float hard_swish_threshold{6.0};
  float hard_swish_scale{6.0};
  float hard_swish_offset{3.0};
  float threshold{6.0f};
};

struct ConvParam : ParamBase {
  lite::Tensor* x{};
  lite::Tensor* filter{};
  lite::Tensor* bias{nullptr};
  lite::Tensor* residualData{nullptr};
  lite::Tensor* output{};
  std::vector<int> strides{1, 1};
  std::shared_ptr<std::vector<int>> paddings;
  int groups{1};
  std::shared_ptr<std::vector<int>> dilations;
  bool fuse_relu_before_depthwise_conv{false};
  bool fuse_relu{false};
  bool fuse_residual_connection{false};
  std::string data_format{"Anylayout"};
  ActivationParam activation_param;
  bool var_length{false};
  std::vector<int> output_size;
  WITH_INT8_CONFIG
};

struct PoolParam : ParamBase {
  lite::Tensor* x{};
  lite::Tensor* output{};
  std::string pooling_type{""};
  std::vector<int> ksize{};
  bool global_pooling{false};
  std::vector<int> strides{1, 1};
  std::shared_ptr<std::vector<int>> paddings;
  bool exclusive{true};
  bool adaptive{false};
  bool ceil_mode{false};
  bool use_quantizer{false};
  std::string data_format{"AnyLayout"};
  WITH_INT8_CONFIG
};

struct ElementwiseParam : ParamBase {
  const lite::Tensor* X{};
  const lite::Tensor* Y{};
  lite::Tensor* Out{};
  int axis{-1};  // for broadcasting.
  WITH_INT8_CONFIG
  float x_input_scale{1.0};
  float y_input_scale{1.0};
};

struct FusionElementwiseActivationParam : public ElementwiseParam {
  std::string act_type;
};

struct ShuffleChannelParam : ParamBase {
  const lite::Tensor* X{};
  lite::Tensor* Out{};
  int group;
};

struct ConcatParam : ParamBase {
  std::vector<lite::Tensor*> x{};
  lite::Tensor* output{};
  int axis{0};
  lite::Tensor* axis_tensor{};
};

struct SplitParam : ParamBase {
  lite::Tensor* x{};
  std::vector<lite::Tensor*> output{};
  lite::Tensor* axis_tensor{};
  std::vector<lite::Tensor*> sections_tensor_list{};
  int axis{-1};
  int num{0};
  std::vector<int> sections;
};

// bilinear_interp / nearest_interp.  kHIP takes the output size from the attributes only: OutSize, SizeTensor and Scale must
// stay empty (fatal in PrepareForRun)
struct InterpolateParam : ParamBase {
  lite::Tensor* X{};
  lite::Tensor* OutSize{};
  lite::Tensor* Out{};
  std::vector<const lite::Tensor*> SizeTensor;
  lite::Tensor* Scale{};
  float scale{0.f};
  int out_h{-1};
  int out_w{-1};
  bool align_corners{true};
  int align_mode{1};
  std::string interp_method{"Nearest"};
  DataLayoutType data_layout{DATALAYOUT(kNCHW)};
};

struct ArgmaxParam : ParamBase {
  lite::Tensor* X{};
  lite::Tensor* Out{};
  int Axis{0};
  int dtype{-1};
  bool keepdims{false};
};

// reshape / reshape2.  kHIP takes the shape from shape_vct only: shape_tensor_vct and shape_tensor must stay empty
struct ReshapeParam : ParamBase {
  const lite::Tensor* x{};
  std::vector<const lite::Tensor*> shape_tensor_vct{};
  const lite::Tensor* shape_tensor{};
  std::vector<int> shape_vct{};
  lite::Tensor* output{};
  lite::Tensor* xshape{};
  bool inplace{false};
};

// transpose / transpose2
struct TransposeParam : ParamBase {
  const lite::Tensor* x{};
  lite::Tensor* output{};
  lite::Tensor* xshape{};
  std::vector<int> axis;
  bool use_mkldnn{false};
  std::string data_format{"AnyLayout"};
};

struct BoxCoderParam : ParamBase {
  const lite::Tensor* prior_box{};
  const lite::Tensor* prior_box_var{};
  const lite::Tensor* target_box{};
  lite::Tensor* proposals{};
  std::string code_type{"encode_center_size"};
  bool box_normalized{true};
  int axis{0};
  std::vector<float> variance{};
};

// kHIP writes out [N, keep_top_k, 6] padded with -1 and the per-image counts into a tensor of its own, which has no field here:
// lite/kernels/hip/detection_fusion.h
struct MulticlassNmsParam : ParamBase {
  const lite::Tensor* bboxes{};
  const lite::Tensor* scores{};
  lite::Tensor* out{};
  lite::Tensor* index{};
  int background_label{0};
  float score_threshold{};
  int nms_top_k{};
  float nms_threshold{0.3f};
  float nms_eta{1.0f};
  int keep_top_k;
  bool normalized{true};
};

// kHIP alias head (fusion P) reads further feature maps, which have no field here: lite/kernels/hip/yolo_fusion.h
struct YoloBoxParam : ParamBase {
  lite::Tensor* X{};
  lite::Tensor* ImgSize{};
  lite::Tensor* Boxes{};
  lite::Tensor* Scores{};

  std::vector<int> anchors{};
  int class_num{0};
  float conf_thresh{0.f};
  int downsample_ratio{0};
  bool clip_bbox{true};
  float scale_x_y{1.0f};
};

struct PriorBoxParam : ParamBase {
  lite::Tensor* input{};
  lite::Tensor* image{};
  lite::Tensor* boxes{};
  lite::Tensor* variances{};
  bool flip;
  bool clip;
  std::vector<float> min_sizes;
  std::vector<float> max_sizes;
  std::vector<float> aspect_ratios;
  std::vector<float> variances_;
  int img_w{0};
  int img_h{0};
  float step_w{0};
  float step_h{0};
  float offset{0.5};
  int prior_num{0};
  std::vector<std::string> order;
  bool min_max_aspect_ratios_order{false};
};

}  // namespace operators
}  // namespace lite
}  // namespace paddle
