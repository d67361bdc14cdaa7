// graph_builder.cc — see graph_builder.h.
#include "lite/api/graph_builder.h"

#include <string.h>

#include "lite/core/mir/fusion/hip_conv_tail_matcher.h"
#include "lite/kernels/hip/image_frame.h"
#include "lite/kernels/hip/image_to_tensor.h"
#include "lite/kernels/hip/prior_box_host.h"
#include "plhip.h"

#include <algorithm>
#include <cstdio>
#include <set>

namespace paddle {
namespace lite {

void GraphBuilder::Feed(const std::string& name, const std::vector<int64_t>& dims, PrecisionType prec) {
  feeds_.push_back({name, dims, prec});
}

void GraphBuilder::FeedImage(const std::string& name, int n, int h, int w, int format, const float* means, const float* scales) {
  CHECK(format >= PLHIP_IMG_RGBA && format <= PLHIP_IMG_GRAY) << "FeedImage: unsupported image format " << format;
  CHECK(n > 0 && h > 0 && w > 0) << "FeedImage: bad image size";
  FeedDesc f;
  f.name = name;
  f.dims = {n, operators::ImageChannels(format), h, w};
  f.prec = PRECISION(kFloat);
  f.image_format = format;
  f.image_dims = {n, h, w, operators::ImagePixelBytes(format)};
  for (int i = 0; i < 3; ++i) {
    f.means[i] = means[i];
    f.scales[i] = scales[i];
  }
  feeds_.push_back(f);
}

void GraphBuilder::FeedFrame(const std::string& name, int n, int src_h, int src_w, int src_format, int dst_h, int dst_w,
                             const float* means, const float* scales) {
  const bool nv = operators::FrameIsNV(src_format);
  CHECK(nv || (src_format >= PLHIP_IMG_RGBA && src_format <= PLHIP_IMG_GRAY)) << "FeedFrame: unsupported frame format " << src_format;
  CHECK(n > 0 && src_h > 0 && src_w > 0 && dst_h > 0 && dst_w > 0) << "FeedFrame: bad frame / image size";
  CHECK(!nv || (src_h % 2 == 0 && src_w % 2 == 0)) << "FeedFrame: an NV12 / NV21 frame needs even w and h";
  const bool resized = src_h != dst_h || src_w != dst_w;
  CHECK(!resized || (src_h >= 2 && src_w >= 2)) << "FeedFrame: a frame that is resized needs at least 2 rows and 2 columns";
  const int fmt = nv ? static_cast<int>(PLHIP_IMG_BGR) : src_format;
  FeedImage(name, n, dst_h, dst_w, fmt, means, scales);
  if (!nv && !resized) return;  // nothing in front of image_to_tensor: an image feed
  FeedDesc& f = feeds_.back();
  f.frame_format = src_format;
  f.frame_h = src_h;
  f.frame_w = src_w;
  f.image_dims = operators::FrameDims(n, src_h, src_w, src_format);
}

GraphOp& GraphBuilder::Add(const std::string& type, const std::vector<std::string>& inputs, const std::string& output) {
  ops_.emplace_back();
  GraphOp& op = ops_.back();
  op.type = type;
  op.inputs = inputs;
  op.output = output;
  return op;
}

void GraphBuilder::FeedSteps(std::vector<Step>* steps) const {
  for (size_t k = 0; k < feeds_.size(); ++k) {
    const FeedDesc& f = feeds_[k];
    auto push = [&](StepKind kind, const std::string& in, const std::string& out, int image_feed) {
      Step s;
      s.kind = kind; s.image_feed = image_feed;
      s.in = in; s.out = out;
      steps->push_back(s);
      return out;
    };
    std::string img = push(StepKind::kIoCopyH2D, f.name, f.name + "/target_trans", -1);
    if (f.frame_format >= 0) {  // FeedFrame: imageConvert (NV only) and imageResize (unequal sizes only) in front
      if (operators::FrameIsNV(f.frame_format)) img = push(StepKind::kImageConvert, img, f.name + "/bgr", static_cast<int>(k));
      if (f.frame_h != f.dims[2] || f.frame_w != f.dims[3]) img = push(StepKind::kImageResize, img, f.name + "/image", static_cast<int>(k));
    }
    if (f.image_format >= 0) push(StepKind::kImageToTensor, img, f.name + "/tensor", static_cast<int>(k));  // FeedImage: the ops' fp32 NCHW tensor
  }
}

namespace {

std::vector<std::string> OutputsOf(const GraphOp& op) { return op.outputs.empty() ? std::vector<std::string>{op.output} : op.outputs; }

std::string DimsStr(const std::vector<int64_t>& d) {
  std::string s = "{";
  for (size_t i = 0; i < d.size(); ++i) s += (i ? "," : "") + std::to_string(d[i]);
  return s + "}";
}

// conv_op.h:149-161: 2-element paddings mean {top = bottom, left = right}
std::vector<int> Pad4(const std::vector<int>& p) { return p.size() == 2 ? std::vector<int>{p[0], p[0], p[1], p[1]} : p; }

// The conv's attributes have the sizes every rewrite below indexes: OIHW weights, four paddings, two strides, two dilations, explicit padding.
bool ConvSizesOk(const GraphOp& op, const std::vector<int>& pad4) {
  return op.w_dims.size() == 4 && pad4.size() == 4 && op.conv.strides.size() == 2 && op.conv.dilations.size() == 2 &&
         op.conv.padding_algorithm.empty();
}

// Output shape of a conv on the NCHW shape `in` (conv_op.cc:25-52); empty where the attributes are not of those sizes
std::vector<int64_t> ConvOutShape(const GraphOp& op, const std::vector<int64_t>& in) {
  const std::vector<int> pd = Pad4(op.conv.paddings);
  if (!ConvSizesOk(op, pd) || in.size() != 4) return {};
  const int64_t keh = op.conv.dilations[0] * (op.w_dims[2] - 1) + 1, kew = op.conv.dilations[1] * (op.w_dims[3] - 1) + 1;
  return {in[0], op.w_dims[0], (in[2] + pd[0] + pd[1] - keh) / op.conv.strides[0] + 1, (in[3] + pd[2] + pd[3] - kew) / op.conv.strides[1] + 1};
}

// Output shape of a conv2d_transpose on the NCHW shape `in` (conv_transpose_op.cc:43-96); CHECKs what the kHIP kernel is fatal on
std::vector<int64_t> ConvTransposeOutShape(const GraphOp& op, const std::vector<int64_t>& in) {
  const std::string who = "conv2d_transpose " + op.output;
  const std::vector<int> pd = Pad4(op.conv.paddings);
  CHECK(ConvSizesOk(op, pd)) << who << ": a 4-D filter, 2 or 4 paddings, 2 strides, 2 dilations and explicit padding";
  CHECK(in.size() == 4) << who << ": input " << DimsStr(in) << " is not [N, C, H, W]";
  CHECK(op.conv.groups >= 1 && in[1] % op.conv.groups == 0 && in[1] == op.w_dims[0])
      << who << ": the filter's first extent " << op.w_dims[0] << " must be the input's " << in[1] << " channels, divisible by groups " << op.conv.groups;
  CHECK(op.conv.output_size.empty() || op.conv.output_size.size() == 2) << who << ": output_size has " << op.conv.output_size.size() << " entries";
  std::vector<int64_t> o{in[0], op.w_dims[1] * op.conv.groups};
  for (int i = 0; i < 2; ++i) {
    CHECK(op.conv.strides[i] >= 1 && op.conv.dilations[i] >= 1 && pd[2 * i] >= 0 && pd[2 * i + 1] >= 0) << who << ": stride / dilation < 1 or a negative padding";
    int64_t e = (in[i + 2] - 1) * op.conv.strides[i] - pd[2 * i] - pd[2 * i + 1] + op.conv.dilations[i] * (op.w_dims[i + 2] - 1) + 1;
    CHECK(e >= 1) << who << ": the output extent " << e << " is empty";
    if (!op.conv.output_size.empty()) {
      const int64_t want = op.conv.output_size[i];
      CHECK(want >= e && want < e + op.conv.strides[i]) << who << ": output_size " << want << " outside [" << e << ", " << e + op.conv.strides[i] << ")";
      e = want;
    }
    o.push_back(e);
  }
  return o;
}

// concat_op.cc:22-62 on the operands' shapes; CHECKs that they differ along the axis only
std::vector<int64_t> ConcatOutShape(const GraphOp& op, const std::vector<std::vector<int64_t>>& ins) {
  std::vector<int64_t> o = ins[0];
  const int rank = static_cast<int>(o.size());
  const int axis = op.axis < 0 ? op.axis + rank : op.axis;
  CHECK(axis >= 0 && axis < rank) << "concat " << op.output << ": axis " << op.axis << " outside the rank " << rank;
  for (size_t i = 1; i < ins.size(); ++i) {
    bool same = ins[i].size() == o.size();
    for (int j = 0; same && j < rank; ++j) same = j == axis || ins[i][j] == ins[0][j];
    CHECK(same) << "concat " << op.output << ": input " << op.inputs[i] << " " << DimsStr(ins[i]) << " differs from " << op.inputs[0] << " "
                << DimsStr(ins[0]) << " outside axis " << axis;
    o[axis] += ins[i][axis];
  }
  return o;
}

// split_op.cc:32-75 on the input's shape: the extent of every output along the axis; CHECKs num / sections against it
std::vector<int64_t> SplitExtents(const GraphOp& op, const std::vector<int64_t>& in, int* axis_out) {
  const int rank = static_cast<int>(in.size());
  const int axis = op.axis < 0 ? op.axis + rank : op.axis;
  CHECK(axis >= 0 && axis < rank) << "split " << op.inputs[0] << ": axis " << op.axis << " outside the rank " << rank;
  const size_t n = OutputsOf(op).size();
  std::vector<int64_t> e;
  if (op.num > 0) {
    CHECK(static_cast<size_t>(op.num) == n) << "split " << op.inputs[0] << ": num " << op.num << " but " << n << " outputs";
    CHECK(in[axis] % op.num == 0) << "split " << op.inputs[0] << ": num " << op.num << " does not divide the axis (" << in[axis] << ")";
    e.assign(n, in[axis] / op.num);
  } else {
    CHECK(op.sections.size() == n) << "split " << op.inputs[0] << ": " << op.sections.size() << " sections but " << n << " outputs";
    int64_t sum = 0;
    for (int v : op.sections) {
      CHECK(v >= 1) << "split " << op.inputs[0] << ": a section of " << v;
      sum += v;
      e.push_back(v);
    }
    CHECK(sum == in[axis]) << "split " << op.inputs[0] << ": the sections do not add up to the axis (" << sum << " of " << in[axis] << ")";
  }
  *axis_out = axis;
  return e;
}

bool IsInterp(const GraphOp& op) { return op.type == "bilinear_interp" || op.type == "nearest_interp"; }

// interpolate_op.cc:37-82 with the size from the attributes; CHECKs what the kHIP kernels are fatal on
std::vector<int64_t> InterpOutShape(const GraphOp& op, const std::vector<int64_t>& in) {
  CHECK(in.size() == 4) << op.type << " " << op.output << ": input " << DimsStr(in) << " is not [N, C, H, W]";
  CHECK(op.align_mode == 0 || op.align_mode == 1) << op.type << " " << op.output << ": align_mode " << op.align_mode;
  int64_t oh = op.out_h, ow = op.out_w;
  if (!(op.out_h > 0 && op.out_w > 0)) {
    CHECK(op.interp_scale > 0.f) << op.type << " " << op.output << ": neither out_h / out_w nor a scale > 0";
    oh = static_cast<int>(in[2] * op.interp_scale);
    ow = static_cast<int>(in[3] * op.interp_scale);
  }
  CHECK(oh >= 1 && ow >= 1) << op.type << " " << op.output << ": the output size " << oh << " x " << ow << " is empty";
  return {in[0], in[1], oh, ow};
}

// argmax_op.cc:29-60: the axis is dropped, or kept as 1
std::vector<int64_t> ArgmaxOutShape(const GraphOp& op, const std::vector<int64_t>& in) {
  const int rank = static_cast<int>(in.size());
  const int axis = op.axis < 0 ? op.axis + rank : op.axis;
  CHECK(axis >= 0 && axis < rank) << "arg_max " << op.output << ": axis " << op.axis << " outside the rank " << rank;
  CHECK(op.dtype == -1 || op.dtype == 2 || op.dtype == 3) << "arg_max " << op.output << ": dtype " << op.dtype << " is neither int64 (-1, 3) nor int32 (2)";
  std::vector<int64_t> o;
  for (int i = 0; i < rank; ++i) {
    if (i != axis) o.push_back(in[i]);
    else if (op.keepdims) o.push_back(1);
  }
  return o;
}

// the output shapes of the detection-head ops on their operands' shapes `ins`; CHECKs what the kHIP kernels are fatal on
std::vector<std::vector<int64_t>> DetectionOutShapes(const GraphOp& op, const std::vector<std::vector<int64_t>>& ins) {
  const std::string who = op.type + " " + op.output;
  if (op.type == "transpose") {
    operators::TransposeOpLite::CheckPerm(op.perm, ins[0].size(), who);
    std::vector<int64_t> o(ins[0].size());
    for (size_t k = 0; k < o.size(); ++k) o[k] = ins[0][op.perm[k]];
    return {o};
  }
  if (op.type == "reshape") return {operators::ReshapeOpLite::OutputDims(ins[0], op.shape, who)};
  if (op.type == "prior_box") {
    CHECK(ins.size() == 2 && ins[0].size() == 4 && ins[1].size() == 4) << who << ": Input and Image must be [N, C, H, W]";
    CHECK(!op.min_sizes.empty() && (op.max_sizes.empty() || op.max_sizes.size() == op.min_sizes.size()) && op.variances.size() == 4)
        << who << ": min_sizes, one max_size per min_size or none, and four variances";
    const int64_t num = kernels::hip::PriorBoxNum(op.min_sizes, op.max_sizes, op.aspect_ratios, op.flip);
    const std::vector<int64_t> o{ins[0][2], ins[0][3], num, 4};
    return {o, o};
  }
  if (op.type == "box_coder") {
    CHECK(ins.size() == 2 || ins.size() == 3) << who << ": {PriorBox, TargetBox} or {PriorBox, PriorBoxVar, TargetBox}";
    CHECK(op.variances.empty() || op.variances.size() == 4) << who << ": the variance attribute has " << op.variances.size() << " values";
    auto flat = [](std::vector<int64_t> d) { return d.size() == 4 ? std::vector<int64_t>{d[0] * d[1] * d[2], d[3]} : d; };
    const std::vector<int64_t> pv = ins.size() == 3 ? flat(ins[1]) : std::vector<int64_t>{};
    operators::BoxCoderOpLite::CheckDims(flat(ins[0]), ins.size() == 3 ? &pv : nullptr, ins.back(), op.axis);
    return {ins.back()};
  }
  CHECK(op.type == "multiclass_nms") << who;
  CHECK(ins.size() == 2) << who << ": {BBoxes, Scores}";
  operators::MulticlassNmsParam p;
  p.background_label = op.background_label; p.nms_top_k = op.nms_top_k; p.keep_top_k = op.keep_top_k; p.nms_eta = op.nms_eta;
  operators::MulticlassNmsOpLite::CheckCall(ins[0], ins[1], false, p);
  std::vector<std::vector<int64_t>> o{{ins[0][0], op.keep_top_k, 6}, {ins[0][0]}};
  if (op.outputs.size() > 2) o.push_back({ins[0][0], op.keep_top_k});
  return o;
}

bool IsDetectionOp(const GraphOp& op) {
  return op.type == "transpose" || op.type == "reshape" || op.type == "prior_box" || op.type == "box_coder" || op.type == "multiclass_nms";
}

void CheckShuffleGroup(const GraphOp& op, const std::vector<int64_t>& in) {
  CHECK(in.size() >= 2) << "shuffle_channel " << op.output << ": input must have a channel axis";
  CHECK(op.group >= 1 && in[1] % op.group == 0) << "shuffle_channel " << op.output << ": group " << op.group << " does not divide C = " << in[1];
}

}  // namespace

std::map<std::string, std::vector<int64_t>> GraphBuilder::InferShapes() const {
  std::map<std::string, std::vector<int64_t>> shape;
  for (auto& f : feeds_) shape[f.name] = f.dims;
  for (const GraphOp& op : ops_) {
    std::vector<std::vector<int64_t>> ins;
    for (auto& v : op.inputs) {
      const auto it = shape.find(v);
      if (it != shape.end()) ins.push_back(it->second);
    }
    if (ins.size() != op.inputs.size() || ins.empty()) continue;  // an operand of unknown shape: nothing to say
    const std::vector<int64_t>& in = ins[0];
    if (op.type == "concat") {
      shape[op.output] = ConcatOutShape(op, ins);
    } else if (op.type == "split") {
      int axis = 0;
      const std::vector<int64_t> e = SplitExtents(op, in, &axis);
      const std::vector<std::string> outs = OutputsOf(op);
      for (size_t i = 0; i < outs.size(); ++i) {
        std::vector<int64_t> o = in;
        o[axis] = e[i];
        shape[outs[i]] = o;
      }
    } else if (op.type == "shuffle_channel") {
      CheckShuffleGroup(op, in);
      shape[op.output] = in;
    } else if (IsDetectionOp(op)) {
      const auto o = DetectionOutShapes(op, ins);
      const std::vector<std::string> outs = OutputsOf(op);
      CHECK(o.size() == outs.size()) << op.type << " " << op.output << ": " << outs.size() << " outputs named, " << o.size() << " expected";
      for (size_t i = 0; i < outs.size(); ++i) shape[outs[i]] = o[i];
    } else if (op.type == "yolo_box") {
      const std::string who = "yolo_box " + op.output;
      CHECK(ins.size() == 2 && op.outputs.size() == 2) << who << ": inputs {X, ImgSize} and outputs {Boxes, Scores}";
      const int64_t p = operators::YoloBoxOpLite::CheckDims(ins[0], ins[1], op.anchors, op.class_num, who);
      shape[op.outputs[0]] = {in[0], p, 4};
      shape[op.outputs[1]] = {in[0], p, op.class_num};
    } else if (IsInterp(op)) {
      shape[op.output] = InterpOutShape(op, in);
    } else if (op.type == "arg_max") {
      shape[op.output] = ArgmaxOutShape(op, in);
    } else if (op.type == "conv2d" || op.type == "depthwise_conv2d") {
      const std::vector<int64_t> o = ConvOutShape(op, in);
      if (!o.empty()) shape[op.output] = o;
    } else if (op.type == "conv2d_transpose") {
      shape[op.output] = ConvTransposeOutShape(op, in);
    } else if (op.type == "pool2d") {
      const std::vector<int> pd = Pad4(op.pool_paddings);
      if (in.size() != 4 || pd.size() != 4) continue;
      if (op.global_pooling) {
        shape[op.output] = {in[0], in[1], 1, 1};
      } else if (op.ksize.size() == 2 && op.pool_strides.size() == 2) {
        shape[op.output] = {in[0], in[1],
                            operators::PoolOutputSize(static_cast<int>(in[2]), op.ksize[0], pd[0], pd[1], op.pool_strides[0], op.ceil_mode),
                            operators::PoolOutputSize(static_cast<int>(in[3]), op.ksize[1], pd[2], pd[3], op.pool_strides[1], op.ceil_mode)};
      }
    } else if (op.type == "fc") {
      if (op.w_dims.size() == 2) shape[op.output] = {in[0], op.w_dims[1]};
    } else if (op.type == "elementwise_add" || op.type == "fusion_elementwise_add_activation" || op.type == "elementwise_mul" ||
               op.type == "softmax" || op.type == "hard_swish" || op.type == "hard_sigmoid") {
      shape[op.output] = in;
    }
  }
  return shape;
}

void GraphBuilder::PickKernels(std::vector<bool>* int8_out, std::vector<float>* out_scale) const {
  // ---- who consumes what (fetch counts as a consumer that is not enable_int8)
  std::map<std::string, std::vector<int>> consumers;
  std::set<std::string> known;
  for (auto& f : feeds_) known.insert(f.name);
  for (size_t i = 0; i < ops_.size(); ++i) {
    for (auto& in : ops_[i].inputs) {
      CHECK(known.count(in)) << ops_[i].type << ": input " << in << " is not produced by an earlier op or feed";
      consumers[in].push_back(static_cast<int>(i));
    }
    for (auto& out : OutputsOf(ops_[i])) {  // every output of a split is a variable of its own
      CHECK(!known.count(out)) << "variable " << out << " is written twice";
      known.insert(out);
    }
  }

  std::set<std::string> fetched(fetches_.begin(), fetches_.end());
  for (auto& f : fetches_) CHECK(known.count(f)) << "fetch of unknown variable " << f;

  // ---- pass 1: static_kernel_pick_pass.cc:92-165
  int8_out->assign(ops_.size(), false);
  out_scale->assign(ops_.size(), 1.f);
  for (size_t i = 0; i < ops_.size(); ++i) {
    if (!ops_[i].enable_int8) continue;
    const auto it = consumers.find(ops_[i].output);
    bool all_int8 = it != consumers.end() && !it->second.empty() && !fetched.count(ops_[i].output);
    if (all_int8)
      for (int c : it->second) all_int8 = all_int8 && ops_[c].enable_int8;
    (*int8_out)[i] = all_int8;
    if (all_int8) (*out_scale)[i] = ops_[it->second.front()].conv.input_scale;  // :118-121 (first adjacent op)
  }
}

std::vector<GraphBuilder::Step> GraphBuilder::Schedule() {
  std::vector<bool> int8_out;
  std::vector<float> out_scale;
  PickKernels(&int8_out, &out_scale);
  // ---- passes 2 + 3 while walking the ops in order
  std::map<std::string, int> producer;         // of the ops walked so far
  std::map<std::string, PrecisionType> prec;   // precision of every device variable
  std::map<std::string, std::string> cast_of;  // type_precision_cast_pass's cast_nodes
  std::vector<Step> steps;
  FeedSteps(&steps);
  for (auto& f : feeds_) prec[f.name] = f.prec;
  auto dev_name = [&](const std::string& v) {
    for (auto& f : feeds_)
      if (f.name == v) return v + (f.image_format >= 0 ? "/tensor" : "/target_trans");
    return v;
  };
  for (size_t i = 0; i < ops_.size(); ++i) {
    const GraphOp& op = ops_[i];
    const PrecisionType want = op.enable_int8 ? PRECISION(kInt8) : PRECISION(kFloat);
    Step s;
    s.op = static_cast<int>(i);
    for (auto& in : op.inputs) {
      std::string use = dev_name(in);
      if (prec[in] != want && prec[in] != PRECISION(kInt32)) {  // an int32 operand (yolo_box's ImgSize) is no tensor to quantise
        auto c = cast_of.find(in);
        if (c == cast_of.end()) {
          Step cs;
          cs.in = use;
          cs.out = in + "/precision_trans";
          if (want == PRECISION(kInt8)) {
            cs.kind = StepKind::kCalibF2I;
            cs.scale = op.conv.input_scale;  // InferScale case 1
          } else {
            cs.kind = StepKind::kCalibI2F;
            const auto p = producer.find(in);
            CHECK(p != producer.end()) << "int8 feed " << in << " consumed by an fp32 op: no scale to dequantise with";
            cs.scale = out_scale[p->second];  // InferScale case 2
          }
          steps.push_back(cs);
          c = cast_of.emplace(in, cs.out).first;
        }
        use = c->second;
      }
      s.op_inputs.push_back(use);
    }
    s.out = op.output;
    s.outs = op.outputs;
    s.int8_out = int8_out[i];
    s.out_scale = out_scale[i];
    steps.push_back(s);
    for (auto& out : OutputsOf(op)) {
      producer[out] = static_cast<int>(i);
      prec[out] = (op.enable_int8 && int8_out[i]) ? PRECISION(kInt8) : PRECISION(kFloat);
    }
  }
  for (auto& f : fetches_) {
    Step s;
    s.kind = StepKind::kIoCopyD2H;
    s.in = dev_name(f);
    s.out = f + "/host";
    steps.push_back(s);
  }
  return steps;
}

namespace {

// The plhip descriptor of `op` on an NCHW input of shape `in`; false (a rewrite then leaves the op alone) where the sizes are not those.
bool ConvDesc(const GraphOp& op, const std::vector<int64_t>& in, plhip_conv_desc* d) {
  const std::vector<int> pd = Pad4(op.conv.paddings);
  if (!ConvSizesOk(op, pd) || in.size() != 4) return false;
  memset(d, 0, sizeof(*d));
  d->n = static_cast<int>(in[0]); d->cin = static_cast<int>(in[1]);
  d->h = static_cast<int>(in[2]); d->w = static_cast<int>(in[3]);
  d->cout = static_cast<int>(op.w_dims[0]); d->kh = static_cast<int>(op.w_dims[2]); d->kw = static_cast<int>(op.w_dims[3]);
  for (int q = 0; q < 4; ++q) d->pad[q] = pd[q];
  d->stride[0] = op.conv.strides[0]; d->stride[1] = op.conv.strides[1];
  d->dil[0] = op.conv.dilations[0]; d->dil[1] = op.conv.dilations[1];
  d->groups = op.conv.groups;
  return true;
}

// A TRUE depthwise conv (channel multiplier 1): anything else stays two instructions instead of failing a CHECK later
bool IsTrueDepthwise(const GraphOp& op) { return op.w_dims.size() == 4 && op.w_dims[1] == 1 && op.w_dims[0] == op.conv.groups; }

// An int8 conv2d 1x1, groups 1, stride 1, dilation 1, no padding: the weight / attribute part of what D, G and J2 take over
bool IsPlain1x1Conv(const GraphOp& c) {
  bool pad0 = true;
  for (int v : c.conv.paddings) pad0 = pad0 && v == 0;
  return c.type == "conv2d" && c.enable_int8 && c.w_dims.size() == 4 && c.w_dims[2] == 1 && c.w_dims[3] == 1 && c.conv.groups == 1 &&
         c.conv.strides == std::vector<int>({1, 1}) && c.conv.dilations == std::vector<int>({1, 1}) && pad0;
}

// Ops whose output has the shape of their first input (PropagateShapes)
const char* const kSameShapeOps[] = {"elementwise_add", "fusion_elementwise_add_activation", "shuffle_channel"};

void AppendNum(std::string* l, const char* key, float x) {
  char buf[64];
  snprintf(buf, sizeof buf, " %s=%.9g", key, x);
  *l += buf;
}

// "a,b,c" of names or ints
const std::string& Str(const std::string& s) { return s; }
std::string Str(int v) { return std::to_string(v); }
template <class T>
std::string Join(const std::vector<T>& v) {
  std::string a;
  for (size_t i = 0; i < v.size(); ++i) a += (i ? "," : "") + Str(v[i]);
  return a;
}

}  // namespace

struct GraphBuilder::Fuser {
  const GraphBuilder& g;
  std::vector<Step>& st;
  std::vector<bool> dead;
  std::map<std::string, std::vector<int64_t>> shape;  // PropagateShapes: NCHW shape of the variables it could follow from the feeds
  const std::map<std::string, std::vector<int64_t>>& var_shape;  // GraphBuilder::InferShapes, by graph variable: followed through every op type
  Fuser(const GraphBuilder& gb, std::vector<Step>* steps, const std::map<std::string, std::vector<int64_t>>& shapes)
      : g(gb), st(*steps), dead(steps->size(), false), var_shape(shapes) {}

  const GraphOp& Op(int t) const { return g.ops_[st[t].op]; }
  bool Live(size_t t, StepKind kind) const { return !dead[t] && st[t].kind == kind; }
  // t is a step (dead or not; -1: none) that runs the graph op `type`
  bool IsOp(int t, const char* type) const { return t >= 0 && st[t].kind == StepKind::kOp && Op(t).type == type; }
  bool IsGlobalAvgPool(int t) const { return IsOp(t, "pool2d") && Op(t).pooling_type == "avg" && Op(t).global_pooling && !st[t].pool_int8; }
  int Uses(const std::string& v) const {
    int n = 0;
    for (size_t i = 0; i < st.size(); ++i) {
      if (dead[i]) continue;
      if (st[i].kind == StepKind::kOp) {
        for (auto& in : st[i].op_inputs) n += in == v;
        n += st[i].res == v;
      } else {
        n += st[i].in == v;
      }
    }
    return n;
  }
  // The one live step that reads v, as its first input; -1 where v has another number of uses or is read as a second operand or a
  // residual.  (With one use at most one step can match, so which match a search keeps is not a question.)
  int SoleReader(const std::string& v) const {
    if (Uses(v) != 1) return -1;
    for (size_t t = 0; t < st.size(); ++t) {
      if (dead[t]) continue;
      const Step& s = st[t];
      if (s.kind == StepKind::kOp ? (!s.op_inputs.empty() && s.op_inputs[0] == v) : s.in == v) return static_cast<int>(t);
    }
    return -1;
  }
  // The last live inserted step of `kind` at or behind `from` whose input is v, or -1
  int FindByInput(StepKind kind, const std::string& v, size_t from = 0) const {
    int k = -1;
    for (size_t t = from; t < st.size(); ++t)
      if (Live(t, kind) && st[t].in == v) k = static_cast<int>(t);
    return k;
  }
  // Step i takes the calib[fp32_to_int8] over that reads v at or behind step `from`: the calib's tensor and scale go to the step and the
  // calib dies.  False (nothing changed) where there is none.  drop_f32 is the caller's: which variable must have no reader left
  // (K1 asks about `hi`, not `out`) it alone knows, and it asks after it killed what else it took over.
  bool TakeCalib(size_t i, const std::string& v, size_t from) {
    const int k = FindByInput(StepKind::kCalibF2I, v, from);
    if (k < 0) return false;
    st[i].calib_out = st[k].out;
    st[i].calib_scale = st[k].scale;
    dead[k] = true;
    return true;
  }
  // The live step of graph op `type` one of whose outputs is v, v being read by exactly one live step (a fetch counts), or -1
  int SoleProducer(const std::string& v, const char* type) const {
    if (Uses(v) != 1) return -1;
    for (size_t t = 0; t < st.size(); ++t) {
      if (dead[t] || !IsOp(static_cast<int>(t), type)) continue;
      if (st[t].out == v || std::find(st[t].outs.begin(), st[t].outs.end(), v) != st[t].outs.end()) return static_cast<int>(t);
    }
    return -1;
  }
  // The descriptor of conv step i on the propagated shape of its input
  bool InputDesc(int i, plhip_conv_desc* d) const {
    const auto it = st[i].op_inputs.empty() ? shape.end() : shape.find(st[i].op_inputs[0]);
    return it != shape.end() && ConvDesc(Op(i), it->second, d);
  }
  // What D and G start from: a true depthwise_conv2d[int8_out] that has not taken a 1x1 conv over yet
  bool FusableDepthwise(size_t i) const {
    return Live(i, StepKind::kOp) && Op(i).type == "depthwise_conv2d" && st[i].int8_out && st[i].pw_op < 0 && IsTrueDepthwise(Op(i));
  }

  void ConvTails();
  void FrameResize();
  bool StemTakesImage(int j, const FeedDesc& f) const;
  void ImageFeed();
  void PropagateShapes();
  void DepthwisePointwise();
  void CalibIntoStem();
  void DepthwiseConv1x1Tail();
  void SeGate();
  void CalibBehind(bool (*takes)(const GraphOp&));
  void HardActCalib();
  void ShuffleTail();
  void ConcatCalib();
  void InterpArgmax();
  void InterpCalib();
  void DetectionHead();
  void YoloHead();
};

// (A) (C) (B): the conv-tail patterns, matched by the SAME code a Paddle-Lite tree runs as a mir pass
// (lite/core/mir/fusion/hip_conv_tail_matcher.h; patches/0006 carries it with its SSAGraph adapter)
void GraphBuilder::Fuser::ConvTails() {
  using mir::fusion::TailInst;
  // A conv whose route has no fused tail (plhip_conv2d_fused_supported: the direct 3x3 stride-2 stem) keeps its separate
  // instructions.  ShuffleNetV2's stem -> max pool -> calib is the first program that asks.  Decided on the shape the program is
  // lowered for, like D, F and G; a feed resized so that a conv with a tail lands on that route is refused by the C ABI, loudly.
  auto takes_tail = [&](const GraphOp& op) {
    const auto it = op.inputs.empty() ? var_shape.end() : var_shape.find(op.inputs[0]);
    plhip_conv_desc d;
    return it == var_shape.end() || !ConvDesc(op, it->second, &d) || plhip_conv2d_fused_supported(&d) != 0;
  };
  std::vector<TailInst> prog(st.size());
  for (size_t i = 0; i < st.size(); ++i) {
    TailInst& t = prog[i];
    t.output = st[i].out;
    if (st[i].kind == StepKind::kOp) {
      const GraphOp& op = Op(i);
      t.inputs = st[i].op_inputs;
      if (op.type == "conv2d" && op.enable_int8 && !st[i].int8_out && takes_tail(op)) t.kind = TailInst::kConvF32;
      else if (op.type == "elementwise_add") t.kind = TailInst::kAdd;
      else if (op.type == "fusion_elementwise_add_activation" && op.act_type == "relu") t.kind = TailInst::kAddRelu;
      else if (op.type == "pool2d" && op.pooling_type == "max") t.kind = TailInst::kMaxPool;
    } else {
      t.inputs = {st[i].in};
      if (st[i].kind == StepKind::kCalibF2I) {
        t.kind = TailInst::kCalibF2I;
        t.calib_scale = st[i].scale;
      }
    }
  }
  mir::fusion::MatchConvTails(&prog);
  for (size_t i = 0; i < st.size(); ++i) {
    const TailInst& t = prog[i];
    dead[i] = t.dead;
    st[i].out = t.output;
    if (st[i].kind == StepKind::kOp) st[i].op_inputs = t.inputs;
    st[i].res = t.residual;
    st[i].res_relu = t.residual_relu;
    st[i].calib_out = t.calib_out;
    if (!t.calib_out.empty()) st[i].calib_scale = t.fused_calib_scale;
    st[i].drop_f32 = t.drop_f32;
    st[i].pool_int8 = t.pool_int8;
  }
}

// (I) a frame feed's image_resize takes the image_to_tensor behind it over, and with it the image_convert in front (the NV taps are
// converted as they are fetched) and, where it is the tensor's only reader (H2's condition), the calib[fp32_to_int8] behind: one
// launch, neither the converted frame nor the resized image nor the fp32 tensor is written.  H1 does not apply to a resized feed.
void GraphBuilder::Fuser::FrameResize() {
  for (size_t i = 0; i < st.size(); ++i) {
    if (!Live(i, StepKind::kImageResize) || Uses(st[i].out) != 1) continue;
    const int t = FindByInput(StepKind::kImageToTensor, st[i].out);
    if (t < 0) continue;
    int c = -1;
    for (size_t q = 0; q < st.size(); ++q)
      if (Live(q, StepKind::kImageConvert) && st[q].out == st[i].in) c = static_cast<int>(q);
    st[i].out = st[t].out;
    st[i].resize_tensor = true;
    dead[t] = true;
    if (c >= 0 && Uses(st[c].out) == 1) {
      st[i].in = st[c].in;
      st[i].resize_nv = true;
      dead[c] = true;
    }
    if (Uses(st[i].out) != 1) continue;
    const int k = FindByInput(StepKind::kCalibF2I, st[i].out);
    if (k < 0) continue;
    st[i].out = st[k].out;
    st[i].scale = st[k].scale;
    st[i].image_int8 = true;
    dead[k] = true;
  }
}

// (H1)'s condition on the reader j of the calib behind the image_to_tensor of feed f: an int8 conv2d without a tail that
// plhip_conv2d_image_supported takes on that image (the 3x3 stride-2 stem)
bool GraphBuilder::Fuser::StemTakesImage(int j, const FeedDesc& f) const {
  plhip_conv_desc d;
  if (!IsOp(j, "conv2d") || !Op(j).enable_int8 || !st[j].res.empty() || !st[j].calib_out.empty() || st[j].pw_op >= 0 ||
      !ConvDesc(Op(j), f.dims, &d))
    return false;
  plhip_image_desc img;
  memset(&img, 0, sizeof(img));
  img.n = d.n; img.h = d.h; img.w = d.w;
  img.format = f.image_format;
  for (int q = 0; q < 3; ++q) {
    img.means[q] = f.means[q];
    img.scales[q] = f.scales[q];
  }
  return plhip_conv2d_image_supported(&d, &img) != 0;
}

// (H) an image feed's image_to_tensor whose only reader is a calib[fp32_to_int8]: (H1) where that calib's only reader is a conv2d
// plhip_conv2d_image_supported takes, the conv takes both over and reads the uint8 image itself (the fp32 and the int8 image are
// never written); (H2) otherwise the calib folds into image_to_tensor (its int8 form).
void GraphBuilder::Fuser::ImageFeed() {
  for (size_t i = 0; i < st.size(); ++i) {
    if (!Live(i, StepKind::kImageToTensor) || Uses(st[i].out) != 1) continue;
    const int k = FindByInput(StepKind::kCalibF2I, st[i].out);
    if (k < 0) continue;
    const int j = SoleReader(st[k].out);
    if (StemTakesImage(j, g.feeds_[st[i].image_feed])) {  // (H1)
      st[j].in_calib_scale = st[k].scale;
      st[j].via_in = st[k].out;
      st[j].op_inputs[0] = st[i].in;
      st[j].image_feed = st[i].image_feed;
      dead[i] = dead[k] = true;
      continue;
    }
    st[i].out = st[k].out;  // (H2)
    st[i].scale = st[k].scale;
    st[i].image_int8 = true;
    dead[k] = true;
  }
}

// The input shapes D (mode 2), F and G ask the kernels' predicates about: propagated from the feeds through io_copy / calib / image
// steps, convs, kSameShapeOps, concat and split (anything else: shape unknown, no fusion)
void GraphBuilder::Fuser::PropagateShapes() {
  for (auto& f : g.feeds_) shape[f.name] = f.dims;
  for (size_t i = 0; i < st.size(); ++i) {
    if (dead[i]) continue;
    if (st[i].kind != StepKind::kOp) {  // io_copy / calib: same shape
      auto it = shape.find(st[i].in);
      if (it != shape.end()) shape[st[i].out] = it->second;
      continue;
    }
    const GraphOp& op = Op(i);
    if (st[i].op_inputs.empty()) continue;
    auto it = shape.find(st[i].op_inputs[0]);
    if (it == shape.end() || it->second.size() != 4) continue;
    const std::vector<int64_t> in = it->second;
    std::vector<int64_t> o;
    if (op.type == "conv2d" || op.type == "depthwise_conv2d") o = ConvOutShape(op, in);
    if (op.type == "conv2d_transpose") o = ConvTransposeOutShape(op, in);
    for (const char* same : kSameShapeOps)
      if (op.type == same) o = in;
    if (op.type == "concat") {  // every operand's shape must have come through
      std::vector<std::vector<int64_t>> ins;
      for (auto& v : st[i].op_inputs)
        if (shape.count(v)) ins.push_back(shape[v]);
      if (ins.size() == st[i].op_inputs.size()) o = ConcatOutShape(op, ins);
    }
    if (op.type == "split") {
      int axis = 0;
      const std::vector<int64_t> e = SplitExtents(op, in, &axis);
      for (size_t q = 0; q < st[i].outs.size(); ++q) {
        std::vector<int64_t> part = in;
        part[axis] = e[q];
        shape[st[i].outs[q]] = part;
      }
      continue;
    }
    if (o.empty()) continue;
    shape[st[i].out] = o;
    if (!st[i].calib_out.empty()) shape[st[i].calib_out] = o;
  }
}

// (D) depthwise_conv2d[int8_out] whose only consumer is a plain 1x1 conv (no tail of its own) takes it over.  Mode 2 (default):
// only where the fused kernel takes the pair on the depthwise conv's propagated input shape
void GraphBuilder::Fuser::DepthwisePointwise() {
  const bool kernel_only = g.fuse_dwpw_ == 2;
  for (size_t i = 0; i < st.size(); ++i) {
    if (!FusableDepthwise(i)) continue;
    const int j = SoleReader(st[i].out);
    if (!IsOp(j, "conv2d") || !IsPlain1x1Conv(Op(j)) || !st[j].res.empty() || !st[j].calib_out.empty() || st[j].drop_f32) continue;
    const int pw_cout = static_cast<int>(Op(j).w_dims[0]);
    plhip_conv_desc d;
    if (kernel_only && (!InputDesc(i, &d) || !plhip_dwpw_fused_supported(&d, pw_cout, st[j].int8_out ? PLHIP_OUT_I8 : PLHIP_OUT_F32)))
      continue;
    st[i].pw_op = st[j].op;
    st[i].pw_int8_out = st[j].int8_out;
    st[i].pw_out_scale = st[j].out_scale;
    st[i].via = st[i].out;
    st[i].out = st[j].out;
    dead[j] = true;
    // (E) ... and the global average pool2d that is the only reader of that conv's fp32 output, where the fused kernel writes
    // the plane average itself (PLHIP_OUT_F32_GAP): MobileNetV1's pw14 -> pool
    if (!kernel_only || st[i].pw_int8_out) continue;
    const int pj = SoleReader(st[i].out);
    if (!IsGlobalAvgPool(pj) || !plhip_dwpw_fused_supported(&d, pw_cout, PLHIP_OUT_F32_GAP)) continue;
    st[i].pw_pool = true;
    st[i].via_pw = st[i].out;
    st[i].out = st[pj].out;
    dead[pj] = true;
  }
}

// (F) a calib[fp32_to_int8] whose only reader is a conv2d that quantises while it stages its rows (plhip_conv2d_calib_supported:
// the 3x3 stride-2 stem) is taken over by that conv: the head of the MobileNet programs, the int8 image is never written
void GraphBuilder::Fuser::CalibIntoStem() {
  for (size_t i = 0; i < st.size(); ++i) {
    if (!Live(i, StepKind::kCalibF2I)) continue;
    const int j = SoleReader(st[i].out);
    if (!IsOp(j, "conv2d") || !Op(j).enable_int8 || !st[j].res.empty() || !st[j].calib_out.empty() || st[j].pw_op >= 0) continue;
    const auto it = shape.find(st[i].in);
    plhip_conv_desc d;
    if (it == shape.end() || !ConvDesc(Op(j), it->second, &d) || !plhip_conv2d_calib_supported(&d)) continue;
    st[j].in_calib_scale = st[i].scale;
    st[j].via_in = st[i].out;
    st[j].op_inputs[0] = st[i].in;
    dead[i] = true;
  }
}

// (G, opt-in) a depthwise_conv2d[int8_out] whose only reader is a 1x1 conv that D left alone — because it carries a fused tail
// (residual add, calib copy, dropped fp32 output) or because D's kernels do not take the shape — takes that conv over with
// its tail, where plhip_dw_conv1x1_fused_supported takes the propagated shapes: MobileNetV2's blocks
void GraphBuilder::Fuser::DepthwiseConv1x1Tail() {
  for (size_t i = 0; i < st.size(); ++i) {
    if (!FusableDepthwise(i)) continue;
    const int j = SoleReader(st[i].out);
    if (!IsOp(j, "conv2d") || st[j].op_inputs.size() != 1 || !IsPlain1x1Conv(Op(j)) || st[j].pool_int8 || st[j].in_calib_scale > 0.f)
      continue;
    // the one instruction runs where the depthwise conv ran: the residual operand must exist by then
    bool late = false;
    for (int t = static_cast<int>(i) + 1; t < j && !st[j].res.empty(); ++t)
      if (!dead[t] && (st[t].out == st[j].res || st[t].calib_out == st[j].res)) late = true;
    if (late) continue;
    plhip_conv_desc d;
    const plhip_out_kind out = st[j].int8_out ? PLHIP_OUT_I8 : PLHIP_OUT_F32;
    const int has_tail = !st[j].res.empty() || !st[j].calib_out.empty();
    if (!InputDesc(i, &d) || !plhip_dw_conv1x1_fused_supported(&d, static_cast<int>(Op(j).w_dims[0]), out, has_tail)) continue;
    st[i].pw_op = st[j].op;
    st[i].pw_tail = true;
    st[i].pw_int8_out = st[j].int8_out;
    st[i].pw_out_scale = st[j].out_scale;
    st[i].via = st[i].out;
    st[i].out = st[j].out;
    st[i].res = st[j].res;
    st[i].res_relu = st[j].res_relu;
    st[i].calib_out = st[j].calib_out;
    st[i].calib_scale = st[j].calib_scale;
    st[i].drop_f32 = st[j].drop_f32;
    dead[j] = true;
  }
}

// (J2) the excite chain behind a global average pool: calib -> conv 1x1 [int8_out] -> conv 1x1 [fp32_out] -> hard_sigmoid, each the
// only reader of the one before and the convs without a tail of their own, becomes one instruction in the calib's place
void GraphBuilder::Fuser::SeGate() {
  auto unary = [&](int t, const char* type) { return IsOp(t, type) && st[t].op_inputs.size() == 1; };
  auto plain_1x1 = [&](int t, bool int8_out) {
    return unary(t, "conv2d") && IsPlain1x1Conv(Op(t)) && st[t].int8_out == int8_out && st[t].res.empty() && st[t].calib_out.empty() &&
           !st[t].drop_f32 && st[t].pw_op < 0 && !(st[t].in_calib_scale > 0.f) && st[t].image_feed < 0;
  };
  for (size_t i = 0; i < st.size(); ++i) {
    if (dead[i] || !IsGlobalAvgPool(static_cast<int>(i))) continue;
    const int k = SoleReader(st[i].out);
    if (k < 0 || st[k].kind != StepKind::kCalibF2I) continue;
    const int a = SoleReader(st[k].out);
    if (!plain_1x1(a, true)) continue;
    const int b = SoleReader(st[a].out);
    if (!plain_1x1(b, false)) continue;
    const int gate = SoleReader(st[b].out);
    if (!unary(gate, "hard_sigmoid")) continue;
    const GraphOp &ca = Op(a), &cb = Op(b);
    if (cb.w_dims[1] != ca.w_dims[0] || cb.w_dims[0] != ca.w_dims[1]) continue;
    if (!plhip_se_gate_supported(static_cast<int>(ca.w_dims[1]), static_cast<int>(ca.w_dims[0]), ca.conv.act, cb.conv.act)) continue;
    st[k].kind = StepKind::kSeGate;
    st[k].via = st[k].out + "," + st[a].out + "," + st[b].out;
    st[k].out = st[gate].out;
    st[k].op = st[a].op;
    st[k].pw_op = st[b].op;
    st[k].out_scale = st[a].out_scale;
    dead[a] = dead[b] = dead[gate] = true;
  }
}

// (J1) (J3) (N) an untouched step of an op `takes` accepts whose fp32 output a calib[fp32_to_int8] reads takes that calib over: one
// launch writes the int8 tensor and, only where it has other readers, the fp32 one
void GraphBuilder::Fuser::CalibBehind(bool (*takes)(const GraphOp&)) {
  for (size_t i = 0; i < st.size(); ++i) {
    if (!Live(i, StepKind::kOp) || st[i].form != Form::kPlain || !st[i].calib_out.empty() || !takes(Op(i))) continue;
    if (TakeCalib(i, st[i].out, i + 1)) st[i].drop_f32 = Uses(st[i].out) == 0;
  }
}

// (J1) (J3) hard_swish / elementwise_mul
void GraphBuilder::Fuser::HardActCalib() {
  CalibBehind([](const GraphOp& op) { return op.type == "hard_swish" || op.type == "elementwise_mul"; });
}

// (K) concat(axis 1, two inputs of equal channels) whose only reader is a shuffle_channel(group 2): (K1) where that op's only reader
// is a split(axis 1) in two equal parts whose second output a calib[fp32_to_int8] reads, the concat step becomes the unit
// instruction: first half fp32, second half int8 and (only with another reader) fp32; (K2) where a calib[fp32_to_int8] reads the
// shuffled tensor itself, the concat step becomes shuffle_channel/int8.  The one instruction runs where the concat ran: both
// operands exist there, and everything it writes was written later before.
void GraphBuilder::Fuser::ShuffleTail() {
  const auto& shapes = var_shape;  // by graph variable: K needs the channels behind pools, which PropagateShapes does not follow
  for (size_t i = 0; i < st.size(); ++i) {
    if (dead[i] || !IsOp(static_cast<int>(i), "concat") || st[i].form != Form::kPlain) continue;
    const GraphOp& cat = Op(i);
    if (cat.inputs.size() != 2) continue;
    const auto a = shapes.find(cat.inputs[0]), b = shapes.find(cat.inputs[1]);
    if (a == shapes.end() || b == shapes.end() || a->second.size() != 4 || a->second != b->second) continue;
    if (cat.axis != 1 && cat.axis != -3) continue;
    const int j = SoleReader(st[i].out);
    if (!IsOp(j, "shuffle_channel") || Op(j).group != 2) continue;
    const int k = SoleReader(st[j].out);
    if (IsOp(k, "split")) {  // (K1)
      const GraphOp& sp = Op(k);
      const int64_t h = a->second[1];
      const bool halves = st[k].outs.size() == 2 && (sp.axis == 1 || sp.axis == -3) &&
                          (sp.num == 2 || (sp.num == 0 && sp.sections == std::vector<int>({static_cast<int>(h), static_cast<int>(h)})));
      if (!halves) continue;
      if (!TakeCalib(i, st[k].outs[1], k + 1)) continue;
      st[i].form = Form::kShuffleUnit;
      st[i].via = st[i].out + "," + st[j].out;
      st[i].out = st[k].outs[0];
      st[i].hi = st[k].outs[1];
      dead[j] = dead[k] = true;
      st[i].drop_f32 = Uses(st[i].hi) == 0;
      continue;
    }
    if (!TakeCalib(i, st[j].out, j + 1)) continue;  // (K2)
    st[i].form = Form::kShuffleInt8;
    st[i].via = st[i].out;
    st[i].out = st[j].out;
    dead[j] = true;
    st[i].drop_f32 = Uses(st[i].out) == 0;
  }
}

// (L) a concat K left alone whose output a calib[fp32_to_int8] reads (L1), and / or max pools whose only reader is such a calib
// (L2): the concat step writes the int8 copy itself, the pools run on it.  The one instruction runs where the concat ran; the
// pools stay where they were, behind it.
void GraphBuilder::Fuser::ConcatCalib() {
  auto same_bits = [](float a, float b) { return memcmp(&a, &b, sizeof a) == 0; };
  for (size_t i = 0; i < st.size(); ++i) {
    if (dead[i] || !IsOp(static_cast<int>(i), "concat") || st[i].form != Form::kPlain) continue;
    const std::string out = st[i].out;
    // D, taken at once: with D the step always becomes concat/int8, and a dead D changes no use count the pools below are asked about
    const bool direct = TakeCalib(i, out, i + 1);
    std::vector<std::pair<int, int>> pools;  // (pool, its calib)
    for (size_t t = i + 1; t < st.size(); ++t) {
      if (dead[t] || !IsOp(static_cast<int>(t), "pool2d") || st[t].pool_int8 || st[t].op_inputs.size() != 1 || st[t].op_inputs[0] != out) continue;
      if (Op(t).pooling_type != "max" || Op(t).global_pooling) continue;
      const int k = SoleReader(st[t].out);
      if (k >= 0 && st[k].kind == StepKind::kCalibF2I) pools.emplace_back(static_cast<int>(t), k);
    }
    if (!direct && pools.empty()) continue;
    const float scale = direct ? st[i].calib_scale : st[pools[0].second].scale;
    bool common = true;
    for (auto& pk : pools) common = common && same_bits(st[pk.second].scale, scale);
    if (!direct && !common) continue;  // no direct calib and no one scale for the int8 copy
    st[i].form = Form::kConcatInt8;
    if (!direct) {
      st[i].calib_out = out + "/precision_trans";
      st[i].calib_scale = scale;
    }
    for (auto& pk : pools) {
      if (!same_bits(st[pk.second].scale, scale)) continue;
      st[pk.first].op_inputs[0] = st[i].calib_out;
      st[pk.first].out = st[pk.second].out;
      st[pk.first].pool_int8 = true;
      dead[pk.second] = true;
    }
    st[i].drop_f32 = Uses(out) == 0;
  }
}

// (M) an interp whose only reader (fetches count) is an arg_max along axis 1: the interp step becomes the arg_max/interp instruction.
// It runs where the interp ran: its one operand exists there, and the labels were written later before.
void GraphBuilder::Fuser::InterpArgmax() {
  for (size_t i = 0; i < st.size(); ++i) {
    if (!Live(i, StepKind::kOp) || !IsInterp(Op(i)) || st[i].form != Form::kPlain || !st[i].calib_out.empty()) continue;
    const int j = SoleReader(st[i].out);
    if (!IsOp(j, "arg_max") || !(Op(j).axis == 1 || Op(j).axis == -3)) continue;
    st[i].form = Form::kArgmaxInterp;
    st[i].argmax_op = st[j].op;
    st[i].via = st[i].out;
    st[i].out = st[j].out;
    dead[j] = true;
  }
}

// (N) an interp M left alone, as J1 / J3
void GraphBuilder::Fuser::InterpCalib() { CalibBehind(IsInterp); }

// (O1) a concat(axis 1) all of whose operands come from transpose(0,2,3,1) -> reshape([0,-1,k]) chains of one k becomes concat/nhwc on
// the chains' NCHW inputs; it runs where the concat ran (every operand exists there).  (O2) a transpose(0,2,1) whose only reader is the
// Scores operand of a multiclass_nms disappears; the NMS reads the transpose's input through its strides.
void GraphBuilder::Fuser::DetectionHead() {
  for (size_t i = 0; i < st.size(); ++i) {
    if (dead[i] || !IsOp(static_cast<int>(i), "concat") || st[i].form != Form::kPlain) continue;
    const auto os = var_shape.find(Op(i).output);
    if (os == var_shape.end() || os->second.size() != 3 || !(Op(i).axis == 1 || Op(i).axis == -2)) continue;
    int k = 0;
    std::vector<int> chain;  // reshape, transpose per operand
    std::vector<std::string> srcs;
    bool ok = !st[i].op_inputs.empty();
    for (size_t q = 0; ok && q < st[i].op_inputs.size(); ++q) {
      const int r = SoleProducer(st[i].op_inputs[q], "reshape");
      if (r < 0) { ok = false; break; }
      const std::vector<int>& sh = Op(r).shape;
      ok = sh.size() == 3 && sh[0] == 0 && sh[1] == -1 && sh[2] > 0 && (k == 0 || sh[2] == k);
      if (!ok) break;
      k = sh[2];
      const int t = SoleProducer(st[r].op_inputs[0], "transpose");
      if (t < 0 || Op(t).perm != std::vector<int>({0, 2, 3, 1})) { ok = false; break; }
      // one operand twice would make its chain's variables have two uses: the use counts above already refuse it
      chain.push_back(r);
      chain.push_back(t);
      srcs.push_back(st[t].op_inputs[0]);
    }
    if (!ok) continue;
    for (size_t q = 0; q < chain.size(); q += 2) {
      st[i].via += (q ? "," : "") + st[chain[q + 1]].out + "," + st[chain[q]].out;
      dead[chain[q]] = dead[chain[q + 1]] = true;
    }
    st[i].op_inputs = srcs;
    st[i].form = Form::kConcatNhwc;
    st[i].nhwc_k = k;
  }
  for (size_t i = 0; i < st.size(); ++i) {
    if (dead[i] || !IsOp(static_cast<int>(i), "multiclass_nms") || st[i].scores_npc) continue;
    const int t = SoleProducer(st[i].op_inputs[1], "transpose");
    if (t < 0 || Op(t).perm != std::vector<int>({0, 2, 1})) continue;
    st[i].via = st[t].out;
    st[i].op_inputs[1] = st[t].op_inputs[0];
    st[i].scores_npc = true;
    dead[t] = true;
  }
}

// (P): see graph_builder.h
void GraphBuilder::Fuser::YoloHead() {
  auto plain_concat = [&](int t) {
    if (t < 0 || st[t].form != Form::kPlain) return false;
    const auto os = var_shape.find(Op(t).output);
    return os != var_shape.end() && os->second.size() == 3 && (Op(t).axis == 1 || Op(t).axis == -2);
  };
  for (size_t i = 0; i < st.size(); ++i) {
    if (dead[i] || !IsOp(static_cast<int>(i), "multiclass_nms") || st[i].scores_npc) continue;
    const int tr = SoleProducer(st[i].op_inputs[1], "transpose");
    if (tr < 0 || Op(tr).perm != std::vector<int>({0, 2, 1})) continue;
    std::vector<int> ys;  // the yolo_box steps in the boxes' order
    int cb = -1, cs = -1;
    const int y1 = SoleProducer(st[i].op_inputs[0], "yolo_box");
    if (y1 >= 0) {  // k = 1
      if (st[y1].outs.size() != 2 || st[y1].outs[0] != st[i].op_inputs[0] || st[y1].outs[1] != st[tr].op_inputs[0] || Uses(st[y1].outs[1]) != 1) continue;
      ys.push_back(y1);
    } else {
      cb = SoleProducer(st[i].op_inputs[0], "concat");
      cs = SoleProducer(st[tr].op_inputs[0], "concat");
      if (!plain_concat(cb) || !plain_concat(cs) || st[cb].op_inputs.size() != st[cs].op_inputs.size()) continue;
      bool ok = true;
      for (size_t q = 0; ok && q < st[cb].op_inputs.size(); ++q) {
        const int y = SoleProducer(st[cb].op_inputs[q], "yolo_box");
        ok = y >= 0 && st[y].outs.size() == 2 && st[y].outs[0] == st[cb].op_inputs[q] && st[y].outs[1] == st[cs].op_inputs[q] &&
             Uses(st[y].outs[1]) == 1 && std::find(ys.begin(), ys.end(), y) == ys.end();
        if (ok) ys.push_back(y);
      }
      if (!ok) continue;
    }
    if (ys.empty() || ys.size() > 8) continue;
    const GraphOp& a = Op(ys[0]);
    bool same = true;
    for (int y : ys) {
      const GraphOp& b = Op(y);
      same = same && st[y].op_inputs[1] == st[ys[0]].op_inputs[1] && b.class_num == a.class_num && b.conf_thresh == a.conf_thresh &&
             b.clip_bbox == a.clip_bbox && b.scale_x_y == a.scale_x_y && b.anchors.size() <= 32;
    }
    if (!same) continue;
    // the last of the yolo_box steps carries the instruction: every feature map has been written in front of it
    const int at = *std::max_element(ys.begin(), ys.end());
    Step head = st[at];
    head.form = Form::kYoloHead;
    head.yolo_ops.clear();
    head.op_inputs = {st[ys[0]].op_inputs[0], st[ys[0]].op_inputs[1]};
    head.via.clear();
    for (size_t q = 0; q < ys.size(); ++q) {
      head.yolo_ops.push_back(st[ys[q]].op);
      if (q) head.op_inputs.push_back(st[ys[q]].op_inputs[0]);
      if (cb >= 0) head.via += (q ? "," : "") + st[ys[q]].outs[0] + "," + st[ys[q]].outs[1];
      dead[ys[q]] = true;
    }
    head.via += (cb >= 0 ? "," + st[cs].out : st[ys[0]].outs[1]);
    head.op = head.yolo_ops[0];
    head.out = st[i].op_inputs[0];
    head.outs = {st[i].op_inputs[0], st[tr].out};
    st[at] = head;
    dead[at] = false;
    dead[tr] = true;
    if (cb >= 0) dead[cb] = dead[cs] = true;
  }
}

// The rewrites in the one order that gives today's programs.  Each takes over steps that a later one would otherwise match:
//   * I before H: H would take the image_to_tensor behind an image_resize (and its calib) and leave the resize a launch of its own.
//   * H before F: F would take the calib behind an image_to_tensor into the stem alone, and the fp32 tensor would still be written.
//   * conv tails before D and G: D must see the 1x1 conv's tail (res / calib_out / drop_f32) to leave that pair alone, G to carry it.
//   * shapes after the tails, I and H: they rename outputs and kill steps, and a dead step passes no shape on; before D, which asks
//     the kernels' predicates about them (as F and G do), and once: nothing behind changes the shape a live variable has.
//   * D (with E) before G: G is for the pairs D left alone (pw_op still < 0); F between them touches calibs and stems only.
//   * J2 and J1/J3 commute: J1/J3 take calibs that read a hard_swish / elementwise_mul, J2 the calib that reads a pool2d, and
//     neither changes a use count the other tests.  J2 stays first, as the letters were added.
//   * K behind every rewrite above: it takes calibs that read a shuffle_channel or a split, which none of them matches, and kills
//     no step they look at.
//   * L last: it is for the concats K left alone, and takes calibs that read a concat or a max pool behind one; C took the max
//     pools behind a conv long before.
//   * M and N behind L: they take an arg_max or a calib that reads an interp, which no rewrite above matches.  M first: an interp it
//     took has no fp32 output for N to quantise (and an interp that a calib reads too has two readers, so M leaves it to N).
//   * O last: it takes transposes and reshapes, which no rewrite above matches, in front of a concat that K and L left alone (a
//     concat whose output a calib reads stays L's) or of a multiclass_nms.
//   * P in front of O: O2 would fold the transpose P needs to see; P takes yolo_box ops and plain rank-3 concats of their outputs,
//     which no rewrite above matches (no calib reads them).
// A rewrite that turns a step into ONE other instruction sets its Step::form, and one that needs an untouched step asks
// form == kPlain.  That asks exactly what the flags of each form asked one by one: the forms of a concat step are set by K, L and
// O1 in that order, and each of them, and P's plain_concat, refused every form set before it; the one form of an interp step is
// M's, which M and N refused (N's calib_out is a modifier, so both still ask for it by name); the one form of a yolo_box step is
// P's, which nothing asks about.  A form never sits on a step of a type whose rewrite did not test for it before.
void GraphBuilder::FuseSteps(std::vector<Step>* steps, const std::map<std::string, std::vector<int64_t>>& shapes) {
  Fuser f(*this, steps, shapes);
  f.ConvTails();
  f.FrameResize();
  f.ImageFeed();
  if (fuse_dwpw_ == 2 || fuse_dwconv_) f.PropagateShapes();
  if (fuse_dwpw_) f.DepthwisePointwise();
  if (fuse_dwpw_ == 2) f.CalibIntoStem();
  if (fuse_dwconv_) f.DepthwiseConv1x1Tail();
  if (fuse_hard_act_) f.SeGate();
  if (fuse_hard_act_) f.HardActCalib();
  if (fuse_shuffle_) f.ShuffleTail();
  if (fuse_concat_) f.ConcatCalib();
  if (fuse_interp_argmax_) f.InterpArgmax();
  if (fuse_interp_calib_) f.InterpCalib();
  if (fuse_yolo_head_) f.YoloHead();
  if (fuse_detection_head_) f.DetectionHead();
  std::vector<Step> kept;
  for (size_t i = 0; i < steps->size(); ++i)
    if (!f.dead[i]) kept.push_back((*steps)[i]);
  steps->swap(kept);
}

std::vector<GraphBuilder::Step> GraphBuilder::Program() {
  auto steps = Schedule();
  const auto shapes = InferShapes();  // once per program: concat / split / shuffle_channel operands that do not fit fail here
  if (fuse_) FuseSteps(&steps, shapes);
  return steps;
}

std::string GraphBuilder::OpLine(const Step& s) const {
  const GraphOp& op = ops_[s.op];
  auto list_of = [](const char* key, const std::vector<float>& v) {
    std::string a = std::string(" ") + key + "=";
    for (size_t i = 0; i < v.size(); ++i) {
      char buf[32];
      snprintf(buf, sizeof buf, "%s%.9g", i ? "," : "", v[i]);
      a += buf;
    }
    return a;
  };
  // yolo_box/def, or (P) yolo_box/head: the attributes of every feature map, '|' between the maps
  auto yolo_line = [&](bool head) {
    std::string l = std::string("yolo_box/") + (head ? "head" : "def") + " in=" + Join(s.op_inputs) + " out=" + s.outs[0] + "," + s.outs[1];
    std::string anchors = " anchors=", ratios = " downsample_ratio=";
    const std::vector<int> self{s.op};
    const std::vector<int>& maps = head ? s.yolo_ops : self;
    for (size_t q = 0; q < maps.size(); ++q) {
      const GraphOp& y = ops_[maps[q]];
      anchors += (q ? "|" : "") + Join(y.anchors);
      ratios += (q ? "|" : "") + std::to_string(y.downsample_ratio);
    }
    l += anchors + " class_num=" + std::to_string(op.class_num);
    AppendNum(&l, "conf_thresh", op.conf_thresh);
    l += ratios + " clip_bbox=" + std::to_string(op.clip_bbox ? 1 : 0);
    AppendNum(&l, "scale_x_y", op.scale_x_y);
    return head ? l + " via=" + s.via : l;
  };
  auto interp_attrs = [](const GraphOp& o) {
    std::string a = o.out_h > 0 && o.out_w > 0 ? " size=" + std::to_string(o.out_h) + "x" + std::to_string(o.out_w) : std::string();
    if (a.empty()) AppendNum(&a, "by", o.interp_scale);
    return a + " align_corners=" + std::to_string(o.align_corners ? 1 : 0) + " align_mode=" + std::to_string(o.align_mode);
  };
  auto argmax_attrs = [](const GraphOp& o) {
    return " axis=" + std::to_string(o.axis) + " dtype=" + std::to_string(o.dtype) + " keepdims=" + std::to_string(o.keepdims ? 1 : 0);
  };
  switch (s.form) {  // the step that became ONE other instruction
    case Form::kShuffleInt8:
    case Form::kShuffleUnit: {
      const bool unit = s.form == Form::kShuffleUnit;
      std::string l = std::string("shuffle_channel/") + (unit ? "unit" : "int8") + " in=" + s.op_inputs[0] + "," + s.op_inputs[1] + " out=" + s.out;
      if (unit && !s.drop_f32) l += " +hi=" + s.hi;
      l += " +calib=" + s.calib_out;
      AppendNum(&l, "scale", s.calib_scale);
      if (!unit && s.drop_f32) l += " -f32";
      return l + " via=" + s.via + (unit && s.drop_f32 ? "," + s.hi : "");
    }
    case Form::kConcatInt8: {
      std::string l = "concat/int8 in=" + Join(s.op_inputs) + " out=" + s.out + " +calib=" + s.calib_out;
      AppendNum(&l, "scale", s.calib_scale);
      if (s.drop_f32) l += " -f32";
      return l + " axis=" + std::to_string(op.axis);
    }
    case Form::kConcatNhwc: return "concat/nhwc in=" + Join(s.op_inputs) + " out=" + s.out + " k=" + std::to_string(s.nhwc_k) + " via=" + s.via;
    case Form::kArgmaxInterp:
      return "arg_max/interp in=" + s.op_inputs[0] + " out=" + s.out + " +interp=" + op.type + interp_attrs(op) + argmax_attrs(ops_[s.argmax_op]) +
             " via=" + s.via;
    case Form::kYoloHead: return yolo_line(true);
    case Form::kPlain: break;
  }
  if (op.type == "yolo_box") return yolo_line(false);
  std::string l = op.type;
  if (op.enable_int8) {
    const bool fc = op.type == "fc";
    l += s.int8_out ? (fc ? "/int8out" : "/int8_out") : (fc ? "/fp32out" : "/fp32_out");
  } else {
    const bool tail_op = op.type == "hard_swish" || op.type == "elementwise_mul" || IsInterp(op);  // (J1) (J3) (N): the alias that carries a calib tail
    l += tail_op && !s.calib_out.empty() ? "/int8" : "/def";
  }
  l += " in=" + Join(s.op_inputs) + " out=" + s.out;
  for (size_t i = 1; i < s.outs.size(); ++i) l += "," + s.outs[i];
  if (op.type == "concat" || op.type == "split") l += " axis=" + std::to_string(op.axis);
  if (op.type == "split" && op.num > 0) l += " num=" + std::to_string(op.num);
  if (op.type == "split" && op.num <= 0) l += " sections=" + Join(op.sections);
  if (op.type == "shuffle_channel") l += " group=" + std::to_string(op.group);
  if (op.type == "conv2d_transpose" && !op.conv.output_size.empty())
    l += " output_size=" + std::to_string(op.conv.output_size[0]) + "x" + std::to_string(op.conv.output_size[1]);
  if (IsInterp(op)) l += interp_attrs(op);
  if (op.type == "arg_max") l += argmax_attrs(op);
  if (op.type == "transpose") l += " perm=" + Join(op.perm);
  if (op.type == "reshape") l += " shape=" + Join(op.shape);
  if (op.type == "prior_box") {
    l += list_of("min_sizes", op.min_sizes) + list_of("max_sizes", op.max_sizes) + list_of("aspect_ratios", op.aspect_ratios) +
         list_of("variances", op.variances) + " flip=" + std::to_string(op.flip ? 1 : 0) + " clip=" + std::to_string(op.clip ? 1 : 0);
    AppendNum(&l, "step_w", op.step_w);
    AppendNum(&l, "step_h", op.step_h);
    AppendNum(&l, "offset", op.offset);
    l += " min_max_aspect_ratios_order=" + std::to_string(op.min_max_aspect_ratios_order ? 1 : 0);
  }
  if (op.type == "box_coder") {
    l += " code_type=decode_center_size axis=" + std::to_string(op.axis) + " normalized=" + std::to_string(op.box_normalized ? 1 : 0);
    if (op.inputs.size() == 2 && !op.variances.empty()) l += list_of("variance", op.variances);
  }
  if (op.type == "multiclass_nms") {
    l += " background=" + std::to_string(op.background_label);
    AppendNum(&l, "score_threshold", op.score_threshold);
    l += " nms_top_k=" + std::to_string(op.nms_top_k);
    AppendNum(&l, "nms_threshold", op.nms_threshold);
    AppendNum(&l, "nms_eta", op.nms_eta);
    l += " keep_top_k=" + std::to_string(op.keep_top_k) + " normalized=" + std::to_string(op.nms_normalized ? 1 : 0) + " count=" + s.outs[1];
    if (s.scores_npc) l += " scores=npc via=" + s.via;  // (O2)
  }
  if (op.enable_int8 && s.int8_out) AppendNum(&l, "oscale", s.out_scale);
  if (s.image_feed >= 0) {  // (H1): image_to_tensor + calib taken over, the conv reads the uint8 image
    const FeedDesc& f = feeds_[s.image_feed];
    l += " +image_in=" + f.name + " fmt=" + operators::ImageFormatName(f.image_format);
    AppendNum(&l, "in_scale", s.in_calib_scale);
  } else if (s.in_calib_scale > 0.f) {
    l += " +calib_in=" + s.via_in;
    AppendNum(&l, "in_scale", s.in_calib_scale);
  }
  if (s.pw_tail) {  // (G): the 1x1 conv taken over, then its own fields as its unfused line had them
    l += std::string(" +conv1x1=conv2d/") + (s.pw_int8_out ? "int8_out" : "fp32_out") + " via=" + s.via;
    if (s.pw_int8_out) AppendNum(&l, "oscale", s.pw_out_scale);
  }
  if (!s.res.empty()) l += std::string(" +add=") + s.res + (s.res_relu ? " +relu" : "");
  if (!s.calib_out.empty()) {
    l += " +calib=" + s.calib_out;
    AppendNum(&l, "scale", s.calib_scale);
  }
  if (s.drop_f32) l += " -f32";
  if (s.pool_int8) l += " int8";
  if (s.pw_op >= 0 && !s.pw_tail) {
    l += std::string(" +pw=conv2d/") + (s.pw_int8_out ? "int8_out" : "fp32_out") + " via=" + s.via;
    if (s.pw_int8_out) AppendNum(&l, "pw_oscale", s.pw_out_scale);
    if (s.pw_pool) l += " +pool=avg/global pw_out=" + s.via_pw;
  }
  return l;
}

std::vector<std::string> GraphBuilder::Plan() {
  std::vector<std::string> lines;
  for (auto& s : Program()) {
    const std::string io = " in=" + s.in + " out=" + s.out;
    const FeedDesc* f = s.image_feed >= 0 ? &feeds_[s.image_feed] : nullptr;
    std::string l;
    switch (s.kind) {
      case StepKind::kOp: l = OpLine(s); break;
      case StepKind::kIoCopyH2D: l = "io_copy/host_to_device" + io; break;
      case StepKind::kIoCopyD2H: l = "io_copy/device_to_host" + io; break;
      case StepKind::kCalibF2I: l = "calib/fp32_to_int8" + io; break;
      case StepKind::kCalibI2F: l = "calib/int8_to_fp32" + io; break;
      case StepKind::kImageToTensor:
        l = std::string("image_to_tensor/") + (s.image_int8 ? "int8" : "fp32") + io + " fmt=" + operators::ImageFormatName(f->image_format);
        break;
      case StepKind::kSeGate: l = "hard_sigmoid/se_gate" + io + " via=" + s.via; break;  // (J2)
      case StepKind::kImageConvert:
        l = "image_convert/def" + io + " src=" + operators::FrameFormatName(f->frame_format) + " dst=BGR";
        break;
      case StepKind::kImageResize: {
        const bool frame_src = s.in == f->name + "/target_trans";  // else: the BGR image an image_convert of its own made
        char buf[64];
        snprintf(buf, sizeof buf, " %dx%d->%dx%d", f->frame_h, f->frame_w, static_cast<int>(f->dims[2]), static_cast<int>(f->dims[3]));
        l = std::string("image_resize/") + (!s.resize_tensor ? "uint8" : s.image_int8 ? "int8" : "fp32") + io + " src=" +
            (frame_src ? operators::FrameFormatName(f->frame_format) : operators::ImageFormatName(f->image_format)) + buf;
        break;
      }
    }
    if (s.kind == StepKind::kCalibF2I || s.kind == StepKind::kCalibI2F || s.kind == StepKind::kSeGate || s.image_int8) AppendNum(&l, "scale", s.scale);
    if (s.kind == StepKind::kSeGate) AppendNum(&l, "mid_scale", s.out_scale);
    lines.push_back(l);
  }
  return lines;
}

// The attributes AddConv takes for a conv step: the op's own, the kernel pick of Schedule() and what FuseSteps() made the conv take over
ConvAttrs GraphBuilder::LoweredConvAttrs(const Step& s) const {
  ConvAttrs a = ops_[s.op].conv;
  a.int8_out = s.int8_out;
  a.output_scale = s.int8_out ? s.out_scale : 1.f;
  a.residual = s.res;
  a.residual_relu = s.res_relu;
  a.calib_out = s.calib_out;
  a.calib_scale = s.calib_scale;
  a.drop_fp32 = s.drop_f32;
  a.in_calib_scale = s.in_calib_scale;
  if (s.image_feed >= 0) {  // (H1)
    const FeedDesc& f = feeds_[s.image_feed];
    a.image_format = f.image_format;
    for (int q = 0; q < 3; ++q) {
      a.image_means[q] = f.means[q];
      a.image_scales[q] = f.scales[q];
    }
    a.image_x = s.via_in;
  }
  if (s.pw_op >= 0) {
    const GraphOp& c = ops_[s.pw_op];
    a.pw_w = c.w.data();
    a.pw_w_dims = c.w_dims;
    a.pw_bias = c.has_bias ? c.bias.data() : nullptr;
    a.pw_weight_scale = c.conv.weight_scale;
    a.pw_output_scale = s.pw_int8_out ? s.pw_out_scale : 1.f;
    a.pw_int8_out = s.pw_int8_out;
    a.pw_act = c.conv.act;
    a.pw_act_coef = c.conv.act_coef;
    a.pw_pool = s.pw_pool;
    a.pw_tail = s.pw_tail;
  }
  return a;
}

void GraphBuilder::LowerOp(const Step& s, HipPredictor* pred) {
  GraphOp& op = ops_[s.op];
  const float* bias = op.has_bias ? op.bias.data() : nullptr;
  switch (s.form) {  // the step that became ONE other instruction
    case Form::kShuffleInt8: pred->AddShuffleUnit(s.op_inputs[0], s.op_inputs[1], "", s.out, s.calib_out, s.calib_scale, s.drop_f32); return;
    case Form::kShuffleUnit: pred->AddShuffleUnit(s.op_inputs[0], s.op_inputs[1], s.out, s.hi, s.calib_out, s.calib_scale, s.drop_f32); return;
    case Form::kConcatInt8: pred->AddConcatCalib(s.op_inputs, s.out, op.axis, s.calib_out, s.calib_scale, s.drop_f32); return;
    case Form::kConcatNhwc: pred->AddConcatNhwc(s.op_inputs, s.out, s.nhwc_k); return;
    case Form::kArgmaxInterp: {
      const GraphOp& am = ops_[s.argmax_op];
      pred->AddInterpArgMax(op.type, s.op_inputs[0], s.out, op.out_h, op.out_w, op.interp_scale, op.align_corners, op.align_mode, am.dtype,
                            am.keepdims);
      return;
    }
    case Form::kYoloHead: {
      std::vector<std::string> xs{s.op_inputs[0]};
      xs.insert(xs.end(), s.op_inputs.begin() + 2, s.op_inputs.end());
      std::vector<std::vector<int>> anchors;
      std::vector<int> ratios;
      for (int y : s.yolo_ops) {
        anchors.push_back(ops_[y].anchors);
        ratios.push_back(ops_[y].downsample_ratio);
      }
      pred->AddYoloHead(xs, s.op_inputs[1], s.outs[0], s.outs[1], anchors, op.class_num, op.conf_thresh, ratios, op.clip_bbox, op.scale_x_y);
      return;
    }
    case Form::kPlain: break;
  }
  if (op.type == "conv2d" || op.type == "depthwise_conv2d") {
    CHECK(op.enable_int8) << "kHIP has int8 conv kernels only";
    pred->AddConv(op.type, s.op_inputs[0], s.out, op.w.data(), op.w_dims, bias, LoweredConvAttrs(s));
  } else if (op.type == "conv2d_transpose") {
    CHECK(op.enable_int8) << "kHIP has int8 conv2d_transpose kernels only";
    CHECK(s.res.empty() && s.calib_out.empty() && s.pw_op < 0 && !(s.in_calib_scale > 0.f) && s.image_feed < 0 && !s.drop_f32)
        << "conv2d_transpose " << s.out << ": no rewrite of FuseSteps may hand it a tail or a front";
    pred->AddConvTranspose(s.op_inputs[0], s.out, op.w.data(), op.w_dims, bias, LoweredConvAttrs(s));
  } else if (op.type == "fc") {
    CHECK(op.enable_int8) << "kHIP has int8 fc kernels only";
    pred->AddFc(s.op_inputs[0], s.out, op.w.data(), static_cast<int>(op.w_dims[0]), static_cast<int>(op.w_dims[1]), bias,
                op.conv.input_scale, op.conv.weight_scale, s.int8_out ? s.out_scale : 1.f, s.int8_out, op.fc_relu);
  } else if (op.type == "pool2d") {
    pred->AddPool(s.op_inputs[0], s.out, op.pooling_type, op.ksize, op.pool_strides, op.pool_paddings,
                  op.global_pooling, op.exclusive, op.ceil_mode, s.pool_int8);
  } else if (op.type == "elementwise_add") {
    pred->AddElementwiseAdd(s.op_inputs[0], s.op_inputs[1], s.out, "");
  } else if (op.type == "fusion_elementwise_add_activation") {
    pred->AddElementwiseAdd(s.op_inputs[0], s.op_inputs[1], s.out, op.act_type);
  } else if (op.type == "softmax") {
    pred->AddSoftmax(s.op_inputs[0], s.out);
  } else if (op.type == "hard_swish" || op.type == "hard_sigmoid") {
    pred->AddActivation(op.type, s.op_inputs[0], s.out, s.calib_out, s.calib_scale, s.drop_f32);
  } else if (IsInterp(op)) {
    pred->AddInterp(op.type, s.op_inputs[0], s.out, op.out_h, op.out_w, op.interp_scale, op.align_corners, op.align_mode, s.calib_out,
                    s.calib_scale, s.drop_f32);
  } else if (op.type == "arg_max") {
    pred->AddArgMax(s.op_inputs[0], s.out, op.axis, op.dtype, op.keepdims);
  } else if (op.type == "transpose") {
    pred->AddTranspose(s.op_inputs[0], s.out, op.perm);
  } else if (op.type == "reshape") {
    pred->AddReshape(s.op_inputs[0], s.out, op.shape);
  } else if (op.type == "prior_box") {
    pred->AddPriorBox(s.op_inputs[0], s.op_inputs[1], s.outs[0], s.outs[1], op.min_sizes, op.max_sizes, op.aspect_ratios, op.variances, op.flip,
                      op.clip, op.step_w, op.step_h, op.offset, op.min_max_aspect_ratios_order);
  } else if (op.type == "box_coder") {
    const bool pv = s.op_inputs.size() == 3;
    pred->AddBoxCoder(s.op_inputs[0], pv ? s.op_inputs[1] : "", s.op_inputs.back(), s.out, pv ? std::vector<float>() : op.variances, op.axis,
                      op.box_normalized);
  } else if (op.type == "yolo_box") {
    CHECK(s.outs.size() == 2) << "yolo_box " << s.out << ": outputs {Boxes, Scores}";
    pred->AddYoloBox(s.op_inputs[0], s.op_inputs[1], s.outs[0], s.outs[1], op.anchors, op.class_num, op.conf_thresh, op.downsample_ratio,
                     op.clip_bbox, op.scale_x_y);
  } else if (op.type == "multiclass_nms") {
    CHECK(s.outs.size() >= 2 && s.outs[1] == s.out + "/count") << "multiclass_nms " << s.out << ": the count variable must be <out>/count";
    pred->AddMulticlassNms(s.op_inputs[0], s.op_inputs[1], s.out, s.outs.size() > 2 ? s.outs[2] : "", op.background_label, op.score_threshold,
                           op.nms_top_k, op.nms_threshold, op.nms_eta, op.keep_top_k, op.nms_normalized, s.scores_npc);
  } else if (op.type == "concat") {
    pred->AddConcat(s.op_inputs, s.out, op.axis);
  } else if (op.type == "split") {
    pred->AddSplit(s.op_inputs[0], s.outs.empty() ? std::vector<std::string>{s.out} : s.outs, op.axis, op.num, op.sections);
  } else if (op.type == "shuffle_channel") {
    pred->AddShuffleChannel(s.op_inputs[0], s.out, op.group);
  } else if (op.type == "elementwise_mul") {
    pred->AddElementwiseMul(s.op_inputs[0], s.op_inputs[1], s.out, op.axis, s.calib_out, s.calib_scale, s.drop_f32);
  } else {
    LOG(FATAL) << "GraphBuilder: no kHIP kernel for op type " << op.type;
  }
}

std::vector<std::string> GraphBuilder::Lower(HipPredictor* pred) {
  for (auto& f : feeds_) {
    if (f.image_format >= 0) pred->AddFeed(f.name, f.image_dims, PRECISION(kUInt8));
    else pred->AddFeed(f.name, f.dims, f.prec);
  }
  std::vector<std::string> outs;
  for (auto& s : Program()) {
    const FeedDesc* f = s.image_feed >= 0 ? &feeds_[s.image_feed] : nullptr;
    switch (s.kind) {
      case StepKind::kOp: LowerOp(s, pred); break;
      case StepKind::kIoCopyH2D: pred->AddIoCopy(s.in, s.out, true); break;
      case StepKind::kIoCopyD2H:
        pred->AddIoCopy(s.in, s.out, false);
        outs.push_back(s.out);
        break;
      case StepKind::kCalibF2I:
      case StepKind::kCalibI2F: pred->AddCalib(s.in, s.out, s.scale, s.kind == StepKind::kCalibF2I); break;
      case StepKind::kSeGate: {
        const GraphOp &ca = ops_[s.op], &cb = ops_[s.pw_op];
        CHECK(ca.conv.input_scale == s.scale && cb.conv.input_scale == s.out_scale) << "se_gate: scales of the chain disagree";
        pred->AddSeGate(s.in, s.out, s.scale, ca.w.data(), ca.w_dims, ca.has_bias ? ca.bias.data() : nullptr, ca.conv, cb.w.data(), cb.w_dims,
                        cb.has_bias ? cb.bias.data() : nullptr, cb.conv);
        break;
      }
      case StepKind::kImageConvert: pred->AddImageConvert(s.in, s.out, f->frame_format, PLHIP_IMG_BGR); break;
      case StepKind::kImageResize: {
        const bool frame_src = s.in == f->name + "/target_trans";  // else: the BGR image an image_convert of its own made
        pred->AddImageResize(s.in, s.out, frame_src ? f->frame_format : f->image_format, static_cast<int>(f->dims[2]),
                             static_cast<int>(f->dims[3]), s.resize_tensor ? f->means : nullptr, f->scales, s.image_int8 ? s.scale : 0.f);
        break;
      }
      case StepKind::kImageToTensor: pred->AddImageToTensor(s.in, s.out, f->image_format, f->means, f->scales, s.image_int8 ? s.scale : 0.f); break;
    }
  }
  return outs;
}

}  // namespace lite
}  // namespace paddle
