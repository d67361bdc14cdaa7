/* lite_capi.h — a small C veneer over the C++ kernel classes (lite/kernels/hip) and the mini predictor, so that
 * the Python test-suite and bench.py can drive the SAME objects a Paddle-Lite build would (KernelFactory lookup,
 * SetContext / SetParam / PrepareForRun / Launch) through ctypes.  Test / bench plumbing only; the drop-in ABI of
 * the device code is include/plhip.h.  Every function returns 0 or -1 (message in pllite_last_error()). */
#ifndef PLLITE_CAPI_H_
#define PLLITE_CAPI_H_
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

const char* pllite_last_error(void);
/* Number of kernels registered for (op_type, kHIP, precision, layout) — registry smoke check. */
int pllite_registered_kernels(const char* op_type, int precision, int layout);
/* Adopt an external hipStream_t (e.g. torch's current stream) as the calling thread's default execution stream on
 * `device`.  A predictor binds the default execution state (stream + workspace) of the thread that CREATES it and keeps
 * it for life: pllite_run / pllite_run_instruction may be called from any thread (one at a time per predictor — a
 * predictor is single-threaded like the reference's, program.cc:282-306) and always enqueue on that stream. */
int pllite_adopt_stream(int device, void* stream);

typedef struct pllite_predictor pllite_predictor;
pllite_predictor* pllite_predictor_create(int device);
void pllite_predictor_destroy(pllite_predictor* p);
int pllite_add_feed(pllite_predictor* p, const char* name, const int64_t* dims, int ndims, int precision);
int pllite_add_io_copy(pllite_predictor* p, const char* in, const char* out, int host_to_device);
int pllite_add_calib(pllite_predictor* p, const char* in, const char* out, float scale, int fp32_to_int8);
int pllite_add_conv(pllite_predictor* p, const char* op_type, const char* in, const char* out, const int8_t* w,
                    const int64_t* w_dims, const float* bias, const int* strides, const int* paddings, int n_paddings,
                    const int* dilations, int groups, int act, float act_coef, float input_scale,
                    const float* weight_scale, int n_weight_scale, float output_scale, int int8_out,
                    const char* padding_algorithm);
int pllite_add_fc(pllite_predictor* p, const char* in, const char* out, const int8_t* w, int k, int n, const float* bias,
                  float input_scale, const float* weight_scale, int n_weight_scale, float output_scale, int int8_out,
                  int relu);
int pllite_add_global_avg_pool(pllite_predictor* p, const char* in, const char* out);
int pllite_add_softmax(pllite_predictor* p, const char* in, const char* out);
int pllite_add_pool(pllite_predictor* p, const char* in, const char* out, const char* pooling_type, const int* ksize,
                    const int* strides, const int* paddings4, int global_pooling, int exclusive, int ceil_mode);
int pllite_add_elementwise_add(pllite_predictor* p, const char* x, const char* y, const char* out, const char* act_type);
/* op_type "hard_swish" | "hard_sigmoid" (the reference's default parameters); elementwise_mul: y is x's shape or [N, C, 1, 1] /
 * [N, C] at axis 0.  calib_out != NULL / "": the int8 alias, the calib[fp32_to_int8](calib_scale) behind the op in the same launch
 * writes that variable; drop_fp32: `out` is not written. */
int pllite_add_activation(pllite_predictor* p, const char* op_type, const char* in, const char* out, const char* calib_out,
                          float calib_scale, int drop_fp32);
int pllite_add_elementwise_mul(pllite_predictor* p, const char* x, const char* y, const char* out, int axis, const char* calib_out,
                               float calib_scale, int drop_fp32);
/* concat / split / shuffle_channel (fp32 ops, the reference's attributes) and the one-launch tail of a ShuffleNetV2 unit
 * (lite/kernels/hip/shuffle_fusion.h): lo NULL / "" = shuffle_channel/int8 (`hi` the shuffled tensor), else shuffle_channel/unit
 * (`lo` / `hi` the halves of the split); calib_out NULL / "" = no int8 image; drop_fp32: `hi` is not written. */
int pllite_add_concat(pllite_predictor* p, const char* const* inputs, int n_inputs, const char* out, int axis);
int pllite_add_split(pllite_predictor* p, const char* in, const char* const* outs, int n_outs, int axis, int num, const int* sections,
                     int n_sections);
int pllite_add_shuffle_channel(pllite_predictor* p, const char* in, const char* out, int group);
int pllite_add_shuffle_unit(pllite_predictor* p, const char* a, const char* b, const char* lo, const char* hi, const char* calib_out,
                            float calib_scale, int drop_fp32);
/* concat/int8 (lite/kernels/hip/concat_fusion.h): concat -> calib[fp32_to_int8](calib_scale) in one launch; `out` the fp32 tensor,
 * calib_out its int8 image (required); drop_fp32: `out` is not written. */
int pllite_add_concat_calib(pllite_predictor* p, const char* const* inputs, int n_inputs, const char* out, int axis, const char* calib_out,
                            float calib_scale, int drop_fp32);

/* ---- graph mode (lite/api/graph_builder.h): ops as the optimiser sees them after its fusion passes; kernel choice
 * (int8_out / fp32_out), io_copy and calib placement are decided by pllite_graph_lower() with the reference's rules.
 * One graph per predictor; ops in topological order. ---- */
int pllite_graph_feed(pllite_predictor* p, const char* name, const int64_t* dims, int ndims, int precision);
/* A feed that takes a decoded uint8 image [n, h, w, cs] instead of the normalised tensor (GraphBuilder::FeedImage): format ==
 * cv::ImageFormat (plhip_image_format), means / scales 3 floats each, indexed by the source byte of a pixel.  The ops name `name`
 * as the fp32 NCHW tensor; pllite_set_input(name, bytes) takes the image's n * h * w * cs bytes. */
int pllite_graph_feed_image(pllite_predictor* p, const char* name, int n, int h, int w, int format, const float* means,
                            const float* scales);
/* A feed that takes a decoder's / camera's frame (GraphBuilder::FeedFrame): n frames of src_h x src_w in src_format (a
 * plhip_image_format, or PLHIP_IMG_NV12 / NV21), converted and resized to dst_h x dst_w on the device and normalised like an image
 * feed.  pllite_set_input(name, bytes) takes the frames' bytes: n * src_h * src_w * cs, or n * src_h * 3 / 2 * src_w for NV. */
int pllite_graph_feed_frame(pllite_predictor* p, const char* name, int n, int src_h, int src_w, int src_format, int dst_h, int dst_w,
                            const float* means, const float* scales);
int pllite_graph_conv(pllite_predictor* p, const char* op_type, const char* in, const char* out, const int8_t* w,
                      const int64_t* w_dims, const float* bias, const int* strides, const int* paddings, int n_paddings,
                      const int* dilations, int groups, int act, float act_coef, float input_scale,
                      const float* weight_scale, int n_weight_scale, const char* padding_algorithm);
/* conv2d_transpose: w [cin][cout / groups][kh][kw] (w_dims), bias cout = w_dims[1] * groups floats or NULL, output_size 2 ints
 * (ConvParam::output_size) or NULL for the default.  Kernel pick as pllite_graph_conv; no fusion takes it. */
int pllite_graph_conv2d_transpose(pllite_predictor* p, const char* in, const char* out, const int8_t* w, const int64_t* w_dims,
                                  const float* bias, const int* strides, const int* paddings, int n_paddings, const int* dilations,
                                  int groups, int act, float act_coef, float input_scale, const float* weight_scale,
                                  int n_weight_scale, const int* output_size);
int pllite_graph_fc(pllite_predictor* p, const char* in, const char* out, const int8_t* w, int k, int n, const float* bias,
                    float input_scale, const float* weight_scale, int n_weight_scale, int relu);
int pllite_graph_pool(pllite_predictor* p, const char* in, const char* out, const char* pooling_type, const int* ksize,
                      const int* strides, const int* paddings4, int global_pooling, int exclusive, int ceil_mode);
int pllite_graph_elementwise_add(pllite_predictor* p, const char* x, const char* y, const char* out, const char* act_type);
int pllite_graph_softmax(pllite_predictor* p, const char* in, const char* out);
/* fp32 ops of MobileNetV3: op_type "hard_swish" | "hard_sigmoid"; elementwise_mul with y [N, C, 1, 1] / [N, C] (axis 0) or x's shape */
int pllite_graph_activation(pllite_predictor* p, const char* op_type, const char* in, const char* out);
/* runs the elementwise_mul kernel class's PrepareForRun on these shapes (no device needed): 0 taken, -1 refused (pllite_last_error) */
int pllite_elementwise_mul_prepare(const int64_t* x_dims, int nx, const int64_t* y_dims, int ny, int axis);
int pllite_graph_elementwise_mul(pllite_predictor* p, const char* x, const char* y, const char* out, int axis);
/* fusions J1 / J2 / J3 (hard_swish / elementwise_mul take the calib behind them over, hard_sigmoid the excite chain in front): off by
 * default, effective with pllite_graph_set_fuse(1) only */
int pllite_graph_set_fuse_hard_act(pllite_predictor* p, int on);
/* fp32 ops along an axis: concat of n_inputs >= 1 variables; split into n_outs variables, num > 0 equal parts or `sections` (one
 * per output); shuffle_channel(group).  Malformed graphs (other dims that differ, num / sections / group that do not fit, a
 * variable written twice) fail in pllite_graph_plan / pllite_graph_lower with a message. */
int pllite_graph_concat(pllite_predictor* p, const char* const* inputs, int n_inputs, const char* out, int axis);
int pllite_graph_split(pllite_predictor* p, const char* in, const char* const* outs, int n_outs, int axis, int num, const int* sections,
                       int n_sections);
int pllite_graph_shuffle_channel(pllite_predictor* p, const char* in, const char* out, int group);
/* bilinear_interp / nearest_interp (op_type) and arg_max with the reference's attributes: the output size is out_h x out_w where
 * both are > 0, else int(in * scale).  calib_out != NULL / "": the int8 alias (lite/kernels/hip/interp_fusion.h), the
 * calib[fp32_to_int8](calib_scale) behind the interp in the same launch writes that variable; drop_fp32: `out` is not written.
 * dtype: -1 or 3 int64 labels, 2 int32.  pllite_add_interp_arg_max: interp -> arg_max(axis 1) in one launch (arg_max/interp); `in`
 * is the interp's low-resolution input, the resampled tensor is no variable. */
int pllite_add_interp(pllite_predictor* p, const char* op_type, const char* in, const char* out, int out_h, int out_w, float scale,
                      int align_corners, int align_mode, const char* calib_out, float calib_scale, int drop_fp32);
int pllite_add_arg_max(pllite_predictor* p, const char* in, const char* out, int axis, int dtype, int keepdims);
int pllite_add_interp_arg_max(pllite_predictor* p, const char* op_type, const char* in, const char* out, int out_h, int out_w, float scale,
                              int align_corners, int align_mode, int dtype, int keepdims);
/* fusion K (concat -> shuffle_channel(2) -> [split ->] calib in one launch): on by default, effective with
 * pllite_graph_set_fuse(1) only; 0 keeps the separate instructions */
int pllite_graph_set_fuse_shuffle(pllite_predictor* p, int on);
/* fusion L (concat -> calib in one launch, the int8 max pool behind a concat): on by default, effective with
 * pllite_graph_set_fuse(1) only; 0 keeps the separate instructions */
int pllite_graph_set_fuse_concat(pllite_predictor* p, int on);
/* bilinear_interp / nearest_interp (op_type; out_h x out_w where both are > 0, else int(in * scale)) and arg_max along `axis`
 * (dtype -1 or 3: int64 labels, 2: int32), fp32 ops like pool2d.  Fusions M (interp -> arg_max(axis 1) in one launch) and N
 * (interp -> calib in one launch): each has a switch of its own, on by default, effective with
 * pllite_graph_set_fuse(p, 1) only. */
int pllite_graph_interp(pllite_predictor* p, const char* op_type, const char* in, const char* out, int out_h, int out_w, float scale,
                        int align_corners, int align_mode);
int pllite_graph_arg_max(pllite_predictor* p, const char* in, const char* out, int axis, int dtype, int keepdims);
int pllite_graph_set_fuse_interp_argmax(pllite_predictor* p, int on);
int pllite_graph_set_fuse_interp_calib(pllite_predictor* p, int on);
/* Detection heads (lite/kernels/hip/detection_compute.cc) with the reference's attributes.  transpose: rank 2 .. 4;
 * reshape: the shape attribute only (0 copies a dim, one -1 is inferred), no launch.  prior_box: Boxes and Variances
 * [H, W, prior_num, 4], computed on the host once per shape; max_sizes: none or one per min_size; variance: 4 values.  box_coder:
 * decode_center_size; prior_var NULL / "": the 4 values of variance4, or none where that is NULL.  multiclass_nms: the 3-D score form;
 * out [N, keep_top_k, 6] padded with -1, the per-image counts in the int32 variable "<out>/count", index (NULL / "": none)
 * [N, keep_top_k] int32; keep_top_k <= 0, nms_eta < 1 and shapes outside the device kernel's envelope (include/plhip.h) are
 * refused.  scores_npc (pllite_add_multiclass_nms): scores is [N, P, C].  pllite_add_concat_nhwc: transpose(0,2,3,1) ->
 * reshape([0,-1,k]) -> concat(axis 1) of NCHW inputs in one launch (concat/nhwc). */
int pllite_add_transpose(pllite_predictor* p, const char* in, const char* out, const int* perm, int rank);
int pllite_add_reshape(pllite_predictor* p, const char* in, const char* out, const int* shape, int rank);
int pllite_add_prior_box(pllite_predictor* p, const char* input, const char* image, const char* boxes, const char* variances,
                         const float* min_sizes, int n_min, const float* max_sizes, int n_max, const float* aspect_ratios, int n_ar,
                         const float* variance4, int flip, int clip, float step_w, float step_h, float offset,
                         int min_max_aspect_ratios_order);
int pllite_add_box_coder(pllite_predictor* p, const char* prior, const char* prior_var, const char* target, const char* out,
                         const float* variance4, int axis, int normalized);
int pllite_add_multiclass_nms(pllite_predictor* p, const char* boxes, const char* scores, const char* out, const char* index,
                              int background_label, float score_threshold, int nms_top_k, float nms_threshold, float nms_eta,
                              int keep_top_k, int normalized, int scores_npc);
int pllite_add_concat_nhwc(pllite_predictor* p, const char* const* inputs, int n_inputs, const char* out, int k);
int pllite_graph_transpose(pllite_predictor* p, const char* in, const char* out, const int* perm, int rank);
int pllite_graph_reshape(pllite_predictor* p, const char* in, const char* out, const int* shape, int rank);
int pllite_graph_prior_box(pllite_predictor* p, const char* input, const char* image, const char* boxes, const char* variances,
                           const float* min_sizes, int n_min, const float* max_sizes, int n_max, const float* aspect_ratios, int n_ar,
                           const float* variance4, int flip, int clip, float step_w, float step_h, float offset,
                           int min_max_aspect_ratios_order);
int pllite_graph_box_coder(pllite_predictor* p, const char* prior, const char* prior_var, const char* target, const char* out,
                           const float* variance4, int axis, int normalized);
int pllite_graph_multiclass_nms(pllite_predictor* p, const char* boxes, const char* scores, const char* out, const char* index,
                                int background_label, float score_threshold, int nms_top_k, float nms_threshold, float nms_eta,
                                int keep_top_k, int normalized);
/* yolo_box (YoloBoxParam): x [N, (n_anchors / 2) * (5 + class_num), H, W]; img_size a feed of precision 3 (int32) and dims [N, 2]
 * = (height, width) per image; anchors: n_anchors ints, (width, height) pairs; boxes [N, P, 4] and scores [N, P, class_num] with
 * P = (n_anchors / 2) * H * W. */
int pllite_graph_yolo_box(pllite_predictor* p, const char* x, const char* img_size, const char* boxes, const char* scores,
                          const int* anchors, int n_anchors, int class_num, float conf_thresh, int downsample_ratio, int clip_bbox,
                          float scale_x_y);
/* fusion P (k yolo_box ops -> the two concats -> the transpose in front of multiclass_nms's scores become ONE yolo_box/head
 * instruction; GraphBuilder::set_fuse_yolo_head) */
int pllite_graph_set_fuse_yolo_head(pllite_predictor* p, int on);
/* fusion O (the transpose -> reshape -> concat head join in one launch; the transpose in front of multiclass_nms's scores folded
 * into its strides): on by default, effective with pllite_graph_set_fuse(1) only */
int pllite_graph_set_fuse_detection_head(pllite_predictor* p, int on);
int pllite_graph_fetch(pllite_predictor* p, const char* name);
/* kHIP graph-level fusions (graph_builder.h set_fuse): on by default; 0 = the reference program instruction for instruction. */
int pllite_graph_set_fuse(pllite_predictor* p, int on);
// opt-in: depthwise_conv2d[int8_out] -> sole consumer conv2d 1x1 as ONE instruction (GraphBuilder::set_fuse_dwpw)
int pllite_graph_set_fuse_dwpw(pllite_predictor* p, int on);
// opt-in (default off): fusion G, depthwise_conv2d[int8_out] -> sole consumer conv2d 1x1 WITH its fused tail as ONE
// instruction (GraphBuilder::set_fuse_dwconv)
int pllite_graph_set_fuse_dwconv(pllite_predictor* p, int on);
/* '\n'-separated plan (GraphBuilder::Plan) — needs no device. */
int pllite_graph_plan(pllite_predictor* p, char* buf, int cap);
/* Emit the program into the predictor; '\n'-separated host names of the fetched variables in buf. */
int pllite_graph_lower(pllite_predictor* p, char* buf, int cap);
/* A predictor object that can only plan (no device needed): for CPU tests of the lowering rules. */
pllite_predictor* pllite_predictor_create_planner(void);

/* ---- model ingestion (lite/model_parser/hip_model.h): parses a PLHIPM01 container, applies the reference's
 * quant/dequant, conv+bn, conv+activation, fc and elementwise+activation fusion semantics and fills the predictor's
 * graph (then: pllite_graph_plan / pllite_graph_lower).  Needs no device. ---- */
int pllite_load_model(pllite_predictor* p, const void* bytes, int64_t nbytes, int batch);
/* The fused parameters of graph op `index` (conv2d / depthwise_conv2d / fc) for inspection: element counts through
 * n_w / n_bias / n_scale; arrays are copied when the pointers are non-null (capacity = the counts of a first call). */
int pllite_graph_num_ops(pllite_predictor* p);
int pllite_graph_op_params(pllite_predictor* p, int index, char* type, int type_cap, int8_t* w, int64_t* n_w, float* bias,
                           int* n_bias, float* weight_scale, int* n_scale, float* input_scale, int* act, float* act_coef);

int pllite_set_input(pllite_predictor* p, const char* name, const void* host, int64_t bytes);
int pllite_run(pllite_predictor* p, int skip_io_copy);
// the device part of the program as one recorded launch graph (first call records; needs one earlier pllite_run)
int pllite_run_graph(pllite_predictor* p);
int pllite_sync(pllite_predictor* p);
/* Per-instruction stepping (bench.py brackets single launches with HIP events for the roofline object). */
int pllite_num_instructions(pllite_predictor* p);
int pllite_run_instruction(pllite_predictor* p, int index);
/* Copies a variable (host or device resident) to `host`; returns bytes written through *bytes. */
int pllite_get_var(pllite_predictor* p, const char* name, void* host, int64_t capacity, int64_t* bytes,
                   int64_t* dims4, int* ndims);
/* Device pointer of a variable (for all_gather of logits etc.); 0 if it is not on the device. */
void* pllite_var_device_ptr(pllite_predictor* p, const char* name);
/* Asynchronous device-to-device copy of a device-resident variable into caller memory, on the predictor's stream. */
int pllite_copy_var_to_device(pllite_predictor* p, const char* name, void* dst_dev, int64_t bytes);
/* Times instruction `index` with profile::DeviceTimer<TargetType::kHIP> (lite/core/profile/timer.h): `reps` laps of
 * one launch each after one untimed launch; returns the average / minimum lap in ms and the kernel_func_name the kernel
 * reports through SetProfileRuntimeKernelInfo (lite/core/kernel.h:66-72). */
int pllite_time_instruction(pllite_predictor* p, int index, int reps, float* avg_ms, float* min_ms, char* func_name, int cap);
/* '\n'-separated "op:target/precision/layout/alias -> kernel_func_name" list of the program. */
int pllite_kernel_names(pllite_predictor* p, char* buf, int cap);

#ifdef __cplusplus
}
#endif
#endif
