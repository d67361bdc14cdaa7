/*
 * plhip.h — C ABI of the MI355X (gfx950) INT8 conv / depthwise / fc / calib backend.
 *
 * This is the drop-in boundary underneath the TARGET(kHIP)/PRECISION(kInt8) kernel classes in
 * paddle-lite_amd/lite/kernels/hip/ (which mirror lite/kernels/arm/{conv,fc,calib}_compute.cc of the
 * reference).  Each entry point names the reference interface it replaces (paths relative to the
 * reference tree).  Conventions:
 *   - every data pointer is a DEVICE pointer unless the name says host; the caller owns all buffers,
 *     the library never frees caller memory and allocates nothing inside a launch function;
 *   - calls are asynchronous on the context's HIP stream; plhip_stream_sync() waits;
 *   - return 0 on success, a negative plhip_status otherwise; the library never aborts (the C++
 *     kernel layer turns non-zero into LOG(FATAL), like CUDA_CALL in lite/backends/cuda/cuda_utils.h);
 *   - one plhip_ctx per host thread and GPU, not shared between threads
 *     (shape of lite/backends/cuda/context.h:35-140).
 * Tensors are dense NCHW; activations/weights int8, bias/scale fp32.  No torch types here.
 */
#ifndef PLHIP_H_
#define PLHIP_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef enum {
  PLHIP_OK = 0,
  PLHIP_ERR_INVALID = -1,     /* bad argument / inconsistent descriptor */
  PLHIP_ERR_HIP = -2,         /* a HIP runtime call failed (see plhip_last_error) */
  PLHIP_ERR_UNSUPPORTED = -3, /* configuration outside the implemented paths */
  PLHIP_ERR_WORKSPACE = -4,   /* workspace missing or too small */
  PLHIP_ERR_NO_DEVICE = -5    /* no HIP device / device is not gfx950 */
} plhip_status;

/* Output kind.  I32_ACC exists for the bit-exact accumulator check only. */
/* PLHIP_OUT_F32_GAP: the fp32 output averaged over each output plane, y = [n][cout] floats: the instruction pair
 * conv2d[fp32_out] -> pool2d(avg, global_pooling) (lite/backends/arm/math/pooling.cc:1006- pooling_global_avg) in the launch that
 * produces the plane; accepted by plhip_dwpw_fused_int8 / plhip_dwpw_fused_supported only (every other entry refuses it). */
typedef enum { PLHIP_OUT_I32_ACC = 0, PLHIP_OUT_F32 = 1, PLHIP_OUT_I8 = 2, PLHIP_OUT_F32_GAP = 3 } plhip_out_kind;

/* Activation codes == lite_api::ActivationType, lite/api/paddle_place.h:101-105. */
typedef enum { PLHIP_ACT_NONE = 0, PLHIP_ACT_RELU = 1, PLHIP_ACT_RELU6 = 2, PLHIP_ACT_LEAKY_RELU = 4 } plhip_act;

/* The kernel's whole shape contract == the fields of operators::ConvParam the ARM kernels read
 * (lite/operators/op_params.h:446-502): x dims, filter dims (OIHW, I = cin/groups), paddings
 * {top,bottom,left,right}, strides {h,w}, dilations {h,w}, groups, activation_param. */
typedef struct {
  int n, cin, h, w;
  int cout, kh, kw;
  int pad[4];
  int stride[2];
  int dil[2];
  int groups;
  int act;         /* plhip_act */
  float act_alpha; /* relu6: clip coefficient (already divided by out_scale for int8-out,
                      conv_gemmlike.cc:259-263); leaky: negative slope */
} plhip_conv_desc;

typedef struct plhip_ctx plhip_ctx;

/* ---- context / memory: replaces TargetWrapper<kCUDA> + CUDAContext for the new target
 *      (lite/backends/cuda/target_wrapper.h:27-85, lite/backends/cuda/context.h:35-140,
 *       lite/core/memory.{h,cc} TargetMalloc/TargetFree/TargetCopy). ---- */
int plhip_device_count(void);
plhip_status plhip_ctx_create(int device_id, plhip_ctx** out);
/* Adopt an existing hipStream_t (e.g. the caller's framework stream); not destroyed with the ctx. */
plhip_status plhip_ctx_create_on_stream(int device_id, void* hip_stream, plhip_ctx** out);
void plhip_ctx_destroy(plhip_ctx* ctx);
void* plhip_ctx_stream(plhip_ctx* ctx);
const char* plhip_last_error(plhip_ctx* ctx);
plhip_status plhip_malloc(plhip_ctx* ctx, size_t bytes, void** dev_ptr);
plhip_status plhip_free(plhip_ctx* ctx, void* dev_ptr);
plhip_status plhip_memcpy_h2d(plhip_ctx* ctx, void* dst_dev, const void* src_host, size_t bytes);
plhip_status plhip_memcpy_d2h(plhip_ctx* ctx, void* dst_host, const void* src_dev, size_t bytes);
plhip_status plhip_memcpy_d2d(plhip_ctx* ctx, void* dst_dev, const void* src_dev, size_t bytes);
plhip_status plhip_memset(plhip_ctx* ctx, void* dst_dev, int value, size_t bytes);
plhip_status plhip_stream_sync(plhip_ctx* ctx);
/* ---- launch graphs (no counterpart in the reference: its CUDA backend launches kernel by kernel) ----
 * Every compute entry point is asynchronous, allocation-free and argument-static, so a whole program step can be recorded
 * once and replayed: plhip_graph_begin puts the context's stream into capture (hipStreamBeginCapture, thread-local mode);
 * the caller issues its launches as usual; plhip_graph_end ends the capture and instantiates an executable graph;
 * plhip_graph_launch replays it on the context's stream (one submission instead of ~30, no per-kernel dispatch gap).
 * Pointers baked into the recorded launches must stay valid; anything that synchronises or allocates is illegal between
 * begin and end (the first, un-captured run of a program does the one-time work: weight packing, workspace, attributes). */
plhip_status plhip_graph_begin(plhip_ctx* ctx);
plhip_status plhip_graph_end(plhip_ctx* ctx, void** graph_exec);
plhip_status plhip_graph_launch(plhip_ctx* ctx, void* graph_exec);
plhip_status plhip_graph_destroy(plhip_ctx* ctx, void* graph_exec);
/* hipEvent timing on the context's stream (DeviceTimer<kCUDA> analogue, lite/core/profile/timer.h:127-158). */
plhip_status plhip_event_create(plhip_ctx* ctx, void** event);
plhip_status plhip_event_record(plhip_ctx* ctx, void* event);
plhip_status plhip_event_elapsed_ms(plhip_ctx* ctx, void* start, void* stop, float* ms);
plhip_status plhip_event_destroy(plhip_ctx* ctx, void* event);

/* ---- dense / grouped conv2d ----
 * Replaces: GemmLikeConv / DirectConv / WinogradConv <kInt8,*>::Run (lite/kernels/arm/conv_gemmlike.cc:
 * 325-462, conv_direct.cc:110-239, conv_winograd.cc:224-475) -> conv1x1s1_gemm_int8 / conv_im2col_gemm_int8
 * (lite/backends/arm/math/conv_impl.cc:260-331, 490-598) -> gemm_prepack_int8 (gemm_prepacked_int8.cc:
 * 5263-5457) with its fused epilogue (:643-796).
 *
 * Weight pre-pack replaces prepackA_int8 (gemm_prepacked_int8.cc:109-224) / trans_gemm_weights<kInt8>
 * (conv_block_utils.h:65-73): OIHW int8 -> per-group MFMA A-fragment order, zero padded.
 *
 * Grouped 3x3 ("conv_grouped3x3_int8_mfma32x32x32"): 3x3, dilation 1, stride (1,1) or (2,2), every padding 0 or 1,
 * groups >= 4, cin / groups == cout / groups in {4, 8, 16, 32} and cin % 32 == 0 (ResNeXt, RegNet), any n, h, w, every
 * output kind, activation and fused tail.  One launch on the input itself for all groups, where the reference loops
 * conv_im2col_gemm_int8's im2col + gemm_prepack_int8 over the groups (conv_impl.cc:490-598).  Packed weights: per chunk of 32
 * consecutive channels (32 / Cg whole groups) and filter tap one 32x32 MFMA A fragment, zero outside the groups' diagonal
 * blocks: (cin / 32) * 9 * 1024 bytes.  plhip_conv_workspace_bytes is 0 for it.  Other grouped shapes (groups 2, 1x1, dilated,
 * cin / groups != cout / groups) keep the per-group GEMMs of the 1x1 / im2col routes. */
size_t plhip_conv_packed_weight_bytes(const plhip_conv_desc* d);
plhip_status plhip_pack_conv_weights(plhip_ctx* ctx, const plhip_conv_desc* d,
                                     const int8_t* w_oihw, void* w_packed);
/* Scratch (0 for 1x1 s1 p0, the small-Cin 3x3 / 7x7 s2 stems and the grouped 3x3 route): the zero-padded input copy of the implicit-GEMM route
 * (dense k x k, stride 1 or 2, wide enough GEMM: ~1.1x the input) or the im2col buffer (everything else: kh*kw x the
 * input); replaces ctx.workspace_data (conv_gemmlike.cc:131).  The caller passes at least this many bytes, 16-byte aligned
 * (4 suffices for every route but the dense 3x3 patch kernel's padded / phase-split copy). */
size_t plhip_conv_workspace_bytes(const plhip_conv_desc* d);
/* scale/bias: folded per-output-channel fp32 arrays of length cout; bias may be NULL
 * (treated as zeros).  y: int32 / float / int8 NCHW according to `out`.  For PLHIP_OUT_I32_ACC scale,
 * bias and activation are ignored.  Name of the path taken (kernel_func_name analogue,
 * conv_gemmlike.cc:384): plhip_conv_impl_name(). */
plhip_status plhip_conv2d_int8(plhip_ctx* ctx, const plhip_conv_desc* d, const int8_t* x,
                               const void* w_packed, const float* scale, const float* bias, void* y,
                               plhip_out_kind out, void* workspace, size_t workspace_bytes);
const char* plhip_conv_impl_name(const plhip_conv_desc* d);
/* fp32-output conv with a fused graph tail (graph-level fusion on this target).  Replaces the
 * instruction run  conv2d[fp32_out] -> elementwise_add | fusion_elementwise_add_activation(relu) -> calib[fp32_to_int8]
 * of the reference's ResNet50 / MobileNetV2 programs (lite/kernels/arm/{conv,elementwise,calib}_compute.cc), any suffix
 * of it:   v = act(fma(float(acc), scale, bias));   if (residual) v = v + residual[i];   if (residual_relu) v = max(v, 0);
 *          if (y_f32) y_f32[i] = v;   if (y_i8) y_i8[i] = sat8(round_half_away(v * (1.f / calib_scale)))
 * Every value is rounded exactly as the separate instructions round it, so the results are bit-identical to running
 * them one by one.  residual / y_f32 / y_i8 have the output's NCHW shape; y_f32 may be NULL when only the int8 copy has
 * consumers.  The field ConvParam::residualData of the reference (lite/operators/op_params.h:446-502) is the operand. */
plhip_status plhip_conv2d_int8_fused(plhip_ctx* ctx, const plhip_conv_desc* d, const int8_t* x, const void* w_packed,
                                     const float* scale, const float* bias, float* y_f32, const float* residual,
                                     int residual_relu, int8_t* y_i8, float calib_scale, void* workspace,
                                     size_t workspace_bytes);
/* 1 where the route that runs `d` takes a residual operand / an int8 copy; 0 for a bad descriptor and for the direct 3x3
 * stride-2 stem, which has no fused tail (plhip_conv2d_int8_fused with a tail returns PLHIP_ERR_UNSUPPORTED there).  The graph
 * builder asks before it lets a conv take its tail over. */
int plhip_conv2d_fused_supported(const plhip_conv_desc* d);

/* ---- conv2d_transpose ----
 * Replaces: the int8 form of conv2d_transpose, which the reference states in deconv_basic<int8_t, int>
 * (lite/tests/utils/naive_math_impl.h:538-635: basic_gemm(trans_a) -> col2im -> fill_bias_relu; its ARM kernel,
 * lite/kernels/arm/conv_transpose_compute.cc, is fp32 only), with the shape rule of lite/operators/conv_transpose_op.cc:45-95.
 * The descriptor is a plhip_conv_desc whose cout is the OUTPUT channel count and whose filter is [cin][cout / groups][kh][kw]
 * (IOHW, no flip), plus ConvParam::output_size (lite/operators/op_params.h): out_h / out_w, 0 = the default
 *   OH = (h - 1) stride_h - pad_top - pad_bottom + dil_h (kh - 1) + 1        (the width alike);
 * an entry o with OH <= o < OH + stride_h replaces OH.  int32 accumulator
 *   acc[n, g Mg + m, iy sh - pt + r dh, ix sw - pl + s dw] += x[n, g Cg + c, iy, ix] * w[g Cg + c, m, r, s],
 * targets outside the output dropped, outputs no tap reaches 0; then plhip_conv2d_int8's epilogue, indexed by output channel.
 * Two routes (plhip_deconv_impl_name), no workspace, no atomics:
 *  - "deconv_phase_int8_mfma32x32x32": groups 1, cin % 32 == 0, dilation 1, kh, kw <= 4, stride (1,1) or (2,2), every padding
 *    < its kernel extent; any cout, n, h, w, output size, output kind and activation.  Per output phase ((oy + pt) % s,
 *    (ox + pl) % s) a stride-1 conv of the input with the phase's taps on v_mfma_i32_32x32x32_i8; the input rows are staged by
 *    the kernel itself.  Packed weights: one 32x32 MFMA A fragment per (32-output-channel tile, 32-input-channel chunk, tap),
 *    lane (m, h) byte j = w[32 chunk + 16 h + j][32 tile + m][r][s], zero for output channels >= cout:
 *    ceil(cout / 32) * (cin / 32) * kh * kw * 1024 bytes, 16-byte aligned.
 *  - "deconv_direct_int8": everything else (any groups incl. depthwise, dilation, stride, kernel size, cin), one lane per
 *    output over its valid taps: the slow path.  Packed weights: the filter itself, cin * cout / groups * kh * kw bytes.
 * PLHIP_ERR_INVALID: a dimension, stride or dilation < 1, a negative padding, groups that do not divide cin and cout, a
 * non-positive output, an output size outside [OH, OH + stride), PLHIP_OUT_F32_GAP.  PLHIP_ERR_UNSUPPORTED: cin * h * w or
 * n * cout * oh * ow >= 2^31.  There is no fused tail.  The call is asynchronous, allocation-free and argument-static
 * (capturable by plhip_graph_begin). */
typedef struct {
  plhip_conv_desc conv;
  int out_h, out_w; /* ConvParam::output_size, 0 = the default */
} plhip_deconv_desc;
plhip_status plhip_deconv_out_dims(const plhip_deconv_desc* d, int* out_h, int* out_w);
size_t plhip_deconv_packed_weight_bytes(const plhip_deconv_desc* d);
plhip_status plhip_pack_deconv_weights(plhip_ctx* ctx, const plhip_deconv_desc* d, const int8_t* w_iohw, void* w_packed);
plhip_status plhip_conv2d_transpose_int8(plhip_ctx* ctx, const plhip_deconv_desc* d, const int8_t* x, const void* w_packed,
                                         const float* scale, const float* bias, void* y, plhip_out_kind out);
const char* plhip_deconv_impl_name(const plhip_deconv_desc* d);

/* ---- calib[fp32_to_int8] + conv2d in one launch (graph-level fusion on this target) ----
 * Replaces the instruction pair  calib[fp32_to_int8](scale) ; conv2d 3x3 s2 (Cin <= 3)  at the head of the MobileNet programs
 * (lite/kernels/arm/calib_compute.cc:25-40 -> type_trans.cc:34-187 ; lite/kernels/arm/conv_direct.cc): x_f32 is the calib's
 * fp32 input [n, cin, h, w], calib_scale its scale; every value is quantised exactly as plhip_calib_f32_to_i8 does and
 * convolved exactly as plhip_conv2d_int8 does: bit-identical to the two calls, the int8 image never exists.  w_packed: what
 * plhip_pack_conv_weights made for `d`.  plhip_conv2d_calib_supported: 1 where the fused kernel takes the conv (3x3 stride 2,
 * cin <= 3, left padding 1, top padding <= 1, w % 4 == 0, ow % 4 == 0), else the caller runs the two instructions. */
int plhip_conv2d_calib_supported(const plhip_conv_desc* d);
plhip_status plhip_conv2d_calib_int8(plhip_ctx* ctx, const plhip_conv_desc* d, const float* x_f32, float calib_scale,
                                     const void* w_packed, const float* scale, const float* bias, void* y, plhip_out_kind out);

/* ---- uint8 image input (ImagePreprocess::image_to_tensor on the device) ----
 * Replaces ImagePreprocess::image_to_tensor (lite/utils/cv/paddle_image_preprocess.cc:143-172 -> Image2Tensor::choose,
 * lite/utils/cv/image2tensor.cc), the host step that turns a decoded image into the fp32 NCHW input tensor:
 *   y[b][c][h][w] = (float(src[((b * h + h) * w + w) * cs + c]) - means[c]) * scales[c]
 * two fp32 roundings (a subtract, then a multiply: image2tensor.cc:481-488, 549-563).  src is the interleaved image [n, h, w, cs],
 * cs = 4 (RGBA / BGRA, the 4th byte dropped), 3 (RGB / BGR) or 1 (GRAY); the output has 3 channels (1 for GRAY), channel c = byte c
 * of the pixel in the image's own order (no swap), and means / scales are indexed by that byte.  The int8 form quantises every value
 * exactly as plhip_calib_f32_to_i8 does (bit-identical to the two calls).  Any n, h, w >= 1; 16-byte aligned pointers and
 * h * w % 16 == 0 take the vector path, anything else a scalar one.  The descriptor is passed by pointer and read at the call:
 * the launches stay capture-safe. */
typedef enum { PLHIP_IMG_RGBA = 0, PLHIP_IMG_BGRA = 1, PLHIP_IMG_RGB = 2, PLHIP_IMG_BGR = 3, PLHIP_IMG_GRAY = 4 } plhip_image_format; /* == cv::ImageFormat */
typedef struct {
  int n, h, w;
  int format; /* plhip_image_format */
  float means[3];
  float scales[3];
} plhip_image_desc;
plhip_status plhip_image_to_tensor_f32(plhip_ctx* ctx, const plhip_image_desc* img, const uint8_t* src, float* y);
plhip_status plhip_image_to_tensor_i8(plhip_ctx* ctx, const plhip_image_desc* img, const uint8_t* src, int8_t* y, float calib_scale);
/* image_to_tensor + calib[fp32_to_int8](calib_scale) + conv2d 3x3 s2 in one launch: plhip_conv2d_calib_int8 with the uint8 image as
 * its source (conv_stem_u8in.hip), bit-identical to plhip_image_to_tensor_i8 followed by plhip_conv2d_int8.  Envelope: that of
 * plhip_conv2d_calib_supported, plus d->cin == the image's output channels and d->n, h, w == the image's.  Rows that start off a
 * dword (w * cs % 4 != 0) cannot occur inside it: w % 4 == 0 is part of that envelope.  src 4-byte aligned, w_packed 16, y 4
 * elements.  plhip_conv2d_image_supported: host logic only, 1 where the fused kernel takes the pair. */
int plhip_conv2d_image_supported(const plhip_conv_desc* d, const plhip_image_desc* img);
plhip_status plhip_conv2d_image_int8(plhip_ctx* ctx, const plhip_conv_desc* d, const plhip_image_desc* img, const uint8_t* src,
                                     float calib_scale, const void* w_packed, const float* scale, const float* bias, void* y,
                                     plhip_out_kind out);

/* ---- uint8 frame input (ImagePreprocess::imageConvert and imageResize on the device) ----
 * The two steps of ImagePreprocess in front of image_to_tensor (lite/utils/cv/paddle_image_preprocess.cc:44-98): a decoder's or
 * camera's frame, at its own size, becomes the network-sized interleaved image, or the input tensor itself, without leaving the
 * device.  Integer arithmetic fully given by the reference's library code; every result is bit-exact.
 *  - convert (image_convert.cc:175-518): an NV12 / NV21 frame is [n][h * 3 / 2][w] bytes, h rows of Y then h / 2 rows of chroma
 *    pairs, (u, v) for NV12, (v, u) for NV21, one pair per 2 x 2 luma block; w and h even.  ra = (179 (v - 128)) >> 7,
 *    ga = (44 (u - 128) + 91 (v - 128)) >> 7, ba = (227 (u - 128)) >> 7; b = clamp(y + ba), g = clamp(y - ga), r = clamp(y + ra);
 *    pixel bytes b, g, r.  Destination PLHIP_IMG_BGR, or PLHIP_IMG_BGRA with the 4th byte 255; anything else UNSUPPORTED.
 *  - resize (image_resize.cc:184-926): bilinear with 11-bit weights; per axis plhip_image_resize_tables gives, for each output
 *    index, a source index s (taps s and s + 1) and weights (c0, c1); source >= 2 per axis.  Per byte k of a pixel:
 *    rows0 = (S0[sx cs + k] a0 + S0[(sx + 1) cs + k] a1) >> 4, rows1 likewise one row below,
 *    dst = (((b0 rows0) >> 16) + ((b1 rows1) >> 16) + 2) >> 2.  GRAY / BGR / RGB / BGRA / RGBA, every byte alike; an NV frame is
 *    converted (b, g, r) tap by tap and resized as BGR, equal to convert then resize.  Equal sizes: a copy.
 *  - frame_to_tensor: resize, then image_to_tensor (above) of the resized image, in one launch; the resized image is never
 *    written.  img: the destination (n == the frame's, h, w, means, scales); img->format must be the frame's, or BGR for an NV
 *    frame.  Equal to plhip_image_convert_u8 -> plhip_image_resize_u8 -> plhip_image_to_tensor_* byte for byte.
 * NV21 / NV12 are FRAME formats only: plhip_image_desc keeps refusing them.  The tables of a (frame size, image size) pair are
 * uploaded on the first call that meets it (an allocation and a synchronous copy: make that call before a capture) and kept with
 * the context.  w_out % 16 == 0 and a 16-byte aligned y take the vector path, anything else a scalar one. */
enum { PLHIP_IMG_NV21 = 11, PLHIP_IMG_NV12 = 12 }; /* == cv::ImageFormat (lite/utils/cv/cv_enum.h:21-29) */
typedef struct {
  int n, h, w;
  int format; /* plhip_image_format, or PLHIP_IMG_NV21 / PLHIP_IMG_NV12 */
} plhip_frame_desc;
/* one axis, host only, no device: ofs[out], coef[out][2].  0, or -1 when in < 2, out < 1 or a pointer is null. */
int plhip_image_resize_tables(int in, int out, int32_t* ofs, int16_t* coef);
plhip_status plhip_image_convert_u8(plhip_ctx* ctx, const plhip_frame_desc* src, const uint8_t* x, int dst_format, uint8_t* y);
plhip_status plhip_image_resize_u8(plhip_ctx* ctx, const plhip_frame_desc* src, const uint8_t* x, int h_out, int w_out, uint8_t* y);
plhip_status plhip_frame_to_tensor_f32(plhip_ctx* ctx, const plhip_frame_desc* src, const plhip_image_desc* img, const uint8_t* x,
                                       float* y);
plhip_status plhip_frame_to_tensor_i8(plhip_ctx* ctx, const plhip_frame_desc* src, const plhip_image_desc* img, const uint8_t* x,
                                      int8_t* y, float calib_scale);

/* ---- depthwise conv (groups == cin == cout) ----
 * Replaces: DepthwiseConv<kInt8,*>::Run (lite/kernels/arm/conv_depthwise.cc:357-446) ->
 * conv_depthwise_3x3_int8_{fp32,int8} / conv_depthwise_5x5_int8_{fp32,int8}
 * (lite/backends/arm/math/conv_impl.cc:798-1184).  Weights are the raw OIHW [C,1,kh,kw] filter
 * (no re-layout needed on this target; cf. conv_trans_weights_numc, conv_block_utils.h:89). */
plhip_status plhip_depthwise_conv_int8(plhip_ctx* ctx, const plhip_conv_desc* d, const int8_t* x,
                                       const int8_t* w_oihw, const float* scale, const float* bias,
                                       void* y, plhip_out_kind out);

/* ---- fused depthwise 3x3 [int8_out] -> pointwise 1x1 (graph-level fusion) ----
 * Replaces the instruction pair  depthwise_conv2d[int8_out] ; conv2d 1x1 s1 p0 g1  of the MobileNet programs
 *  when the depthwise output has no other consumer.  Result is bit-identical to running
 * plhip_depthwise_conv_int8 (PLHIP_OUT_I8) followed by plhip_conv2d_int8; the int8 intermediate never leaves the CU.
 * dw: descriptor of the depthwise conv (groups == cin == cout, 3x3, stride 1|2, dilation 1); dw_scale / dw_bias: its
 * folded int8-out scale / bias; pw_cout, pw_w_packed (from plhip_pack_conv_weights of the 1x1 conv), pw_scale / pw_bias,
 * pw_act / pw_alpha describe the pointwise conv; y: [n, pw_cout, oh, ow] of kind `out`.
 * Returns PLHIP_ERR_UNSUPPORTED when the shape is outside the fused path (caller falls back to the two calls):
 * 3x3, stride 1 | 2, dilation 1, <= 1024 channels, a 128..1024-column tile touching <= 4 images, and 4 K-steps of the
 * tile's staged input rows (32 channels each) fitting the CU's LDS — plhip_dwpw_fused_supported answers that up front. */
int plhip_dwpw_fused_supported(const plhip_conv_desc* dw, int pw_cout, plhip_out_kind out);
plhip_status plhip_dwpw_fused_int8(plhip_ctx* ctx, const plhip_conv_desc* dw, const int8_t* x, const int8_t* dw_w_oihw,
                                   const float* dw_scale, const float* dw_bias, int pw_cout, const void* pw_w_packed,
                                   const float* pw_scale, const float* pw_bias, int pw_act, float pw_alpha, void* y,
                                   plhip_out_kind out);

/* ---- fused depthwise 3x3 [int8_out] -> 1x1 conv with the conv's graph tail (fusion G, graph-level fusion) ----
 * Replaces the instruction pair  depthwise_conv2d[int8_out] ; conv2d 1x1 s1 p0 g1 [+ residual add + calib]  of the MobileNetV2
 * blocks when the depthwise output has no other consumer.  Bit-identical to plhip_depthwise_conv_int8 (PLHIP_OUT_I8) followed by
 * plhip_conv2d_int8 (no tail) or plhip_conv2d_int8_fused (tail); the int8 intermediate never leaves the CU.
 * dw: the depthwise conv; dw_scale / dw_bias its folded int8-out scale / bias.  pw_cout, pw_w_packed (plhip_pack_conv_weights of
 * the 1x1 conv [n, C, oh, ow] -> pw_cout), pw_scale / pw_bias, pw_act / pw_alpha describe the 1x1 conv; y: [n, pw_cout, oh, ow]
 * of kind `out`.  The tail (residual, residual_relu, y_i8, calib_scale) has plhip_conv2d_int8_fused's meaning and needs
 * PLHIP_OUT_F32; y may then be NULL when y_i8 is set.
 * Envelope, all at run time: depthwise 3x3, channel multiplier 1 (groups == cin == cout), dilation 1, stride 1 or 2 (the same
 * in both directions), each padding 0 or 1, activation none / relu / relu6 / leaky; any n, h, w >= 1; cin % 16 == 0 and
 * cin <= 1024; pw_cout % 8 == 0 and pw_cout <= 1024; every element offset of the input and of the output below 2^31; out
 * PLHIP_OUT_I32_ACC, PLHIP_OUT_F32 or PLHIP_OUT_I8, and a tail only with PLHIP_OUT_F32.  Outside it the call returns
 * PLHIP_ERR_UNSUPPORTED and launches nothing; plhip_dw_conv1x1_fused_supported (host logic, no device query) answers the
 * same question up front (has_tail: 1 when a residual or a calib copy is requested). */
int plhip_dw_conv1x1_fused_supported(const plhip_conv_desc* dw, int pw_cout, plhip_out_kind out, int has_tail);
plhip_status plhip_dw_conv1x1_fused_int8(plhip_ctx* ctx, const plhip_conv_desc* dw, const int8_t* x,
                                         const int8_t* dw_w_oihw, const float* dw_scale, const float* dw_bias, int pw_cout,
                                         const void* pw_w_packed, const float* pw_scale, const float* pw_bias, int pw_act,
                                         float pw_alpha, void* y, plhip_out_kind out, const float* residual,
                                         int residual_relu, int8_t* y_i8, float calib_scale);

/* ---- fc ----
 * Replaces: FcCompute<kInt8,*>::Run (lite/kernels/arm/fc_compute.cc:229-344) -> gemm_s8 / gemv_int8
 * (lite/backends/arm/math/gemm_s8.cc:23-47, gemv_arm_int8.cc:701-760).
 * x [m,k] int8 row-major; w [k,n] int8 (Paddle "mul" layout); scale/bias per output column n.
 * Pre-pack (an opaque block of plhip_fc_packed_weight_bytes: a [k/4][n][4] copy for the dot4 kernels followed by the
 * MFMA A-fragment order, both zero padded) replaces the weight transpose of fc_compute.cc:53-62. */
/* `relu` is a flag word: bit 0 = fused relu; bit 1 (fp32 output only) = round twice, float(acc)*scale then + bias, as
 * the reference's gemm_s8 + fill_bias_fc route does (fc_compute.cc:250-266, taken there when m > 1 and the weight
 * scale is a single value); without it the epilogue is the single fused multiply-add of its gemv route. */
size_t plhip_fc_packed_weight_bytes(int k, int n);
plhip_status plhip_pack_fc_weights(plhip_ctx* ctx, int k, int n, const int8_t* w_kn, void* w_packed);
plhip_status plhip_fc_int8(plhip_ctx* ctx, int m, int k, int n, const int8_t* x, const void* w_packed,
                           const float* scale, const float* bias, int relu, void* y, plhip_out_kind out);

/* ---- calib (graph-edge precision casts) ----
 * Replaces: CalibComputeFp32ToInt8 / Int8ToFp32 (lite/kernels/arm/calib_compute.cc:25-57) ->
 * fp32_to_int8 / int8_to_fp32 (lite/backends/arm/math/type_trans.cc:34-187, 268-371), single scale. */
plhip_status plhip_calib_f32_to_i8(plhip_ctx* ctx, const float* x, int8_t* y, float scale, int64_t count);
plhip_status plhip_calib_i8_to_f32(plhip_ctx* ctx, const int8_t* x, float* y, float scale, int64_t count);

/* ---- fp32 glue ops of the MobileNet graph kept on device ----
 * Replaces: PoolCompute global-avg (lite/backends/arm/math/pooling.cc:1006-) and SoftmaxCompute
 * (lite/backends/arm/math/softmax.cc) for the tail pool2d -> calib -> fc -> softmax. */
plhip_status plhip_global_avg_pool_f32(plhip_ctx* ctx, const float* x, int nc, int spatial, float* y);
plhip_status plhip_softmax_f32(plhip_ctx* ctx, const float* x, int rows, int cols, float* y);

/* ---- fp32 glue ops of the ResNet50 / MobileNetV2 programs (both ops are fp32-only on the
 * reference's ARM target, so residual edges de/re-quantise through calib) ----
 * pool2d replaces PoolCompute::Run (lite/kernels/arm/pool_compute.cc:36-345) -> pooling_basic and its specialisations
 * (lite/backends/arm/math/pooling.cc:38-215): max, or avg with the exclusive flag, over windows clipped to the image;
 * paddings {top, bottom, left, right}; output dims are the caller's (PoolOutputSize, lite/operators/pool_op.h, incl.
 * ceil_mode).  x [n*c, h, w] -> y [n*c, oh, ow]. */
typedef struct {
  int planes, h, w, oh, ow;
  int kh, kw;
  int pad[4];
  int stride[2];
  int is_max;     /* 1 max, 0 avg */
  int exclusive;  /* avg: divide by the clipped window size (pooling.cc:160-164) */
} plhip_pool_desc;
plhip_status plhip_pool2d_f32(plhip_ctx* ctx, const plhip_pool_desc* d, const float* x, float* y);
/* int8 max pool: the kHIP graph fusion turns conv2d[fp32_out] -> pool2d(max) -> calib into conv+calib -> this (max
 * commutes with the monotonic quantiser of type_trans.cc:183-184, so y == calib(pool2d_f32(x_f32))). */
plhip_status plhip_pool2d_max_i8(plhip_ctx* ctx, const plhip_pool_desc* d, const int8_t* x, int8_t* y);
/* elementwise_add / fusion_elementwise_add_activation(relu), same-shape operands: replaces ElementwiseAddCompute /
 * ElementwiseAddActivationCompute (lite/kernels/arm/elementwise_compute.cc:85-140) -> elementwise_add{,_relu}<float>
 * (lite/backends/arm/math/elementwise.cc).  out may alias x or y. */
plhip_status plhip_elementwise_add_f32(plhip_ctx* ctx, const float* x, const float* y, float* out, int64_t count,
                                       int relu);

/* ---- the fp32 ops MobileNetV3 adds (hard_act.hip): the reference's int8 conv fuses relu / relu6 / leaky_relu only
 * (lite/core/mir/fusion/conv_activation_fuse_pass.cc:26-44), so these run as fp32 ops between the convs ----
 * plhip_hard_act_f32 replaces HardSwishCompute / HardSigmoidCompute (lite/kernels/arm/activation_compute.cc:150-195,
 * 319-345) -> act_hard_swish / act_hard_sigmoid<float> (lite/backends/arm/math/activation.cc:716-731, 678-691):
 *   PLHIP_HARD_SWISH    params {threshold, scale, offset}: min(max(0.f, x + offset), threshold) * x / scale, one add, one
 *                       multiply, one IEEE division, each rounded to fp32
 *   PLHIP_HARD_SIGMOID  params {slope, offset, unused}: t = x * slope + offset (two roundings); t < 1 ? t : 1; t > 0 ? t : 0
 * Outputs: y_f32 (fp32), y_i8 (the calib[fp32_to_int8] with calib_scale behind it, quantised exactly as
 * plhip_calib_f32_to_i8 does), or both in one launch; at least one is required, calib_scale > 0 with y_i8.  Any count;
 * 16-byte aligned fp32 pointers and a 4-byte aligned y_i8 take the vector path, anything else the scalar one. */
typedef enum { PLHIP_HARD_SWISH = 0, PLHIP_HARD_SIGMOID = 1 } plhip_hard_act_kind;
plhip_status plhip_hard_act_f32(plhip_ctx* ctx, plhip_hard_act_kind kind, const float* params, const float* x, float* y_f32,
                                int8_t* y_i8, float calib_scale, int64_t count);
/* elementwise_mul with a per-(image, channel) operand, the squeeze-excite gate: out[n][c][i] = x[n][c][i] * gate[n][c],
 * i < hw.  Replaces ElementwiseMulCompute's fast-broadcast case pre = 1, n = N * C, post = H * W
 * (lite/kernels/arm/elementwise_compute.cc:30-84).  hw = 1 is the same-shape product.  Outputs as plhip_hard_act_f32. */
plhip_status plhip_se_scale_f32(plhip_ctx* ctx, const float* x, const float* gate, int n, int c, int hw, float* y_f32,
                                int8_t* y_i8, float calib_scale);

/* The excite stage of a squeeze-excite block in ONE launch (se_gate.hip): pooled fp32 [n, c] (what plhip_global_avg_pool_f32
 * wrote) -> calib[fp32_to_int8](calib_scale) -> conv2d 1x1 c -> cr [int8_out, act1] -> conv2d 1x1 cr -> c [fp32_out, act2] ->
 * hard_sigmoid(slope, offset) -> gate fp32 [n, c]; bit-identical to the separate calls.  scale / bias are the convs' FOLDED
 * per-channel arrays exactly as plhip_conv2d_int8 takes them (conv 1: the int8_out form, its output scale is conv 2's input
 * scale); bias may be NULL.  Envelope (plhip_se_gate_supported): 8 <= c, cr <= 960, activations none / relu / relu6 / leaky.
 * Packed weights: plhip_se_gate_packed_weight_bytes bytes, 4-byte aligned, made from the two filters [cr][c] and [c][cr]. */
typedef struct {
  int n, c, cr;
  float calib_scale;
  int act1, act2;            /* plhip_act */
  float act1_alpha, act2_alpha;
  float slope, offset;       /* hard_sigmoid */
} plhip_se_gate_desc;
int plhip_se_gate_supported(int c, int cr, int act1, int act2);
size_t plhip_se_gate_packed_weight_bytes(int c, int cr);
plhip_status plhip_pack_se_gate_weights(plhip_ctx* ctx, int c, int cr, const int8_t* w1_cr_c, const int8_t* w2_c_cr, void* w_packed);
plhip_status plhip_se_gate_int8(plhip_ctx* ctx, const plhip_se_gate_desc* d, const float* pooled, const void* w_packed,
                                const float* scale1, const float* bias1, const float* scale2, const float* bias2, float* gate);

/* ---- the fp32 ops that join, part and permute tensors along an axis (shuffle_ops.hip).  All tensors are dense fp32.  An op
 * along `axis` of dims is described by outer = prod(dims[:axis]), the extent of each part along the axis, and inner =
 * prod(dims[axis+1:]).  fp32 values are moved: the output bits equal the input bits (NaN payloads, -0.0).  Where every row of
 * every operand starts 16-byte aligned (aligned bases, extent * inner a multiple of 4 for each part) a lane moves 16 bytes,
 * anything else takes a scalar path.  No call copies to the device or synchronises: all may be captured by plhip_graph_begin.
 *
 * plhip_concat_f32 replaces ConcatCompute (lite/kernels/arm/concat_compute.cc:37-57): `count` >= 1 inputs xs[i] of
 * [outer][extents[i]][inner] into y [outer][sum extents][inner].  outer, inner, extents[i] >= 1; xs, every xs[i], extents and y
 * non-null; outer * sum(extents) * inner <= 2^40 elements.  The input pointers travel in the kernel's arguments, 8 per launch: more inputs are several launches of the one
 * call.  xs / extents are host arrays, read before the call returns. */
plhip_status plhip_concat_f32(plhip_ctx* ctx, const float* const* xs, const int64_t* extents, int count, int64_t outer,
                              int64_t inner, float* y);
/* concat -> calib[fp32_to_int8] in ONE launch (the tail of a fire / inception module): the operands as plhip_concat_f32 takes
 * them, y_i8 [outer][sum extents][inner] = round_sat_i8((1.f / calib_scale) * v), the quantiser of plhip_calib_f32_to_i8, and,
 * where y_f32 is not NULL, y_f32 of the same shape with the input bits unchanged: byte for byte what plhip_concat_f32 followed
 * by plhip_calib_f32_to_i8 write.  Refused before any launch: count < 1, a NULL operand, an extent < 1, outer or inner < 1, NULL
 * y_i8, a calib_scale that is not a positive finite number, more than 2^40 elements.  A lane takes 16 consecutive floats of a row
 * (four 16-byte loads, one 16-byte int8 store) where every extents[i] * inner is a multiple of 16 and xs[i], y_f32, y_i8 are
 * 16-byte aligned; quads where they are multiples of 4 (y_i8 4-byte aligned); else elements.  Pointers travel in the kernel's
 * arguments, 8 per launch, as plhip_concat_f32's: no copy, no synchronise, capturable. */
plhip_status plhip_concat_calib_f32(plhip_ctx* ctx, const float* const* xs, const int64_t* extents, int count, int64_t outer,
                                    int64_t inner, float* y_f32, int8_t* y_i8, float calib_scale);
/* plhip_split_f32 replaces SplitCompute (lite/backends/arm/math/split.cc:54-82, shapes lite/operators/split_op.cc:32-75):
 * x [outer][extent][inner] into `count` >= 1 outputs ys[i] [outer][e_i][inner].  num > 0: equal parts, e_i = extent / num,
 * num must divide extent and count == num (sections is ignored, may be NULL); num == 0: e_i = sections[i] >= 1, which must add
 * up to extent; outer * extent * inner <= 2^40 elements.  Anything else is refused. */
plhip_status plhip_split_f32(plhip_ctx* ctx, const float* x, int64_t outer, int64_t extent, int64_t inner, int num,
                             const int64_t* sections, int count, float* const* ys);
/* plhip_shuffle_channel_f32 replaces ShuffleChannelCompute -> shuffle_channel<float>
 * (lite/backends/arm/math/shuffle_channel.cc:24-55): x [n][c][hw], out[b][j * group + i] = in[b][i * (c / group) + j].
 * n, c, hw, group >= 1, group divides c, n * c <= 2^30.  Outputs as plhip_hard_act_f32: y_f32, y_i8 (the calib[fp32_to_int8]
 * with calib_scale behind it, quantised exactly as plhip_calib_f32_to_i8 does: calib_scale > 0 required), or both; at least
 * one.  Vector path: hw % 4 == 0, x / y_f32 16-byte and y_i8 4-byte aligned. */
plhip_status plhip_shuffle_channel_f32(plhip_ctx* ctx, const float* x, int n, int c, int hw, int group, float* y_f32, int8_t* y_i8,
                                       float calib_scale);
/* The tail of a ShuffleNetV2 unit in ONE launch: concat([a, b], axis 1) -> shuffle_channel(group 2) -> split at channel split_at
 * -> calib[fp32_to_int8] of the second part; byte for byte what the four calls write.  a, b [n][h][hw] fp32, non-null.  Shuffled
 * channel c' in [0, 2 h) is (c' % 2 ? b : a)[c' / 2]; channels < split_at go to lo_f32 [n][split_at][hw], the rest to hi_f32
 * and / or hi_i8 [n][2 h - split_at][hw].  0 <= split_at <= 2 h; lo_f32 is NULL exactly when split_at == 0; with split_at < 2 h at
 * least one of hi_f32 / hi_i8 is required, with split_at == 2 h both are ignored; calib_scale > 0 with hi_i8.  n, h, hw >= 1,
 * n * h <= 2^29.  Vector path: hw % 4 == 0, fp32 pointers 16-byte and hi_i8 4-byte aligned. */
plhip_status plhip_shuffle_unit_f32(plhip_ctx* ctx, const float* a, const float* b, int n, int h, int hw, int split_at,
                                    float* lo_f32, float* hi_f32, int8_t* hi_i8, float calib_scale);

/* ---- dense prediction (interp_ops.hip): bilinear_interp / nearest_interp of fp32 NCHW planes, arg_max along an axis, and
 * interp -> arg_max(axis 1) in one launch.  Replaces lite/backends/arm/math/interpolate.cc:65-463 (bilinear), :465-499 (nearest)
 * and argmax.cc:29-61.  Per axis, with `in`, `out` and output index l, every operation one rounded fp32 operation (no FMA):
 *   ratio     align_corners ? (out > 1 ? float(in - 1) / float(out - 1) : 0.f) : float(in) / float(out)
 *   bilinear  f = float(l) * ratio                                with align_corners, and with align_mode 1 without
 *             f = max(ratio * (float(l) + 0.5f) - 0.5f, 0.f)      with align_mode 0 without align_corners
 *             i0 = min((int)f, in - 1), i1 = min(i0 + 1, in - 1), w1 = f - float(i0), w0 = 1.f - w1
 *             r0 = x[y0][x0] * a0 + x[y0][x1] * a1, r1 = x[y1][x0] * a0 + x[y1][x1] * a1, y = r0 * b0 + r1 * b1
 *   nearest   i = min((int)(double(ratio * float(l)) + 0.5), in - 1) with align_corners (a double addition),
 *             i = min((int)(ratio * float(l)), in - 1) without; align_mode is not read
 *   in == out on both axes copies the bits, whatever the method.
 * Refused before any launch, each with a text of its own: a NULL ctx, input or output; a dimension < 1; in_h, in_w, out_h, out_w
 * or c above 2^15; a method other than the two below, an align_corners or align_mode other than 0 / 1; with y_i8 a calib_scale
 * that is not a positive finite number; a dtype other than -1, 2, 3; more than 2^40 input or output elements.  No call copies
 * tables to the device or synchronises: all three may be captured by plhip_graph_begin. */
typedef enum { PLHIP_INTERP_BILINEAR = 0, PLHIP_INTERP_NEAREST = 1 } plhip_interp_method;
/* x [planes][in_h][in_w] (planes = N * C) -> y_f32 and / or y_i8 [planes][out_h][out_w]; at least one.  y_i8 is the quantiser of
 * plhip_calib_f32_to_i8 applied to the fp32 value, round_sat_i8((1.f / calib_scale) * v): byte for byte what this call with
 * y_f32 followed by plhip_calib_f32_to_i8 write.  A lane owns 4 consecutive outputs of a row (16-byte fp32 and 4-byte int8
 * stores) where out_w is a multiple of 4, y_f32 is 16-byte and y_i8 4-byte aligned; else one output. */
plhip_status plhip_interp_f32(plhip_ctx* ctx, const float* x, int64_t planes, int in_h, int in_w, int out_h, int out_w, int method,
                              int align_corners, int align_mode, float* y_f32, int8_t* y_i8, float calib_scale);
/* x [outer][c][inner] -> y [outer][inner], the index of the maximum along c; among equal maxima the LARGEST index (the reference
 * sorts (value, index) pairs with std::greater).  dtype -1 or 3: int64 labels, 2: int32.  A NaN never replaces the running
 * maximum, so the result is always in [0, c).  Quads of inner positions per lane where inner is a multiple of 4 and x, y are
 * 16-byte aligned. */
plhip_status plhip_arg_max_f32(plhip_ctx* ctx, const float* x, int64_t outer, int c, int64_t inner, void* y, int dtype);
/* x [n][c][in_h][in_w] -> y [n][out_h][out_w]: plhip_arg_max_f32 (axis 1) of plhip_interp_f32's output, which is never written.
 * The resampled values come from the device function plhip_interp_f32 uses and the comparison from plhip_arg_max_f32's, so the
 * labels equal the two calls' exactly.  A block stages the source tile of all c channels of its 32 x 32 output tile in LDS where
 * it fits 64 KB, and reads global memory otherwise. */
plhip_status plhip_interp_argmax_f32(plhip_ctx* ctx, const float* x, int n, int c, int in_h, int in_w, int out_h, int out_w,
                                     int method, int align_corners, int align_mode, void* y, int dtype);

/* ---- detection heads (transpose_ops.hip, detection_ops.hip): transpose, the one-launch join of an SSD head's feature maps,
 * box_coder (decode_center_size) and multiclass_nms.  Every entry point checks its arguments before any launch, each failure
 * with a text of its own; none synchronises with the host, copies tables or uses atomics, so all may be captured by
 * plhip_graph_begin and every result is a function of the inputs alone. ---- */
/* y = transpose(x, perm) (lite/kernels/arm/transpose_compute.cc): x fp32 of extents dims[rank], rank 2 .. 4, every extent >= 1,
 * at most 2^40 elements; perm a permutation of 0 .. rank - 1; axis k of y is axis perm[k] of x.  The bits are moved.  x and y
 * must not overlap.  Where the innermost source axis is not the innermost destination axis (NCHW -> NHWC, (0, 2, 1)) a block
 * moves 64 x 64 tiles through LDS, whole rows on both sides, 16 bytes per lane where both extents are multiples of 4 and both
 * bases 16-byte aligned. */
plhip_status plhip_transpose_f32(plhip_ctx* ctx, const float* x, const int64_t* dims, const int* perm, int rank, float* y);
/* transpose(0,2,3,1) -> reshape([0,-1,k]) -> concat(axis 1) of `count` NCHW tensors xs[i] [n][channels[i]][hw[i]] in ONE launch
 * (per 8 operands): y [n][sum channels[i] * hw[i]], operand i of image b as [hw[i]][channels[i]] behind the operands in front
 * of it; byte for byte what the three ops write, for every k that divides all channels[i]. */
plhip_status plhip_concat_nhwc_f32(plhip_ctx* ctx, const float* const* xs, const int64_t* channels, const int64_t* hw, int count,
                                   int64_t n, float* y);
/* box_coder, code_type decode_center_size (lite/kernels/arm/box_coder_compute.cc:92-158): target, y [rows][cols][4]; the prior
 * box of element (i, j) is row j of prior [cols][4] with axis 0 and row i of prior [rows][4] with axis 1; its variance is the
 * same row of prior_var when that is given, else variance4[0 .. 3] (host memory, read during the call) when that is given, else
 * none.  normalized == 0 adds 1 to widths and heights and subtracts it from the far corner.  fp32 in the reference's order of
 * operations with no contraction; exp is the library's expf.  One lane per box, 16-byte accesses where every base is aligned. */
plhip_status plhip_box_coder_decode_f32(plhip_ctx* ctx, const float* prior, const float* prior_var_or_null,
                                        const float* variance4_or_null, const float* target, int64_t rows, int64_t cols, int axis,
                                        int normalized, float* y);
/* multiclass_nms (lite/kernels/host/multiclass_nms_compute.cc:31-322), the 3-D score form, exact to the host algorithm:
 * a candidate needs score > score_threshold (a NaN never is one); candidates are ordered by descending score, equal scores (-0
 * and +0 are equal) by ascending prior; the list is cut at nms_top_k (negative: all); a candidate is kept iff
 * overlap <= nms_threshold against every box kept before it, overlap being JaccardOverlap as written there (0 for disjoint
 * boxes, area 0 for an inverted box, +1 on every extent with normalized == 0, inter / (a1 + a2 - inter); 0 / 0 = NaN suppresses);
 * background_label is skipped (-1: none); an image with more than keep_top_k kept boxes keeps the keep_top_k best by (score
 * descending, label, order of selection) and lists them by label.
 * Score of image i, class c, prior p: scores[i * C * P + c * score_stride_class + p * score_stride_prior] (strides in elements):
 * [N, C, P] is (P, 1), [N, P, C] is (1, C), so a transpose in front of the op can be folded away. */
typedef struct {
  int n, c, p;
  int64_t score_stride_class, score_stride_prior;
  int background_label;
  float score_threshold;
  int nms_top_k;
  float nms_threshold;
  float nms_eta;
  int keep_top_k;
  int normalized;
} plhip_nms_desc;
/* Device bytes plhip_multiclass_nms_f32 needs for desc (the classes' kept lists); 0 for a descriptor it refuses. */
size_t plhip_multiclass_nms_workspace_bytes(const plhip_nms_desc* desc);
/* boxes [N][P][4]; out [N][keep_top_k][6] rows (label, score, x1, y1, x2, y2), rows past an image's count filled with -1;
 * count [N] int32; index_or_null [N][keep_top_k] int32, i * P + prior, -1 past the count.  workspace: 8-byte aligned.
 * PLHIP_ERR_INVALID: a NULL pointer, a dimension < 1, keep_top_k <= 0 (it sizes the output), strides that leave the image's
 * C * P scores.  PLHIP_ERR_UNSUPPORTED, outside the envelope of the two kernels (each keeps its keys in one workgroup's LDS):
 *   nms_eta < 1 (the adaptive threshold);  P > 16384;  min(nms_top_k, P) > 4096;
 *   (classes other than the background) * min(nms_top_k, keep_top_k, P) > 16384;  N > 65535 or N * P >= 2^31.
 * SSD300 (P 1917, C 21, top 400, keep 200) and YOLOv3-416 (P 10647, C 80, top 1000, keep 100) are inside. */
plhip_status plhip_multiclass_nms_f32(plhip_ctx* ctx, const float* boxes, const float* scores, const plhip_nms_desc* desc,
                                      void* workspace, float* out, int* index_or_null, int* count);

/* ---- YOLOv3 heads (yolo_ops.hip): yolo_box (lite/backends/arm/math/yolo_box.cc:24-178) of one feature map in the reference's
 * output layout, and the head of up to 8 feature maps in one launch, written in the layout plhip_multiclass_nms_f32 reads.  x is
 * fp32 [n][an * (5 + c)][h][w]; img_size int32 [n][2] = (height, width) of every image, on the device; anchors: `an` (width,
 * height) pairs of int in HOST memory, read during the call and passed to the kernel by value (no table is copied; at most 16
 * pairs per feature map).  conf = sigmoid(objectness); a cell with conf < conf_thresh is skipped (a NaN is kept); its box and
 * scores are zeros.  The box centre uses h as the grid size on BOTH axes and downsample_ratio * h as the input size, as the
 * reference does; bias = -0.5 * (scale_x_y - 1) is computed in double and narrowed; clip_bbox clamps as `v > 0 ? v : 0` and
 * `v < img - 1 ? v : img - 1`, so a NaN becomes 0 and img - 1.  fp32 in the reference's order of operations with no contraction;
 * exp is the library's expf.  Every output element is written by the call, the zeros included: the outputs need no clearing.
 * Both check their arguments before any launch, each failure with a text of its own; PLHIP_ERR_INVALID: a NULL pointer, a
 * dimension < 1, an empty or odd anchor list, downsample_ratio < 1, count outside 1 .. 8; PLHIP_ERR_UNSUPPORTED: n * P * max(c, 4)
 * reaches 2^31 (P = the boxes of one image), downsample_ratio * h reaches 2^31, more than 16 anchor pairs in a feature map,
 * (head) c above 2^18.  No atomics, no host synchronisation: both may be captured by plhip_graph_begin. ---- */
/* boxes [n][an * h * w][4], one 16-byte store per box where boxes is 16-byte aligned; scores [n][an * h * w][c], the transposed
 * side: a block stages 64 cells x 64 classes in LDS, reads whole rows of x and writes whole rows of scores.  Box an_idx * h * w
 * + k * w + l is cell (row k, column l) of anchor an_idx. */
plhip_status plhip_yolo_box_f32(plhip_ctx* ctx, const float* x, const int* img_size, int n, int an, int c, int h, int w,
                                const int* anchors, float conf_thresh, int downsample_ratio, int clip_bbox, float scale_x_y,
                                float* boxes, float* scores);
/* `count` feature maps xs[i] [n][(anchor_lens[i] / 2) * (5 + c)][hs[i]][ws[i]] with anchors[i][0 .. anchor_lens[i] - 1] and
 * downsample_ratios[i] (the arrays in host memory, as plhip_concat_nhwc_f32's); img_size, c, conf_thresh, clip_bbox and scale_x_y
 * are shared.  ONE launch writes boxes [n][P][4] and scores [n][c][P], P = sum of (anchor_lens[i] / 2) * hs[i] * ws[i], feature
 * map i behind the ones in front of it: byte for byte plhip_yolo_box_f32 per feature map -> plhip_concat_f32 (axis 1) of the
 * boxes and of the scores -> plhip_transpose_f32 (0, 2, 1) of the scores, the per-cell arithmetic being the same device
 * functions.  A lane owns 4 consecutive cells of a row of x where hs[i] * ws[i] % 4 == 0 and xs[i], scores, every row of scores
 * (P % 4 == 0) and the feature map's offset into P are on 16 bytes, and one cell otherwise. */
plhip_status plhip_yolo_head_f32(plhip_ctx* ctx, const float* const* xs, const int* hs, const int* ws, const int* const* anchors,
                                 const int* anchor_lens, const int* downsample_ratios, int count, const int* img_size, int n, int c,
                                 float conf_thresh, int clip_bbox, float scale_x_y, float* boxes, float* scores);

/* ---- introspection used by tests: operand-layout self-check of the MFMA tile on this device.
 * Runs a tiny known-answer GEMM through the MFMA path; returns PLHIP_OK iff bit-exact. ---- */
plhip_status plhip_selftest(plhip_ctx* ctx);

/* ---- diagnostics: switches of the shipped library are set HERE, never through the environment, so that a stray variable
 * cannot change which kernel a benchmark measures.  Keys: the A/B knobs of DESIGN.md 3.6 without their former PLHIP_ prefix
 * ("GEMM_WIDE", "CONV_PATCH", "DW_STAGE", ...).  Each selects one of several kernels or tiles that compute the same result;
 * "DWCONV_FUSED" = 0: plhip_dw_conv1x1_fused_supported refuses every shape, so callers run the two instructions;
 * "CONV_GROUPED" = 0: the grouped 3x3 route takes no descriptor, grouped convs run im2col + one GEMM per group;
 * "DECONV_ROUTE" = 1: every conv2d_transpose runs the direct route (name, packed bytes, packer and run alike), 0 = automatic.  A
 * `make EXPERIMENTS=1` build also accepts "STAMPS" (in-kernel timelines).  Returns 0, or -1 for an unknown key. ---- */
int plhip_debug_set(const char* key, int value);

/* The launch plan (csrc/dw_plan.h) of a depthwise conv (kind 0: plhip_depthwise_conv_int8), of a fused depthwise -> pointwise
 * pair (kind 1: plhip_dwpw_fused_int8) or of a fused depthwise -> 1x1 conv (kind 2: plhip_dw_conv1x1_fused_int8) under the knobs
 * in force, as one line of text: "name <template parameters> grid=x,y block=.. lds=.. | <launch-plan fields>", or
 * "none why=<the entry point's error text>".  pw_cout, has_tail: the fused kinds; x_aligned: kind 2, the input pointer sits on
 * 4 bytes.  Host logic only: launches nothing, needs no context.  Returns the text's length, -1 for a bad kind or buffer. */
int plhip_debug_dw_plan(const plhip_conv_desc* dw, int kind /*0 depthwise, 1 D pair, 2 G pair*/, int pw_cout, int out, int has_tail,
                        int x_aligned, char* buf, size_t cap);

#ifdef __cplusplus
}
#endif
#endif /* PLHIP_H_ */
