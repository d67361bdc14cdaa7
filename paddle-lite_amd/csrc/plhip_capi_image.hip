// plhip_capi_image.hip — the C ABI (include/plhip.h), part 3 of 4: uint8 images (image_to_tensor) and camera frames (NV12 / NV21
// convert, bilinear resize) in front of a network.  The image stem itself (plhip_conv2d_image_int8) is a conv: plhip_capi_conv.hip.
#include <math.h>

#include "plhip_capi.h"

namespace plhip {
// ImagePreprocess::image_to_tensor (paddle_image_preprocess.cc:143-172 -> Image2Tensor::choose, image2tensor.cc:85-128): which
// formats exist and how many bytes a pixel has / how many channels come out
bool image_args(const plhip_image_desc* img, const uint8_t* src, ImageArgs* a) {
  if (!img || img->n < 1 || img->h < 1 || img->w < 1 || img->format < PLHIP_IMG_RGBA || img->format > PLHIP_IMG_GRAY) return false;
  a->src = src;
  a->n = img->n; a->h = img->h; a->w = img->w;
  a->cs = img->format == PLHIP_IMG_GRAY ? 1 : (img->format == PLHIP_IMG_RGB || img->format == PLHIP_IMG_BGR) ? 3 : 4;
  a->c = img->format == PLHIP_IMG_GRAY ? 1 : 3;
  for (int i = 0; i < 3; ++i) {
    a->mean[i] = img->means[i];
    a->scale[i] = img->scales[i];
  }
  return true;
}
}  // namespace plhip

extern "C" {

plhip_status plhip_image_to_tensor_f32(plhip_ctx* ctx, const plhip_image_desc* img, const uint8_t* src, float* y) {
  plhip::ImageArgs a;
  if (!ctx || !src || !y) return fail(ctx, PLHIP_ERR_INVALID, "plhip_image_to_tensor_f32: null argument");
  if (!image_args(img, src, &a)) return fail(ctx, PLHIP_ERR_INVALID, "plhip_image_to_tensor_f32: bad image descriptor");
  plhip::launch_image_to_tensor_f32(a, y, ctx->stream);
  LAUNCHCHK(ctx, "image_to_tensor_f32");
  return PLHIP_OK;
}

plhip_status plhip_image_to_tensor_i8(plhip_ctx* ctx, const plhip_image_desc* img, const uint8_t* src, int8_t* y, float calib_scale) {
  plhip::ImageArgs a;
  if (!ctx || !src || !y || !(calib_scale > 0.f)) return fail(ctx, PLHIP_ERR_INVALID, "plhip_image_to_tensor_i8: null / bad argument");
  if (!image_args(img, src, &a)) return fail(ctx, PLHIP_ERR_INVALID, "plhip_image_to_tensor_i8: bad image descriptor");
  plhip::launch_image_to_tensor_i8(a, y, calib_scale, ctx->stream);
  LAUNCHCHK(ctx, "image_to_tensor_i8");
  return PLHIP_OK;
}

// ------------------------------------------------------------------ uint8 frame input: convert + resize in front of image_to_tensor
// resize_table in image_resize.cc:57-117 (and the same lines inlined at :193-259 etc.), one axis: the double expression is rounded to
// float ONCE, floor, a float subtract, the two clamps, then SATURATE_CAST_SHORT.  No contraction: the sequence is the contract.
int plhip_image_resize_tables(int in, int out, int32_t* ofs, int16_t* coef) {
#pragma clang fp contract(off)
  if (in < 2 || out < 1 || !ofs || !coef) return -1;
  const double scale = static_cast<double>(in) / out;
  auto sat_short = [](float x) {
    const int v = static_cast<int>(x + (x >= 0.f ? 0.5f : -0.5f));
    return static_cast<int16_t>(v < -32768 ? -32768 : (v > 32767 ? 32767 : v));
  };
  for (int d = 0; d < out; ++d) {
    float f = static_cast<float>((d + 0.5) * scale - 0.5);
    int s = static_cast<int>(floorf(f));
    f -= s;
    if (s < 0) {
      s = 0;
      f = 0.f;
    }
    if (s >= in - 1) {
      s = in - 2;
      f = 1.f;
    }
    ofs[d] = s;
    coef[2 * d] = sat_short((1.f - f) * 2048.f);
    coef[2 * d + 1] = sat_short(f * 2048.f);
  }
  return 0;
}

static bool is_nv(int format) { return format == PLHIP_IMG_NV12 || format == PLHIP_IMG_NV21; }
static int pixel_bytes(int format) {  // 0 = not an interleaved format
  return format == PLHIP_IMG_GRAY ? 1 : (format == PLHIP_IMG_RGB || format == PLHIP_IMG_BGR) ? 3
         : (format == PLHIP_IMG_RGBA || format == PLHIP_IMG_BGRA) ? 4 : 0;
}
// nullptr = a valid frame, else what is wrong with it (*st says how)
static const char* frame_check(const plhip_frame_desc* f, plhip_status* st) {
  *st = PLHIP_ERR_INVALID;
  if (!f || f->n < 1 || f->n > 65535 || f->h < 1 || f->w < 1) return "bad frame descriptor";
  if (!is_nv(f->format) && !pixel_bytes(f->format)) return "unknown frame format";
  *st = PLHIP_ERR_UNSUPPORTED;
  if (is_nv(f->format) && ((f->h | f->w) & 1)) return "an NV12 / NV21 frame needs even w and h";
  if ((int64_t)f->h * f->w * 4 >= ((int64_t)1 << 31)) return "frame too large";
  return nullptr;
}

// The tables of (frame size -> image size) in device memory, made on first use and kept with the context.  The first use of a size
// allocates and copies (not capture-safe); every later one is a lookup.
static plhip_status resize_tables(plhip_ctx* ctx, int w_in, int h_in, int w_out, int h_out, plhip::ResizeArgs* a) {
  const ResizeTables* t = nullptr;
  for (auto& e : ctx->resize_tables)
    if (e.w_in == w_in && e.h_in == h_in && e.w_out == w_out && e.h_out == h_out) t = &e;
  if (!t) {
    auto r64 = [](size_t v) { return (v + 63) / 64 * 64; };
    ResizeTables e{w_in, h_in, w_out, h_out, nullptr, 0, 0, 0};
    e.xcoef_off = r64((size_t)w_out * 4);
    e.yofs_off = e.xcoef_off + r64((size_t)w_out * 4);
    e.ycoef_off = e.yofs_off + r64((size_t)h_out * 4);
    const size_t bytes = e.ycoef_off + r64((size_t)h_out * 4);
    std::vector<char> host(bytes, 0);
    if (plhip_image_resize_tables(w_in, w_out, reinterpret_cast<int32_t*>(host.data()), reinterpret_cast<int16_t*>(host.data() + e.xcoef_off)) ||
        plhip_image_resize_tables(h_in, h_out, reinterpret_cast<int32_t*>(host.data() + e.yofs_off), reinterpret_cast<int16_t*>(host.data() + e.ycoef_off)))
      return fail(ctx, PLHIP_ERR_UNSUPPORTED, "image resize: the source needs at least 2 rows and 2 columns");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    HIPCHK(ctx, hipMalloc(&e.dev, bytes));
    hipError_t st = hipMemcpyAsync(e.dev, host.data(), bytes, hipMemcpyHostToDevice, ctx->stream);
    if (st == hipSuccess) st = hipStreamSynchronize(ctx->stream);  // `host` dies with this scope
    if (st != hipSuccess) {
      (void)hipFree(e.dev);
      return fail(ctx, PLHIP_ERR_HIP, "image resize: table upload failed: %s", hipGetErrorString(st));
    }
    ctx->resize_tables.push_back(e);
    t = &ctx->resize_tables.back();
  }
  const char* d = static_cast<const char*>(t->dev);
  a->xofs = reinterpret_cast<const int32_t*>(d);
  a->xcoef = reinterpret_cast<const int16_t*>(d + t->xcoef_off);
  a->yofs = reinterpret_cast<const int32_t*>(d + t->yofs_off);
  a->ycoef = reinterpret_cast<const int16_t*>(d + t->ycoef_off);
  return PLHIP_OK;
}

static void resize_src(const plhip_frame_desc* f, const uint8_t* x, int h_out, int w_out, plhip::ResizeArgs* a) {
  a->src = x;
  a->n = f->n; a->h_in = f->h; a->w_in = f->w; a->h_out = h_out; a->w_out = w_out;
  a->nv = f->format == PLHIP_IMG_NV12 ? 1 : f->format == PLHIP_IMG_NV21 ? 2 : 0;
  a->cs = a->nv ? 3 : pixel_bytes(f->format);
  for (int i = 0; i < 3; ++i) {
    a->mean[i] = 0.f;
    a->scale[i] = 1.f;
  }
}

plhip_status plhip_image_convert_u8(plhip_ctx* ctx, const plhip_frame_desc* src, const uint8_t* x, int dst_format, uint8_t* y) {
  if (!ctx || !x || !y) return fail(ctx, PLHIP_ERR_INVALID, "plhip_image_convert_u8: null argument");
  plhip_status st;
  if (const char* why = frame_check(src, &st)) return fail(ctx, st, "plhip_image_convert_u8: %s", why);
  if (!is_nv(src->format)) return fail(ctx, PLHIP_ERR_UNSUPPORTED, "plhip_image_convert_u8: the source must be an NV12 / NV21 frame");
  if (dst_format != PLHIP_IMG_BGR && dst_format != PLHIP_IMG_BGRA)
    return fail(ctx, PLHIP_ERR_UNSUPPORTED, "plhip_image_convert_u8: an NV frame converts to BGR or BGRA only");
  plhip::NvArgs a{x, src->n, src->h, src->w, src->format == PLHIP_IMG_NV21 ? 1 : 0};
  plhip::launch_nv_to_bgr(a, y, dst_format == PLHIP_IMG_BGR ? 3 : 4, ctx->stream);
  LAUNCHCHK(ctx, "nv_to_bgr_u8");
  return PLHIP_OK;
}

plhip_status plhip_image_resize_u8(plhip_ctx* ctx, const plhip_frame_desc* src, const uint8_t* x, int h_out, int w_out, uint8_t* y) {
  if (!ctx || !x || !y) return fail(ctx, PLHIP_ERR_INVALID, "plhip_image_resize_u8: null argument");
  plhip_status st;
  if (const char* why = frame_check(src, &st)) return fail(ctx, st, "plhip_image_resize_u8: %s", why);
  if (h_out < 1 || w_out < 1 || (int64_t)h_out * w_out * 4 >= ((int64_t)1 << 31)) return fail(ctx, PLHIP_ERR_INVALID, "plhip_image_resize_u8: bad output size");
  if (!is_nv(src->format) && h_out == src->h && w_out == src->w) {  // image_resize.cc:905-915: a copy
    HIPCHK(ctx, hipMemcpyAsync(y, x, (size_t)src->n * src->h * src->w * pixel_bytes(src->format), hipMemcpyDeviceToDevice, ctx->stream));
    return PLHIP_OK;
  }
  plhip::ResizeArgs a;
  resize_src(src, x, h_out, w_out, &a);
  if (plhip_status rs = resize_tables(ctx, src->w, src->h, w_out, h_out, &a)) return rs;
  plhip::launch_image_resize(a, y, plhip::RESIZE_OUT_U8, 0.f, ctx->stream);
  LAUNCHCHK(ctx, "image_resize_u8");
  return PLHIP_OK;
}

static plhip_status frame_to_tensor(plhip_ctx* ctx, const char* who, const plhip_frame_desc* src, const plhip_image_desc* img,
                                    const uint8_t* x, void* y, int out, float calib_scale) {
  if (!ctx || !x || !y || (out == plhip::RESIZE_OUT_I8 && !(calib_scale > 0.f))) return fail(ctx, PLHIP_ERR_INVALID, "%s: null / bad argument", who);
  plhip_status st;
  if (const char* why = frame_check(src, &st)) return fail(ctx, st, "%s: %s", who, why);
  plhip::ImageArgs ia;
  if (!image_args(img, x, &ia) || (int64_t)img->h * img->w * 4 >= ((int64_t)1 << 31)) return fail(ctx, PLHIP_ERR_INVALID, "%s: bad image descriptor", who);
  if (img->n != src->n) return fail(ctx, PLHIP_ERR_INVALID, "%s: frame and image disagree on n", who);
  if (img->format != (is_nv(src->format) ? (int)PLHIP_IMG_BGR : src->format))
    return fail(ctx, PLHIP_ERR_UNSUPPORTED, "%s: the image's format must be the frame's, or BGR for an NV12 / NV21 frame", who);
  if (!is_nv(src->format) && img->h == src->h && img->w == src->w) {  // nothing to resize: image_to_tensor itself
    if (out == plhip::RESIZE_OUT_I8) plhip::launch_image_to_tensor_i8(ia, static_cast<int8_t*>(y), calib_scale, ctx->stream);
    else plhip::launch_image_to_tensor_f32(ia, static_cast<float*>(y), ctx->stream);
    LAUNCHCHK(ctx, "image_to_tensor");
    return PLHIP_OK;
  }
  plhip::ResizeArgs a;
  resize_src(src, x, img->h, img->w, &a);
  for (int i = 0; i < 3; ++i) {
    a.mean[i] = img->means[i];
    a.scale[i] = img->scales[i];
  }
  if (plhip_status rs = resize_tables(ctx, src->w, src->h, img->w, img->h, &a)) return rs;
  plhip::launch_image_resize(a, y, out, calib_scale, ctx->stream);
  LAUNCHCHK(ctx, "image_resize_to_tensor");
  return PLHIP_OK;
}

plhip_status plhip_frame_to_tensor_f32(plhip_ctx* ctx, const plhip_frame_desc* src, const plhip_image_desc* img, const uint8_t* x, float* y) {
  return frame_to_tensor(ctx, "plhip_frame_to_tensor_f32", src, img, x, y, plhip::RESIZE_OUT_F32, 0.f);
}

plhip_status plhip_frame_to_tensor_i8(plhip_ctx* ctx, const plhip_frame_desc* src, const plhip_image_desc* img, const uint8_t* x, int8_t* y,
                                      float calib_scale) {
  return frame_to_tensor(ctx, "plhip_frame_to_tensor_i8", src, img, x, y, plhip::RESIZE_OUT_I8, calib_scale);
}

}  // extern "C"
