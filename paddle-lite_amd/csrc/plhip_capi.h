// plhip_capi.h — what the translation units of the C ABI (plhip_capi_*.hip) share: the context, the error text and the argument
// checks.  Internal to libplhip.so.
#pragma once
#include "../../include/plhip.h"

#include <hip/hip_runtime.h>
#include <stdio.h>
#include <string.h>

#include <vector>

#include "plhip_kernels.h"

// device copy of the resize tables of one (w_in, h_in, w_out, h_out): plhip_image_resize_tables' output for both axes
struct ResizeTables {
  int w_in, h_in, w_out, h_out;
  void* dev;  // [xofs][xcoef][yofs][ycoef], every section 64-byte aligned
  size_t xcoef_off, yofs_off, ycoef_off;
};

struct plhip_ctx {
  int device;
  hipStream_t stream;
  bool own_stream;
  char err[512];
  std::vector<ResizeTables> resize_tables;  // uint8 frame input: a few KB per frame size a context has seen
};

namespace plhip {

// writes the text plhip_last_error(c) returns (c == nullptr: the calling thread's) and returns st     (plhip_capi_ctx.hip)
plhip_status fail(plhip_ctx* c, plhip_status st, const char* fmt, const char* a = "", const char* b = "");

inline int cdiv(int a, int b) { return (a + b - 1) / b; }
inline int rup(int a, int b) { return cdiv(a, b) * b; }
inline bool aligned(const void* p, size_t a) { return ((uintptr_t)p & (a - 1)) == 0; }

// The output-kind / scale / activation checks of a compute entry point, in this order, `who` = its name in the texts.
// gap_ok: PLHIP_OUT_F32_GAP is one of its kinds; scale_name: what it calls the scale; act: nullptr = no activation enum to check
inline plhip_status check_out_scale_act(plhip_ctx* ctx, const char* who, plhip_out_kind out, bool gap_ok, const float* scale,
                                        const char* scale_name, const int* act, const char* act_name = "activation") {
  if (out != PLHIP_OUT_I32_ACC && out != PLHIP_OUT_F32 && out != PLHIP_OUT_I8 && !(gap_ok && out == PLHIP_OUT_F32_GAP))
    return fail(ctx, PLHIP_ERR_INVALID, "%s: bad out kind", who);
  if (out != PLHIP_OUT_I32_ACC && !scale) return fail(ctx, PLHIP_ERR_INVALID, "%s: %s required", who, scale_name);
  if (act && *act != PLHIP_ACT_NONE && *act != PLHIP_ACT_RELU && *act != PLHIP_ACT_RELU6 && *act != PLHIP_ACT_LEAKY_RELU)
    return fail(ctx, PLHIP_ERR_UNSUPPORTED, "%s: unsupported %s", who, act_name);
  return PLHIP_OK;
}

// ImageArgs of an image descriptor; false: a bad descriptor.  The image entry points and the image stem share it (plhip_capi_image.hip)
bool image_args(const plhip_image_desc* img, const uint8_t* src, ImageArgs* a);

}  // namespace plhip

using plhip::aligned;
using plhip::cdiv;
using plhip::check_out_scale_act;
using plhip::fail;
using plhip::image_args;
using plhip::rup;

#define HIPCHK(ctx, call)                                                                         \
  do {                                                                                            \
    hipError_t e_ = (call);                                                                       \
    if (e_ != hipSuccess) return fail((ctx), PLHIP_ERR_HIP, "%s failed: %s", #call, hipGetErrorString(e_)); \
  } while (0)

#define LAUNCHCHK(ctx, what)                                                                      \
  do {                                                                                            \
    hipError_t e_ = hipGetLastError();                                                            \
    if (e_ != hipSuccess) return fail((ctx), PLHIP_ERR_HIP, "launch %s failed: %s", what, hipGetErrorString(e_)); \
  } while (0)
