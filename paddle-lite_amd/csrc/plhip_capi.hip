// plhip_capi.hip — the C ABI (include/plhip.h) over the gfx950 kernels: argument validation, path
// selection (the analogue of ConvCompute<kInt8,*>::PrepareForRun's impl_ choice,
// lite/kernels/arm/conv_compute.cc:87-185) and launches.  No allocation and no synchronisation happens
// inside a compute entry point, so callers may capture them into a hipGraph.
#include "../../include/plhip.h"

#include <hip/hip_runtime.h>
#include <math.h>
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

namespace {

thread_local char g_err[512] = "";

plhip_status fail(plhip_ctx* c, plhip_status st, const char* fmt, const char* a = "", const char* b = "") {
  char* dst = c ? c->err : g_err;
  snprintf(dst, 512, fmt, a, b);
  return st;
}

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

inline int cdiv(int a, int b) { return (a + b - 1) / b; }
inline int rup(int a, int b) { return cdiv(a, b) * b; }

enum ConvImpl { IMPL_GEMM_1X1 = 0, IMPL_DIRECT_3X3S2 = 1, IMPL_IM2COL_GEMM = 2, IMPL_IMPLICIT_GEMM = 3, IMPL_PATCH_GEMM = 4, IMPL_PATCH_S2 = 5, IMPL_STEM_7X7S2 = 6 };

struct ConvGeom {
  int oh, ow, G, Mg, Cg, Kg, N, Np, MA, MT, MT32, KS;
  bool is_1x1_s1_p0;
  ConvImpl impl;  // a pure function of the descriptor, so that pack and run agree
};

static bool implicit_gemm_disabled() {  // knob IMPLICIT_GEMM = 0: A/B runs against the im2col route
  return plhip::knob("IMPLICIT_GEMM", 1) == 0;
}
// dims of the padded copy of the implicit-GEMM route: stride 1 the padded plane; stride 2 ONE of the 4 phase planes
// (rows / columns 2y + p, 2x + q of the padded plane), its rows padded to a multiple of 4 columns
static void padded_dims(const plhip_conv_desc* d, int* ph, int* pw) {
  const int PH = d->h + d->pad[0] + d->pad[1], PW = d->w + d->pad[2] + d->pad[3];
  if (d->stride[0] == 2) {
    *ph = (PH + 1) / 2;
    *pw = rup((PW + 1) / 2, 4);
  } else {
    *ph = PH;
    *pw = PW;
  }
}
// the padded copy of the patch route (conv_patch_i8.hip): rows of PWp (a multiple of 8) bytes, + slack for the tiles that run
// past the last plane
static size_t patch_input_bytes(const plhip_conv_desc* d) {
  const int pwp = plhip::conv_patch_row_pitch(d->w, d->pad[2], d->pad[3]);
  const size_t b = (size_t)d->n * d->cin * (d->h + d->pad[0] + d->pad[1]) * pwp;
  return ((b + 15) & ~(size_t)15) + 4096;
}
// the phase-split copy of the stride-2 patch route: 4 phase planes per channel, rows of PW2p (a multiple of 8) bytes
static void patch_s2_dims(const plhip_conv_desc* d, int* ph2, int* pw2p) {
  *pw2p = plhip::conv_patch_s2_row_pitch(d->w, d->pad[2], d->pad[3]);
  *ph2 = (d->h + d->pad[0] + d->pad[1] + 1) >> 1;
}
static size_t patch_s2_input_bytes(const plhip_conv_desc* d) {
  int ph2, pw2p;
  patch_s2_dims(d, &ph2, &pw2p);
  const size_t b = (size_t)d->n * d->cin * 4 * ph2 * pw2p;
  return ((b + 15) & ~(size_t)15) + 4096;
}
static size_t padded_input_bytes(const plhip_conv_desc* d) {  // + slack: the last 16-byte pieces run past the last row
  int ph, pw;
  padded_dims(d, &ph, &pw);
  const size_t b = (size_t)d->n * d->cin * (d->stride[0] == 2 ? 4 : 1) * ph * pw;
  return ((b + 3) & ~(size_t)3) + 64;
}

bool conv_geom(const plhip_conv_desc* d, ConvGeom* g) {
  if (!d || d->n < 1 || d->cin < 1 || d->cout < 1 || d->h < 1 || d->w < 1 || d->kh < 1 || d->kw < 1) return false;
  if (d->groups < 1 || d->cin % d->groups || d->cout % d->groups) return false;
  if (d->stride[0] < 1 || d->stride[1] < 1 || d->dil[0] < 1 || d->dil[1] < 1) return false;
  for (int i = 0; i < 4; ++i)
    if (d->pad[i] < 0) return false;
  // conv_int8_compute_test.cc:67-88
  const int keh = d->dil[0] * (d->kh - 1) + 1, kew = d->dil[1] * (d->kw - 1) + 1;
  const int hn = d->h + d->pad[0] + d->pad[1] - keh, wn = d->w + d->pad[2] + d->pad[3] - kew;
  // C integer division (truncation), exactly as the reference computes it; a kernel extent larger than
  // the padded input is legal there as long as the quotient still yields >= 1 output.
  g->oh = hn / d->stride[0] + 1;
  g->ow = wn / d->stride[1] + 1;
  if (g->oh < 1 || g->ow < 1) return false;
  g->G = d->groups;
  g->Mg = d->cout / d->groups;
  g->Cg = d->cin / d->groups;
  g->Kg = g->Cg * d->kh * d->kw;
  g->N = g->oh * g->ow;
  g->Np = rup(g->N, 4);
  g->MA = g->Mg > 32 ? 2 : 1;
  g->MT = cdiv(g->Mg, 32 * g->MA);
  g->MT32 = g->MT * g->MA;
  g->KS = cdiv(g->Kg, 32);
  g->is_1x1_s1_p0 = d->kh == 1 && d->kw == 1 && d->stride[0] == 1 && d->stride[1] == 1 && d->pad[0] == 0 &&
                    d->pad[1] == 0 && d->pad[2] == 0 && d->pad[3] == 0;
  // impl selection (the analogue of conv_compute.cc:87-134): 1x1 -> GEMM straight on the NCHW slab; small-Cin 3x3 s2
  // stem -> direct (reference: DirectConv / conv3x3s2_direct_int8.cc); everything else im2col + GEMM (GemmLikeConv)
  if (g->is_1x1_s1_p0) g->impl = IMPL_GEMM_1X1;
  else if (plhip::conv3x3s2_direct_supported(d->cin, d->cout, d->kh, d->kw, d->stride[0], d->stride[1], d->dil[0], d->dil[1],
                                             d->groups, d->pad[2]))
    g->impl = IMPL_DIRECT_3X3S2;
  else if (plhip::conv7x7s2_stem_supported(d->cin, d->cout, d->kh, d->kw, d->stride[0], d->stride[1], d->dil[0], d->dil[1],
                                           d->groups, d->n, d->h, d->w, g->oh, g->ow, d->pad[2])) {
    g->impl = IMPL_STEM_7X7S2;  // ResNet50's stem: direct (conv_stem7_i8.hip), no padded copy
    return true;
  } else g->impl = IMPL_IM2COL_GEMM;
  // dense k x k stride-1 convs whose GEMM fits the LDS-DMA ring kernel (64-row wave tiles: M > 128, 32-row tiles: 96 < M <=
  // 128 with K >= 256) skip the im2col buffer: implicit GEMM on a zero-padded copy of the input (1.08x the input
  // instead of kh*kw x: BASELINE config #2 spent 128 of 149 us writing its 57.8 MB im2col buffer)
  const bool s1 = d->stride[0] == 1 && d->stride[1] == 1, s2 = d->stride[0] == 2 && d->stride[1] == 2;
  // dense 3x3 stride 1 with Cin % 32 == 0: the patch kernel (conv_patch_i8.hip): 3 shifted copies of the input rows per
  // 32-channel chunk in LDS instead of 9 K rows per channel
  if (g->impl == IMPL_IM2COL_GEMM &&
      plhip::conv_patch_supported(d->cin, d->cout, d->kh, d->kw, d->stride[0], d->stride[1], d->dil[0], d->dil[1], d->groups, d->w,
                                  d->pad[2], d->pad[3]) &&
      patch_input_bytes(d) < ((size_t)1 << 31) - 4096 && g->oh >= 1 &&
      // (global mode, planes smaller than a tile: a 16-byte output piece may end in the NEXT image, not beyond it)
      !(plhip::conv_patch_global(plhip::conv_patch_row_pitch(d->w, d->pad[2], d->pad[3])) && g->oh * g->ow < 16)) {
    g->impl = IMPL_PATCH_GEMM;
    return true;
  }
  // dense 3x3 stride 2 (ResNet50's downsampling convs): the same kernel as a 2x2 stride-1 conv over the 4 phase planes of
  // every channel (conv_patch_i8.hip)
  if (g->impl == IMPL_IM2COL_GEMM &&
      plhip::conv_patch_s2_supported(d->cin, d->cout, d->kh, d->kw, d->stride[0], d->stride[1], d->dil[0], d->dil[1], d->groups,
                                     d->w, d->pad[2], d->pad[3]) &&
      patch_s2_input_bytes(d) < ((size_t)1 << 31) - 4096 &&
      !(plhip::conv_patch_global(plhip::conv_patch_s2_row_pitch(d->w, d->pad[2], d->pad[3])) && g->oh * g->ow < 16)) {
    g->impl = IMPL_PATCH_S2;
    return true;
  }
  if (g->impl == IMPL_IM2COL_GEMM && d->groups == 1 && (s1 || s2) && d->dil[0] == 1 && d->dil[1] == 1 && d->kw <= 11 &&
      d->kh * d->kw <= 121 && !implicit_gemm_disabled()) {
    const size_t padded = padded_input_bytes(d);
    const bool fits = padded < ((size_t)1 << 31) - 4096 && (size_t)d->n * g->oh * rup(g->ow, 16) < ((size_t)1 << 31) - 1024;  // launch_gemm_tr's own bound (gemm_tr_i8.hip)
    if (plhip::gemm_tr_enabled()) {
      // transposed-read ring kernel: any M > 32, K >= 97, output rows down to 7 columns (one start-aligned 16-byte
      // chunk per row: the 14x14 and 7x7 planes of ResNet50's last stages), and stride 2 on a phase-split padded copy
      // (ResNet50's 7x7 stem and its three 3x3 downsampling convs); a 1x1 stride-2 conv would use one phase plane of
      // four: it keeps the (strided-copy) im2col route
      if (fits && g->Mg > 32 && g->KS >= 4 && g->ow >= 7 && !(s2 && d->kh * d->kw == 1)) g->impl = IMPL_IMPLICIT_GEMM;
    } else if (s1) {
      const int ma = (g->MA == 2 && g->Mg <= 128 && g->Mg > 64) ? 1 : g->MA;  // launch_gemm_i8's tile choice
      const int mt = cdiv(g->Mg, 32 * ma);
      if (fits && g->ow >= 16 && mt >= 4 && g->KS >= 4 && (ma == 2 || g->KS >= 8)) g->impl = IMPL_IMPLICIT_GEMM;
    }
  }
  return true;
}

inline bool aligned(const void* p, size_t a) { return ((uintptr_t)p & (a - 1)) == 0; }

}  // namespace

extern "C" {

int plhip_device_count(void) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) return 0;
  return n;
}

static plhip_status ctx_new(int device_id, hipStream_t stream, bool own, plhip_ctx** out) {
  if (!out) return fail(nullptr, PLHIP_ERR_INVALID, "null out pointer");
  int n = plhip_device_count();
  if (device_id < 0 || device_id >= n) return fail(nullptr, PLHIP_ERR_NO_DEVICE, "no HIP device %s", "with that id");
  HIPCHK(nullptr, hipSetDevice(device_id));
  hipDeviceProp_t prop;
  HIPCHK(nullptr, hipGetDeviceProperties(&prop, device_id));
  if (strncmp(prop.gcnArchName, "gfx950", 6) != 0)
    return fail(nullptr, PLHIP_ERR_NO_DEVICE, "device arch %s is not gfx950 (this library carries gfx950 code objects only)",
                prop.gcnArchName);
  plhip_ctx* c = new plhip_ctx;
  c->device = device_id;
  c->own_stream = own;
  c->err[0] = 0;
  if (own) {
    hipError_t e = hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking);
    if (e != hipSuccess) {
      delete c;
      return fail(nullptr, PLHIP_ERR_HIP, "hipStreamCreate failed: %s", hipGetErrorString(e));
    }
  } else {
    c->stream = stream;
  }
  *out = c;
  return PLHIP_OK;
}

plhip_status plhip_ctx_create(int device_id, plhip_ctx** out) { return ctx_new(device_id, nullptr, true, out); }

plhip_status plhip_ctx_create_on_stream(int device_id, void* hip_stream, plhip_ctx** out) {
  return ctx_new(device_id, (hipStream_t)hip_stream, false, out);
}

void plhip_ctx_destroy(plhip_ctx* ctx) {
  if (!ctx) return;
  for (auto& t : ctx->resize_tables) (void)hipFree(t.dev);
  if (ctx->own_stream) (void)hipStreamDestroy(ctx->stream);
  delete ctx;
}

void* plhip_ctx_stream(plhip_ctx* ctx) { return ctx ? (void*)ctx->stream : nullptr; }
const char* plhip_last_error(plhip_ctx* ctx) { return ctx ? ctx->err : g_err; }

plhip_status plhip_malloc(plhip_ctx* ctx, size_t bytes, void** dev_ptr) {
  if (!ctx || !dev_ptr) return fail(ctx, PLHIP_ERR_INVALID, "plhip_malloc: null argument");
  HIPCHK(ctx, hipSetDevice(ctx->device));
  HIPCHK(ctx, hipMalloc(dev_ptr, bytes ? bytes : 1));
  return PLHIP_OK;
}
plhip_status plhip_free(plhip_ctx* ctx, void* dev_ptr) {
  if (!ctx) return fail(ctx, PLHIP_ERR_INVALID, "plhip_free: null ctx");
  if (dev_ptr) HIPCHK(ctx, hipFree(dev_ptr));
  return PLHIP_OK;
}
plhip_status plhip_memcpy_h2d(plhip_ctx* ctx, void* dst, const void* src, size_t bytes) {
  if (!ctx) return fail(ctx, PLHIP_ERR_INVALID, "null ctx");
  if (bytes) HIPCHK(ctx, hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, ctx->stream));
  HIPCHK(ctx, hipStreamSynchronize(ctx->stream));  // pageable host memory: complete before returning
  return PLHIP_OK;
}
plhip_status plhip_memcpy_d2h(plhip_ctx* ctx, void* dst, const void* src, size_t bytes) {
  if (!ctx) return fail(ctx, PLHIP_ERR_INVALID, "null ctx");
  if (bytes) HIPCHK(ctx, hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
  return PLHIP_OK;
}
plhip_status plhip_memcpy_d2d(plhip_ctx* ctx, void* dst, const void* src, size_t bytes) {
  if (!ctx) return fail(ctx, PLHIP_ERR_INVALID, "null ctx");
  if (bytes) HIPCHK(ctx, hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToDevice, ctx->stream));
  return PLHIP_OK;
}
plhip_status plhip_memset(plhip_ctx* ctx, void* dst, int value, size_t bytes) {
  if (!ctx) return fail(ctx, PLHIP_ERR_INVALID, "null ctx");
  if (bytes) HIPCHK(ctx, hipMemsetAsync(dst, value, bytes, ctx->stream));
  return PLHIP_OK;
}
plhip_status plhip_stream_sync(plhip_ctx* ctx) {
  if (!ctx) return fail(ctx, PLHIP_ERR_INVALID, "null ctx");
  HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
  return PLHIP_OK;
}
plhip_status plhip_graph_begin(plhip_ctx* ctx) {
  if (!ctx) return fail(ctx, PLHIP_ERR_INVALID, "null ctx");
  HIPCHK(ctx, hipStreamBeginCapture(ctx->stream, hipStreamCaptureModeThreadLocal));
  return PLHIP_OK;
}
plhip_status plhip_graph_end(plhip_ctx* ctx, void** graph_exec) {
  if (!ctx || !graph_exec) return fail(ctx, PLHIP_ERR_INVALID, "null argument");
  hipGraph_t g = nullptr;
  HIPCHK(ctx, hipStreamEndCapture(ctx->stream, &g));
  hipGraphExec_t e = nullptr;
  const hipError_t st = hipGraphInstantiate(&e, g, nullptr, nullptr, 0);
  (void)hipGraphDestroy(g);
  if (st != hipSuccess) return fail(ctx, PLHIP_ERR_HIP, "hipGraphInstantiate failed: %s", hipGetErrorString(st));
  *graph_exec = (void*)e;
  return PLHIP_OK;
}
plhip_status plhip_graph_launch(plhip_ctx* ctx, void* graph_exec) {
  if (!ctx || !graph_exec) return fail(ctx, PLHIP_ERR_INVALID, "null argument");
  HIPCHK(ctx, hipGraphLaunch((hipGraphExec_t)graph_exec, ctx->stream));
  return PLHIP_OK;
}
plhip_status plhip_graph_destroy(plhip_ctx* ctx, void* graph_exec) {
  if (graph_exec) HIPCHK(ctx, hipGraphExecDestroy((hipGraphExec_t)graph_exec));
  return PLHIP_OK;
}
plhip_status plhip_event_create(plhip_ctx* ctx, void** event) {
  if (!ctx || !event) return fail(ctx, PLHIP_ERR_INVALID, "null argument");
  hipEvent_t e;
  HIPCHK(ctx, hipEventCreate(&e));
  *event = (void*)e;
  return PLHIP_OK;
}
plhip_status plhip_event_record(plhip_ctx* ctx, void* event) {
  if (!ctx || !event) return fail(ctx, PLHIP_ERR_INVALID, "null argument");
  HIPCHK(ctx, hipEventRecord((hipEvent_t)event, ctx->stream));
  return PLHIP_OK;
}
plhip_status plhip_event_elapsed_ms(plhip_ctx* ctx, void* start, void* stop, float* ms) {
  if (!ctx || !start || !stop || !ms) return fail(ctx, PLHIP_ERR_INVALID, "null argument");
  HIPCHK(ctx, hipEventSynchronize((hipEvent_t)stop));
  HIPCHK(ctx, hipEventElapsedTime(ms, (hipEvent_t)start, (hipEvent_t)stop));
  return PLHIP_OK;
}
plhip_status plhip_event_destroy(plhip_ctx* ctx, void* event) {
  if (event) HIPCHK(ctx, hipEventDestroy((hipEvent_t)event));
  return PLHIP_OK;
}

// ------------------------------------------------------------------ conv2d
size_t plhip_conv_packed_weight_bytes(const plhip_conv_desc* d) {
  ConvGeom g;
  if (!conv_geom(d, &g)) return 0;
  if (g.impl == IMPL_DIRECT_3X3S2) return plhip::conv3x3s2_direct_packed_bytes(d->cin, d->cout);
  if (g.impl == IMPL_PATCH_GEMM) return plhip::conv_patch_packed_bytes(d->cin, d->cout);
  if (g.impl == IMPL_PATCH_S2) return plhip::conv_patch_s2_packed_bytes(d->cin, d->cout);
  if (g.impl == IMPL_STEM_7X7S2) return plhip::conv7x7s2_stem_packed_bytes(d->cout);
  return (size_t)g.G * g.MT32 * g.KS * 1024;
}

plhip_status plhip_pack_conv_weights(plhip_ctx* ctx, const plhip_conv_desc* d, const int8_t* w_oihw, void* w_packed) {
  ConvGeom g;
  if (!ctx || !w_oihw || !w_packed) return fail(ctx, PLHIP_ERR_INVALID, "plhip_pack_conv_weights: null argument");
  if (!conv_geom(d, &g)) return fail(ctx, PLHIP_ERR_INVALID, "plhip_pack_conv_weights: bad conv descriptor");
  if (g.impl == IMPL_DIRECT_3X3S2) {
    if (!aligned(w_packed, 4)) return fail(ctx, PLHIP_ERR_INVALID, "plhip_pack_conv_weights: packed buffer must be 4-byte aligned");
    plhip::launch_pack_conv3x3s2_direct(w_oihw, (uint32_t*)w_packed, d->cin, d->cout, ctx->stream);
  } else if (g.impl == IMPL_PATCH_GEMM) {
    plhip::launch_pack_conv_patch(w_oihw, (int8_t*)w_packed, d->cin, d->cout, ctx->stream);
  } else if (g.impl == IMPL_PATCH_S2) {
    plhip::launch_pack_conv_patch_s2(w_oihw, (int8_t*)w_packed, d->cin, d->cout, ctx->stream);
  } else if (g.impl == IMPL_STEM_7X7S2) {
    plhip::launch_pack_conv7x7s2_stem(w_oihw, (int8_t*)w_packed, d->cin, d->cout, ctx->stream);
  } else {
    plhip::launch_pack_weights(w_oihw, (int8_t*)w_packed, g.G, g.Mg, g.Kg, g.MT32, g.KS, ctx->stream);
  }
  LAUNCHCHK(ctx, "pack_weights");
  return PLHIP_OK;
}

size_t plhip_conv_workspace_bytes(const plhip_conv_desc* d) {
  ConvGeom g;
  if (!conv_geom(d, &g)) return 0;
  if (g.impl == IMPL_IMPLICIT_GEMM) return padded_input_bytes(d);
  if (g.impl == IMPL_PATCH_GEMM) return patch_input_bytes(d);
  if (g.impl == IMPL_PATCH_S2) return patch_s2_input_bytes(d);
  if (g.impl != IMPL_IM2COL_GEMM) return 0;
  return (size_t)d->n * g.G * g.Kg * g.Np;
}

const char* plhip_conv_impl_name(const plhip_conv_desc* d) {
  ConvGeom g;
  if (!conv_geom(d, &g)) return "invalid";
  if (g.impl == IMPL_GEMM_1X1) return "conv1x1s1_gemm_int8_mfma32x32x32";
  if (g.impl == IMPL_DIRECT_3X3S2)  // one MFMA K-step when the taps fit (Cin <= 3, OW % 4 == 0), v_dot4 otherwise
    return (d->cin * 3 <= 9 && (g.ow & 3) == 0) ? "conv_3x3s2_direct_int8_mfma32x32x32" : "conv_3x3s2_direct_int8_dot4";
  if (g.impl == IMPL_IMPLICIT_GEMM) return "conv_implicit_gemm_int8_mfma32x32x32";
  if (g.impl == IMPL_PATCH_GEMM) return "conv_patch_gemm_int8_mfma32x32x32";
  if (g.impl == IMPL_PATCH_S2) return "conv_patch_s2_gemm_int8_mfma32x32x32";
  if (g.impl == IMPL_STEM_7X7S2) return "conv_7x7s2_direct_int8_mfma32x32x32";
  return "conv_im2col_gemm_int8_mfma32x32x32";
}

// The output-kind / scale / activation checks of a compute entry point, in this order, `who` = its name in the texts.
// gap_ok: PLHIP_OUT_F32_GAP is one of its kinds; scale_name: what it calls the scale; act: nullptr = no activation enum to check
static plhip_status check_out_scale_act(plhip_ctx* ctx, const char* who, plhip_out_kind out, bool gap_ok, const float* scale,
                                        const char* scale_name, const int* act, const char* act_name = "activation") {
  if (out != PLHIP_OUT_I32_ACC && out != PLHIP_OUT_F32 && out != PLHIP_OUT_I8 && !(gap_ok && out == PLHIP_OUT_F32_GAP))
    return fail(ctx, PLHIP_ERR_INVALID, "%s: bad out kind", who);
  if (out != PLHIP_OUT_I32_ACC && !scale) return fail(ctx, PLHIP_ERR_INVALID, "%s: %s required", who, scale_name);
  if (act && *act != PLHIP_ACT_NONE && *act != PLHIP_ACT_RELU && *act != PLHIP_ACT_RELU6 && *act != PLHIP_ACT_LEAKY_RELU)
    return fail(ctx, PLHIP_ERR_UNSUPPORTED, "%s: unsupported %s", who, act_name);
  return PLHIP_OK;
}

// the shape half of a stem kernel's arguments; the pointers and the fused front / tail are the caller's
static plhip::DirectS2Args direct_s2_args(const plhip_conv_desc* d, const ConvGeom& g) {
  plhip::DirectS2Args a = plhip::DirectS2Args();
  a.n = d->n; a.cin = d->cin; a.h = d->h; a.w = d->w; a.cout = d->cout; a.coutp = rup(d->cout, 4);
  a.oh = g.oh; a.ow = g.ow; a.pt = d->pad[0]; a.pl = d->pad[2]; a.act = d->act; a.alpha = d->act_alpha;
  return a;
}

struct ConvTail {  // fused graph tail of an fp32-output conv (plhip_conv2d_int8_fused)
  const float* residual;
  int residual_relu;
  int8_t* y_i8;
  float calib_scale;
};

static plhip_status conv2d_impl(plhip_ctx* ctx, const plhip_conv_desc* d, const int8_t* x, const void* w_packed,
                                const float* scale, const float* bias, void* y, plhip_out_kind out, void* workspace,
                                size_t workspace_bytes, const ConvTail* tail) {
  ConvGeom g;
  const bool y_opt = tail && tail->y_i8;  // the fp32 tensor itself may be dropped when only the int8 copy is consumed
  if (!ctx || !x || !w_packed || (!y && !y_opt)) return fail(ctx, PLHIP_ERR_INVALID, "plhip_conv2d_int8: null argument");
  if (!conv_geom(d, &g)) return fail(ctx, PLHIP_ERR_INVALID, "plhip_conv2d_int8: bad conv descriptor");
  if (plhip_status st = check_out_scale_act(ctx, "plhip_conv2d_int8", out, false, scale, "scale", &d->act)) return st;
  if ((size_t)d->n * g.Np >= ((size_t)1 << 31) - 256 || (size_t)d->cin * d->h * d->w >= ((size_t)1 << 31) ||
      (size_t)d->cout * g.N >= ((size_t)1 << 31))
    return fail(ctx, PLHIP_ERR_UNSUPPORTED, "plhip_conv2d_int8: tensor too large for 32-bit column index");

  const float* t_res = tail ? tail->residual : nullptr;
  const int t_relu = tail ? tail->residual_relu : 0;
  int8_t* t_y2 = tail ? tail->y_i8 : nullptr;
  const float t_inv = (tail && tail->y_i8) ? 1.f / tail->calib_scale : 0.f;  // type_trans.cc:45
  const bool has_tail = t_res || t_y2;
  if (g.impl == IMPL_DIRECT_3X3S2) {
    if (has_tail) return fail(ctx, PLHIP_ERR_UNSUPPORTED, "plhip_conv2d_int8_fused: the direct 3x3 s2 stem has no fused tail");
    plhip::DirectS2Args a = direct_s2_args(d, g);
    a.x = x;
    a.wp = (const uint32_t*)w_packed;
    a.y = y;
    a.scale = scale;
    a.bias = bias;
    plhip::launch_conv3x3s2_direct(a, (int)out, ctx->stream);
    LAUNCHCHK(ctx, "conv3x3s2_direct");
    return PLHIP_OK;
  }
  if (g.impl == IMPL_STEM_7X7S2) {
    if (!aligned(w_packed, 16)) return fail(ctx, PLHIP_ERR_INVALID, "plhip_conv2d_int8: packed weights must be 16-byte aligned");
    plhip::DirectS2Args a = direct_s2_args(d, g);
    a.x = x;
    a.wp = (const uint32_t*)w_packed;
    a.y = y;
    a.scale = scale;
    a.bias = bias;
    a.res = t_res; a.res_relu = t_relu; a.y2 = t_y2; a.inv_scale2 = t_inv;
    const size_t esz_s = out == PLHIP_OUT_I8 ? 1 : 4;
    const bool vec = aligned(y, 4 * esz_s) && aligned(t_res, 16) && aligned(t_y2, 4);
    plhip::launch_conv7x7s2_stem(a, (int)out, vec, ctx->stream);
    LAUNCHCHK(ctx, "conv7x7s2_stem");
    return PLHIP_OK;
  }
  if (g.impl == IMPL_PATCH_GEMM || g.impl == IMPL_PATCH_S2) {
    const bool s2 = g.impl == IMPL_PATCH_S2;
    const size_t need = s2 ? patch_s2_input_bytes(d) : patch_input_bytes(d);
    if (!workspace || workspace_bytes < need || !aligned(workspace, 16))
      return fail(ctx, PLHIP_ERR_WORKSPACE, "plhip_conv2d_int8: padded-input workspace missing, too small or unaligned (16 bytes)");
    int PWp = plhip::conv_patch_row_pitch(d->w, d->pad[2], d->pad[3]), PH = d->h + d->pad[0] + d->pad[1];
    if (s2) patch_s2_dims(d, &PH, &PWp);
    const int CE = s2 ? 4 * d->cin : d->cin;  // the kernel's channels: stride 2 = (channel, row phase, column phase)
    plhip::PadArgs pa;
    pa.stride = d->stride[0];
    pa.x = x;
    pa.xp = (int8_t*)workspace;
    pa.planes = d->n * CE;
    pa.h = d->h; pa.w = d->w; pa.ph = PH; pa.pw = PWp; pa.pt = d->pad[0]; pa.pl = d->pad[2];
    pa.total = (long)need;
    pa.tb = plhip::conv_patch_global(PWp) ? d->n : 0;  // planes smaller than a tile: channel-major copy
    pa.tc = CE;
    if (s2) plhip::launch_pad_phase8(pa, ctx->stream);
    else plhip::launch_pad_rows8(pa, ctx->stream);
    LAUNCHCHK(ctx, "pad_rows8");
    plhip::PatchArgs a;
    memset(&a, 0, sizeof(a));
    a.xp = (const int8_t*)workspace;
    a.wp = (const int8_t*)w_packed;
    a.y = y;
    a.scale = scale;
    a.bias = bias;
    a.B = d->n; a.C = CE; a.M = d->cout; a.OH = g.oh; a.OW = g.ow;
    a.PWp = PWp;
    a.PLANE = PH * PWp;
    a.s2 = s2 ? 1 : 0;
    a.act = d->act;
    a.alpha = d->act_alpha;
    a.res = t_res; a.res_relu = t_relu; a.y2 = t_y2; a.inv_scale2 = t_inv;
    plhip::launch_conv_patch(a, (int)out, ctx->stream);
    LAUNCHCHK(ctx, "conv_patch");
    return PLHIP_OK;
  }
  if (g.impl == IMPL_IMPLICIT_GEMM) {
    const size_t need = padded_input_bytes(d);
    if (!workspace || workspace_bytes < need || !aligned(workspace, 4))
      return fail(ctx, PLHIP_ERR_WORKSPACE, "plhip_conv2d_int8: padded-input workspace missing, too small or unaligned");
    int PH, PW;
    padded_dims(d, &PH, &PW);
    plhip::PadArgs pa;
    pa.stride = d->stride[0];
    pa.x = x;
    pa.xp = (int8_t*)workspace;
    pa.planes = d->n * d->cin;
    pa.h = d->h; pa.w = d->w; pa.ph = PH; pa.pw = PW; pa.pt = d->pad[0]; pa.pl = d->pad[2];
    pa.total = (long)need;
    plhip::launch_pad_input(pa, ctx->stream);
    LAUNCHCHK(ctx, "pad_input");
    const size_t esz_i = out == PLHIP_OUT_I8 ? 1 : 4;
    plhip::GemmArgs a;
    a.wp = (const int8_t*)w_packed;
    a.x = (const int8_t*)workspace;
    a.y = y;
    a.scale = scale;
    a.bias = bias;
    a.M = g.Mg;
    a.K = g.Kg;
    a.KS = g.KS;
    a.HWX = g.ow;          // an "image" of the column space is one output row
    a.HWY = g.N;
    a.XP = 0;
    a.x_bytes = (long)need;
    a.NB = d->n * g.oh;
    a.x_bstride = 0;
    a.y_bstride = (size_t)d->cout * g.N;
    a.MT = g.MT;
    a.NT = 0;              // set by the launcher from NB and HWX
    a.act = d->act;
    a.alpha = d->act_alpha;
    a.im_kw = d->kw; a.im_khkw = d->kh * d->kw; a.im_c = d->cin; a.im_ph = PH; a.im_pw = PW; a.im_oh = g.oh;
    a.im_s = d->stride[0];
    a.res = t_res; a.res_relu = t_relu; a.y2 = t_y2; a.inv_scale2 = t_inv;
    const bool vec_store_i = (g.ow & 3) == 0 && aligned(y, 4 * esz_i) && aligned(t_res, 16) && aligned(t_y2, 4);
    if (plhip::launch_gemm_i8(a, g.MA, (int)out, vec_store_i, true, ctx->stream) != 0)
      return fail(ctx, PLHIP_ERR_UNSUPPORTED, "conv2d: implicit GEMM outside the transposed-read kernel's column space");
    LAUNCHCHK(ctx, "gemm_i8_implicit");
    return PLHIP_OK;
  }
  const bool direct = g.impl == IMPL_GEMM_1X1;
  const int8_t* bmat = x;
  size_t x_bstride = (size_t)d->cin * g.N, x_gstride = (size_t)g.Cg * g.N;
  int hwx = g.Np, xp = g.N;
  long x_bytes = (long)d->n * d->cin * g.N;
  bool aligned_loads = (g.N & 3) == 0 && aligned(x, 4);
  if (!direct) {
    const size_t need = (size_t)d->n * g.G * g.Kg * g.Np;
    if (!workspace || workspace_bytes < need || !aligned(workspace, 4))
      return fail(ctx, PLHIP_ERR_WORKSPACE, "plhip_conv2d_int8: im2col workspace missing, too small or unaligned");
    plhip::Im2colArgs ia;
    ia.x = x;
    ia.col = (int8_t*)workspace;
    ia.cin = d->cin;
    ia.cin_g = g.Cg;
    ia.h = d->h;
    ia.w = d->w;
    ia.kh = d->kh;
    ia.kw = d->kw;
    ia.pt = d->pad[0];
    ia.pl = d->pad[2];
    ia.sh = d->stride[0];
    ia.sw = d->stride[1];
    ia.dh = d->dil[0];
    ia.dw = d->dil[1];
    ia.oh = g.oh;
    ia.ow = g.ow;
    ia.G = g.G;
    ia.Kg = g.Kg;
    ia.N = g.N;
    ia.Np = g.Np;
    ia.rows = (size_t)d->n * g.G * g.Kg;
    if (g.Kg > 65535 || (size_t)d->n * g.G > 65535)
      return fail(ctx, PLHIP_ERR_UNSUPPORTED, "plhip_conv2d_int8: im2col route needs Kg and batch*groups <= 65535");
    plhip::launch_im2col(ia, ctx->stream);
    LAUNCHCHK(ctx, "im2col");
    bmat = (const int8_t*)workspace;
    x_bstride = (size_t)g.G * g.Kg * g.Np;
    x_gstride = (size_t)g.Kg * g.Np;
    xp = g.Np;
    x_bytes = (long)need;
    aligned_loads = true;
  }
  const size_t esz = out == PLHIP_OUT_I8 ? 1 : 4;
  const bool vec_store = hwx == g.N && aligned(y, 4 * esz) && aligned(t_res, 16) && aligned(t_y2, 4);
  for (int grp = 0; grp < g.G; ++grp) {
    plhip::GemmArgs a;
    a.wp = (const int8_t*)w_packed + (size_t)grp * g.MT32 * g.KS * 1024;
    a.x = bmat + (size_t)grp * x_gstride;
    a.y = y ? (char*)y + (size_t)grp * g.Mg * g.N * esz : nullptr;
    a.res = t_res ? t_res + (size_t)grp * g.Mg * g.N : nullptr;
    a.res_relu = t_relu;
    a.y2 = t_y2 ? t_y2 + (size_t)grp * g.Mg * g.N : nullptr;
    a.inv_scale2 = t_inv;
    a.scale = scale ? scale + (size_t)grp * g.Mg : nullptr;
    a.bias = bias ? bias + (size_t)grp * g.Mg : nullptr;
    a.M = g.Mg;
    a.K = g.Kg;
    a.KS = g.KS;
    a.HWX = hwx;
    a.HWY = g.N;
    a.XP = xp;
    a.x_bytes = x_bytes - (long)grp * (long)x_gstride;
    a.NB = d->n;
    a.x_bstride = x_bstride;
    a.y_bstride = (size_t)d->cout * g.N;
    a.MT = g.MT;
    a.NT = cdiv(d->n * hwx, 128);
    a.act = d->act;
    a.alpha = d->act_alpha;
    a.im_kw = a.im_khkw = a.im_c = a.im_ph = a.im_pw = a.im_oh = 0;
    a.im_s = 1;
    if (plhip::launch_gemm_i8(a, g.MA, (int)out, vec_store, aligned_loads, ctx->stream) != 0)
      return fail(ctx, PLHIP_ERR_UNSUPPORTED, "conv2d: GEMM shape outside every kernel");
    LAUNCHCHK(ctx, "gemm_i8");
  }
  return PLHIP_OK;
}

plhip_status plhip_conv2d_int8(plhip_ctx* ctx, const plhip_conv_desc* d, const int8_t* x, const void* w_packed,
                               const float* scale, const float* bias, void* y, plhip_out_kind out, void* workspace,
                               size_t workspace_bytes) {
  return conv2d_impl(ctx, d, x, w_packed, scale, bias, y, out, workspace, workspace_bytes, nullptr);
}

plhip_status plhip_conv2d_int8_fused(plhip_ctx* ctx, const plhip_conv_desc* d, const int8_t* x, const void* w_packed,
                                     const float* scale, const float* bias, float* y_f32, const float* residual,
                                     int residual_relu, int8_t* y_i8, float calib_scale, void* workspace,
                                     size_t workspace_bytes) {
  if (!y_f32 && !y_i8) return fail(ctx, PLHIP_ERR_INVALID, "plhip_conv2d_int8_fused: no output");
  if (y_i8 && !(calib_scale > 0.f)) return fail(ctx, PLHIP_ERR_INVALID, "plhip_conv2d_int8_fused: calib scale must be > 0");
  if (residual_relu && !residual) return fail(ctx, PLHIP_ERR_INVALID, "plhip_conv2d_int8_fused: residual_relu without a residual");
  ConvTail t{residual, residual_relu, y_i8, calib_scale};
  return conv2d_impl(ctx, d, x, w_packed, scale, bias, y_f32, PLHIP_OUT_F32, workspace, workspace_bytes, &t);
}

// ------------------------------------------------------------------ calib[fp32_to_int8] + conv in one launch
static bool calib_conv_args(const plhip_conv_desc* d, plhip::DirectS2Args* a) {
  ConvGeom g;
  if (!d || !conv_geom(d, &g) || g.impl != IMPL_DIRECT_3X3S2) return false;
  *a = direct_s2_args(d, g);
  return plhip::conv3x3s2_f32in_supported(*a);
}

// The calib and image stems behind their envelope checks.  false: a pointer is misaligned (in: in_align bytes, w_packed: 16, y: 4
// elements); else a's pointers and quantiser are set and *afrag = the MFMA A fragments inside the packed block.
static bool fused_stem_tail(plhip::DirectS2Args* a, const void* in, size_t in_align, float calib_scale, const void* w_packed,
                            const float* scale, const float* bias, void* y, plhip_out_kind out, const int8_t** afrag) {
  const size_t esz = out == PLHIP_OUT_I8 ? 1 : 4;
  if (!aligned(in, in_align) || !aligned(y, 4 * esz) || !aligned(w_packed, 16)) return false;
  a->x_inv_scale = 1.f / calib_scale;  // type_trans.cc:45
  a->wp = (const uint32_t*)w_packed;
  a->y = y;
  a->scale = scale;
  a->bias = bias;
  *afrag = reinterpret_cast<const int8_t*>(w_packed) + plhip::conv3x3s2_dot4_bytes(a->cin, a->cout);
  return true;
}

int plhip_conv2d_calib_supported(const plhip_conv_desc* d) {
  plhip::DirectS2Args a;
  return calib_conv_args(d, &a) ? 1 : 0;
}

plhip_status plhip_conv2d_calib_int8(plhip_ctx* ctx, const plhip_conv_desc* d, const float* x_f32, float calib_scale,
                                     const void* w_packed, const float* scale, const float* bias, void* y, plhip_out_kind out) {
  if (!ctx || !x_f32 || !w_packed || !y || !(calib_scale > 0.f)) return fail(ctx, PLHIP_ERR_INVALID, "plhip_conv2d_calib_int8: null / bad argument");
  if (plhip_status st = check_out_scale_act(ctx, "plhip_conv2d_calib_int8", out, false, scale, "scale", d ? &d->act : nullptr)) return st;
  plhip::DirectS2Args a;
  if (!calib_conv_args(d, &a)) return fail(ctx, PLHIP_ERR_UNSUPPORTED, "plhip_conv2d_calib_int8: shape outside the fused stem");
  const int8_t* afrag;
  if (!fused_stem_tail(&a, x_f32, 16, calib_scale, w_packed, scale, bias, y, out, &afrag))
    return fail(ctx, PLHIP_ERR_INVALID, "plhip_conv2d_calib_int8: x / w_packed must be 16-byte aligned, y 4 elements");
  a.xf = x_f32;
  plhip::launch_conv3x3s2_f32in(a, afrag, (int)out, ctx->stream);
  LAUNCHCHK(ctx, "conv3x3s2_f32in");
  return PLHIP_OK;
}

// ------------------------------------------------------------------ uint8 image input
// ImagePreprocess::image_to_tensor (paddle_image_preprocess.cc:143-172 -> Image2Tensor::choose, image2tensor.cc:85-128): which
// formats exist and how many bytes a pixel has / how many channels come out
static bool image_args(const plhip_image_desc* img, const uint8_t* src, plhip::ImageArgs* a) {
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

int plhip_conv2d_image_supported(const plhip_conv_desc* d, const plhip_image_desc* img) {
  plhip::DirectS2Args a;
  plhip::ImageArgs im;
  return calib_conv_args(d, &a) && image_args(img, nullptr, &im) && plhip::conv3x3s2_u8in_supported(a, im) ? 1 : 0;
}

plhip_status plhip_conv2d_image_int8(plhip_ctx* ctx, const plhip_conv_desc* d, const plhip_image_desc* img, const uint8_t* src,
                                     float calib_scale, const void* w_packed, const float* scale, const float* bias, void* y,
                                     plhip_out_kind out) {
  if (!ctx || !src || !w_packed || !y || !(calib_scale > 0.f)) return fail(ctx, PLHIP_ERR_INVALID, "plhip_conv2d_image_int8: null / bad argument");
  if (plhip_status st = check_out_scale_act(ctx, "plhip_conv2d_image_int8", out, false, scale, "scale", d ? &d->act : nullptr)) return st;
  plhip::DirectS2Args a;
  plhip::ImageArgs im;
  if (!image_args(img, src, &im)) return fail(ctx, PLHIP_ERR_INVALID, "plhip_conv2d_image_int8: bad image descriptor");
  if (!calib_conv_args(d, &a) || !plhip::conv3x3s2_u8in_supported(a, im))
    return fail(ctx, PLHIP_ERR_UNSUPPORTED, "plhip_conv2d_image_int8: shape outside the fused stem");
  const int8_t* afrag;
  if (!fused_stem_tail(&a, src, 4, calib_scale, w_packed, scale, bias, y, out, &afrag))
    return fail(ctx, PLHIP_ERR_INVALID, "plhip_conv2d_image_int8: src must be 4-byte aligned, w_packed 16, y 4 elements");
  plhip::launch_conv3x3s2_u8in(a, im, afrag, (int)out, ctx->stream);
  LAUNCHCHK(ctx, "conv3x3s2_u8in");
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

// ------------------------------------------------------------------ depthwise
plhip_status plhip_depthwise_conv_int8(plhip_ctx* ctx, const plhip_conv_desc* d, const int8_t* x, const int8_t* w_oihw,
                                       const float* scale, const float* bias, void* y, plhip_out_kind out) {
  ConvGeom g;
  if (!ctx || !x || !w_oihw || !y) return fail(ctx, PLHIP_ERR_INVALID, "plhip_depthwise_conv_int8: null argument");
  if (!conv_geom(d, &g)) return fail(ctx, PLHIP_ERR_INVALID, "plhip_depthwise_conv_int8: bad conv descriptor");
  if (d->groups != d->cin || d->cin != d->cout)
    return fail(ctx, PLHIP_ERR_UNSUPPORTED, "plhip_depthwise_conv_int8: needs groups == cin == cout");
  if (plhip_status st = check_out_scale_act(ctx, "plhip_depthwise_conv_int8", out, false, scale, "scale", &d->act)) return st;
  const size_t esz = out == PLHIP_OUT_I8 ? 1 : 4;
  if (!aligned(y, 4 * esz) && (g.ow & 3) == 0)
    return fail(ctx, PLHIP_ERR_UNSUPPORTED, "plhip_depthwise_conv_int8: output pointer must be 4-element aligned");

  plhip::DwArgs a;
  a.x = x;
  a.wt = w_oihw;
  a.y = y;
  a.scale = scale;
  a.bias = bias;
  a.planes = d->n * d->cin;
  a.C = d->cin;
  a.h = d->h;
  a.w = d->w;
  a.oh = g.oh;
  a.ow = g.ow;
  a.kh = d->kh;
  a.kw = d->kw;
  a.pt = d->pad[0];
  a.pl = d->pad[2];
  a.sh = d->stride[0];
  a.sw = d->stride[1];
  a.dh = d->dil[0];
  a.dw = d->dil[1];
  a.act = d->act;
  a.alpha = d->act_alpha;
  // Tiling: a block covers PB planes x OB output rows; aim at ~2K quads (8 per thread) per block and keep
  // the LDS tile under 48 KiB so that several blocks share a CU.
  const int owq = cdiv(g.ow, 4);
  const int OFF = rup(d->pad[2], 4);
  const int maxcol = (4 * owq - 1) * d->stride[1] - d->pad[2] + (d->kw - 1) * d->dil[1] + OFF;
  int pitch = rup((maxcol > OFF + d->w ? maxcol : OFF + d->w) + 1 + 16, 4);
  const int target = 2048;
  int OB, PB;
  if (g.oh * owq >= target) {
    PB = 1;
    OB = target / owq;
    if (OB < 1) OB = 1;
    if (OB > g.oh) OB = g.oh;
  } else {
    OB = g.oh;
    PB = target / (g.oh * owq);
    if (PB < 1) PB = 1;
    if (PB > 64) PB = 64;
    if (PB > a.planes) PB = a.planes;
  }
  auto in_rows_of = [&](int ob) { return (ob - 1) * d->stride[0] + (d->kh - 1) * d->dil[0] + 1; };
  auto lds_of = [&](int pb, int ob) {
    return (size_t)pb * in_rows_of(ob) * pitch + (size_t)pb * d->kh * 8 + (size_t)pb * 8 + (size_t)pb * d->kh * d->kw + 16;
  };
  while (lds_of(PB, OB) > 48 * 1024 && PB > 1) PB = PB / 2;
  while (lds_of(PB, OB) > 48 * 1024 && OB > 1) OB = (OB + 1) / 2;
  if (lds_of(PB, OB) > 60 * 1024)
    return fail(ctx, PLHIP_ERR_UNSUPPORTED, "plhip_depthwise_conv_int8: a single row band does not fit in LDS");
  a.PB = PB;
  a.OB = OB;
  a.bands = cdiv(g.oh, OB);
  a.in_rows = in_rows_of(OB);
  a.pitch = pitch;
  if (plhip::launch_depthwise(a, (int)out, ctx->stream) != 0)
    return fail(ctx, PLHIP_ERR_UNSUPPORTED, "plhip_depthwise_conv_int8: LDS tile too large");
  LAUNCHCHK(ctx, "depthwise_i8");
  return PLHIP_OK;
}

// ------------------------------------------------------------------ fused depthwise -> pointwise
// geometry + launch plan of the fused pair; false: not a depthwise 3x3 the fused kernel takes (the caller runs two kernels)
static bool dwpw_plan(const plhip_conv_desc* dw, int pw_cout, plhip_out_kind out, plhip::FusedArgs* a, const char** why) {
  ConvGeom g;
  *why = "bad depthwise descriptor";
  if (!dw || pw_cout < 1 || !conv_geom(dw, &g)) return false;
  *why = "first conv must be depthwise";
  if (dw->groups != dw->cin || dw->cin != dw->cout) return false;
  *why = "tensor too large";
  if ((size_t)pw_cout * g.N >= ((size_t)1 << 31) || (size_t)dw->cin * dw->h * dw->w >= ((size_t)1 << 31)) return false;
  memset(a, 0, sizeof(*a));
  a->dw_act = dw->act;
  a->dw_alpha = dw->act_alpha;
  a->n = dw->n; a->C = dw->cin; a->h = dw->h; a->w = dw->w; a->oh = g.oh; a->ow = g.ow;
  a->pt = dw->pad[0]; a->pl = dw->pad[2]; a->stride = dw->stride[0];
  a->pw.M = pw_cout;
  a->pw.K = dw->cin;
  a->pw.KS = cdiv(dw->cin, 32);
  a->pw.HWY = g.N;
  a->pw.y_bstride = (size_t)pw_cout * g.N;
  *why = "shape outside the fused path";
  return plhip::fused_dwpw_plan(a, dw->kh, dw->kw, dw->stride[0], dw->stride[1], dw->dil[0], dw->dil[1], (int)out);
}

int plhip_dwpw_fused_supported(const plhip_conv_desc* dw, int pw_cout, plhip_out_kind out) {
  plhip::FusedArgs a;
  const char* why;
  return dwpw_plan(dw, pw_cout, out, &a, &why) ? 1 : 0;
}

plhip_status plhip_dwpw_fused_int8(plhip_ctx* ctx, const plhip_conv_desc* dw, const int8_t* x, const int8_t* dw_w_oihw,
                                   const float* dw_scale, const float* dw_bias, int pw_cout, const void* pw_w_packed,
                                   const float* pw_scale, const float* pw_bias, int pw_act, float pw_alpha, void* y,
                                   plhip_out_kind out) {
  if (!ctx || !dw || !x || !dw_w_oihw || !dw_scale || !pw_w_packed || !y || pw_cout < 1)
    return fail(ctx, PLHIP_ERR_INVALID, "plhip_dwpw_fused_int8: null / bad argument");
  if (plhip_status st = check_out_scale_act(ctx, "plhip_dwpw_fused_int8", out, true, pw_scale, "pw_scale", nullptr)) return st;
  plhip::FusedArgs a;
  const char* why;
  if (!dwpw_plan(dw, pw_cout, out, &a, &why)) {
    return fail(ctx, PLHIP_ERR_UNSUPPORTED, "plhip_dwpw_fused_int8: %s", why);
  }
  a.x = x;
  a.dw_w = dw_w_oihw;
  a.dw_scale = dw_scale;
  a.dw_bias = dw_bias;
  a.pw.wp = (const int8_t*)pw_w_packed;
  a.pw.y = y;
  a.pw.scale = pw_scale;
  a.pw.bias = pw_bias;
  a.pw.act = pw_act;
  a.pw.alpha = pw_alpha;
  plhip::launch_fused_dwpw(a, (int)out, ctx->stream);
  LAUNCHCHK(ctx, "fused_dwpw");
  return PLHIP_OK;
}

// ------------------------------------------------------------------ fused depthwise -> 1x1 conv with the conv's tail (fusion G)
// geometry + launch plan; false: outside the kernel's envelope (the caller runs the two instructions).  Host logic only.
static bool dw_conv1x1_plan(const plhip_conv_desc* dw, int pw_cout, plhip_out_kind out, int has_tail, plhip::DwConvArgs* a,
                            const char** why) {
  ConvGeom g;
  *why = "bad depthwise descriptor";
  if (!dw || !conv_geom(dw, &g)) return false;
  *why = "output kind";
  if (out != PLHIP_OUT_I32_ACC && out != PLHIP_OUT_F32 && out != PLHIP_OUT_I8) return false;
  *why = "a graph tail needs fp32 output";
  if (has_tail && out != PLHIP_OUT_F32) return false;
  *why = "first conv must be a 3x3 depthwise conv, channel multiplier 1, dilation 1, stride 1 | 2, paddings 0 | 1";
  if (dw->groups != dw->cin || dw->cin != dw->cout || dw->kh != 3 || dw->kw != 3 || dw->dil[0] != 1 || dw->dil[1] != 1 ||
      dw->stride[0] != dw->stride[1] || (dw->stride[0] != 1 && dw->stride[0] != 2))
    return false;
  for (int i = 0; i < 4; ++i)
    if (dw->pad[i] != 0 && dw->pad[i] != 1) return false;
  *why = "unsupported depthwise activation";
  if (dw->act != PLHIP_ACT_NONE && dw->act != PLHIP_ACT_RELU && dw->act != PLHIP_ACT_RELU6 && dw->act != PLHIP_ACT_LEAKY_RELU)
    return false;
  memset(a, 0, sizeof(*a));
  a->dw_act = dw->act;
  a->dw_alpha = dw->act_alpha;
  a->n = dw->n; a->C = dw->cin; a->h = dw->h; a->w = dw->w; a->oh = g.oh; a->ow = g.ow;
  a->pt = dw->pad[0]; a->pl = dw->pad[2]; a->stride = dw->stride[0];
  a->M = pw_cout;
  *why = "fused depthwise -> 1x1 kernel switched off (diagnostics knob DWCONV_FUSED = 0)";
  if (!plhip::knob("DWCONV_FUSED", 1)) return false;
  *why = "shape outside the fused kernel (C % 16, C <= 1024, M % 8, M <= 1024, 32-bit element offsets)";
  return plhip::dw_conv1x1_plan(a);
}

int plhip_dw_conv1x1_fused_supported(const plhip_conv_desc* dw, int pw_cout, plhip_out_kind out, int has_tail) {
  plhip::DwConvArgs a;
  const char* why;
  return dw_conv1x1_plan(dw, pw_cout, out, has_tail, &a, &why) ? 1 : 0;
}

plhip_status plhip_dw_conv1x1_fused_int8(plhip_ctx* ctx, const plhip_conv_desc* dw, const int8_t* x, const int8_t* dw_w_oihw,
                                         const float* dw_scale, const float* dw_bias, int pw_cout, const void* pw_w_packed,
                                         const float* pw_scale, const float* pw_bias, int pw_act, float pw_alpha, void* y,
                                         plhip_out_kind out, const float* residual, int residual_relu, int8_t* y_i8,
                                         float calib_scale) {
  const int has_tail = residual || y_i8;
  if (!ctx || !dw || !x || !dw_w_oihw || !dw_scale || !pw_w_packed || (!y && !y_i8) || pw_cout < 1)
    return fail(ctx, PLHIP_ERR_INVALID, "plhip_dw_conv1x1_fused_int8: null / bad argument");
  if (plhip_status st = check_out_scale_act(ctx, "plhip_dw_conv1x1_fused_int8", out, false, pw_scale, "pw_scale", &pw_act, "1x1 activation"))
    return st;
  plhip::DwConvArgs a;
  const char* why;
  if (!dw_conv1x1_plan(dw, pw_cout, out, has_tail, &a, &why)) return fail(ctx, PLHIP_ERR_UNSUPPORTED, "plhip_dw_conv1x1_fused_int8: %s", why);
  if (!y && out != PLHIP_OUT_F32) return fail(ctx, PLHIP_ERR_INVALID, "plhip_dw_conv1x1_fused_int8: y required");
  if (y_i8 && !(calib_scale > 0.f)) return fail(ctx, PLHIP_ERR_INVALID, "plhip_dw_conv1x1_fused_int8: calib scale must be > 0");
  if (residual_relu && !residual) return fail(ctx, PLHIP_ERR_INVALID, "plhip_dw_conv1x1_fused_int8: residual_relu without a residual");
  if (!aligned(pw_w_packed, 16)) return fail(ctx, PLHIP_ERR_INVALID, "plhip_dw_conv1x1_fused_int8: packed weights must be 16-byte aligned");
  a.x = x;
  a.dw_w = dw_w_oihw;
  a.dw_scale = dw_scale;
  a.dw_bias = dw_bias;
  a.wp = (const int8_t*)pw_w_packed;
  a.y = y;
  a.scale = pw_scale;
  a.bias = pw_bias;
  a.act = pw_act;
  a.alpha = pw_alpha;
  a.res = residual;
  a.res_relu = residual_relu;
  a.y2 = y_i8;
  a.inv_scale2 = y_i8 ? 1.f / calib_scale : 0.f;  // type_trans.cc:45
  plhip::launch_dw_conv1x1(a, (int)out, ctx->stream);
  LAUNCHCHK(ctx, "dw_conv1x1_fused");
  return PLHIP_OK;
}

// ------------------------------------------------------------------ fc
size_t plhip_fc_packed_weight_bytes(int k, int n) {
  if (k < 1 || n < 1) return 0;
  return plhip::fc_packed_bytes(k, n);  // [dot4 layout][MFMA A fragments]
}

plhip_status plhip_pack_fc_weights(plhip_ctx* ctx, int k, int n, const int8_t* w_kn, void* w_packed) {
  if (!ctx || !w_kn || !w_packed || k < 1 || n < 1) return fail(ctx, PLHIP_ERR_INVALID, "plhip_pack_fc_weights: bad argument");
  plhip::launch_pack_fc(w_kn, (int8_t*)w_packed, k, n, ctx->stream);
  LAUNCHCHK(ctx, "pack_fc");
  return PLHIP_OK;
}

plhip_status plhip_fc_int8(plhip_ctx* ctx, int m, int k, int n, const int8_t* x, const void* w_packed, const float* scale,
                           const float* bias, int relu, void* y, plhip_out_kind out) {
  if (!ctx || !x || !w_packed || !y || m < 1 || k < 1 || n < 1) return fail(ctx, PLHIP_ERR_INVALID, "plhip_fc_int8: bad argument");
  if (plhip_status st = check_out_scale_act(ctx, "plhip_fc_int8", out, false, scale, "scale", nullptr)) return st;
  if (!aligned(w_packed, 4)) return fail(ctx, PLHIP_ERR_INVALID, "plhip_fc_int8: packed weights must be 4-byte aligned");
  plhip::launch_fc(x, (const int8_t*)w_packed, scale, bias, y, m, k, n, relu, (int)out, ctx->stream);
  LAUNCHCHK(ctx, "fc_i8");
  return PLHIP_OK;
}

// ------------------------------------------------------------------ calib / pool / softmax
plhip_status plhip_calib_f32_to_i8(plhip_ctx* ctx, const float* x, int8_t* y, float scale, int64_t count) {
  if (!ctx || !x || !y || count < 0 || !(scale > 0.f)) return fail(ctx, PLHIP_ERR_INVALID, "plhip_calib_f32_to_i8: bad argument");
  if (count == 0) return PLHIP_OK;
  plhip::launch_calib_f32_to_i8(x, y, scale, count, ctx->stream);
  LAUNCHCHK(ctx, "calib_f32_to_i8");
  return PLHIP_OK;
}

plhip_status plhip_calib_i8_to_f32(plhip_ctx* ctx, const int8_t* x, float* y, float scale, int64_t count) {
  if (!ctx || !x || !y || count < 0) return fail(ctx, PLHIP_ERR_INVALID, "plhip_calib_i8_to_f32: bad argument");
  if (count == 0) return PLHIP_OK;
  plhip::launch_calib_i8_to_f32(x, y, scale, count, ctx->stream);
  LAUNCHCHK(ctx, "calib_i8_to_f32");
  return PLHIP_OK;
}

plhip_status plhip_global_avg_pool_f32(plhip_ctx* ctx, const float* x, int nc, int spatial, float* y) {
  if (!ctx || !x || !y || nc < 1 || spatial < 1) return fail(ctx, PLHIP_ERR_INVALID, "plhip_global_avg_pool_f32: bad argument");
  plhip::launch_global_avg_pool(x, nc, spatial, y, ctx->stream);
  LAUNCHCHK(ctx, "global_avg_pool");
  return PLHIP_OK;
}

plhip_status plhip_softmax_f32(plhip_ctx* ctx, const float* x, int rows, int cols, float* y) {
  if (!ctx || !x || !y || rows < 1 || cols < 1) return fail(ctx, PLHIP_ERR_INVALID, "plhip_softmax_f32: bad argument");
  plhip::launch_softmax(x, rows, cols, y, ctx->stream);
  LAUNCHCHK(ctx, "softmax");
  return PLHIP_OK;
}

static plhip_status pool2d_impl(plhip_ctx* ctx, const plhip_pool_desc* d, const void* x, void* y, bool i8);
plhip_status plhip_pool2d_f32(plhip_ctx* ctx, const plhip_pool_desc* d, const float* x, float* y) {
  return pool2d_impl(ctx, d, x, y, false);
}
plhip_status plhip_pool2d_max_i8(plhip_ctx* ctx, const plhip_pool_desc* d, const int8_t* x, int8_t* y) {
  if (d && !d->is_max) return fail(ctx, PLHIP_ERR_UNSUPPORTED, "plhip_pool2d_max_i8: max pooling only (avg does not commute with the quantiser)");
  return pool2d_impl(ctx, d, x, y, true);
}
static plhip_status pool2d_impl(plhip_ctx* ctx, const plhip_pool_desc* d, const void* x, void* y, bool i8) {
  if (!ctx || !d || !x || !y) return fail(ctx, PLHIP_ERR_INVALID, "plhip_pool2d_f32: null argument");
  if (d->planes < 1 || d->h < 1 || d->w < 1 || d->oh < 1 || d->ow < 1 || d->kh < 1 || d->kw < 1 || d->stride[0] < 1 ||
      d->stride[1] < 1 || d->pad[0] < 0 || d->pad[1] < 0 || d->pad[2] < 0 || d->pad[3] < 0)
    return fail(ctx, PLHIP_ERR_INVALID, "plhip_pool2d_f32: bad descriptor");
  // every window must start inside the padded image (PoolOutputSize guarantees it, ceil_mode included; windows that
  // only cover padding yield 0 like pooling_basic)
  if ((d->oh - 1) * d->stride[0] - d->pad[0] >= d->h + d->pad[1] || (d->ow - 1) * d->stride[1] - d->pad[2] >= d->w + d->pad[3])
    return fail(ctx, PLHIP_ERR_INVALID, "plhip_pool2d_f32: output dims do not match the window geometry");
  if ((size_t)d->h * d->w >= ((size_t)1 << 31) || (size_t)d->oh * d->ow >= ((size_t)1 << 31))
    return fail(ctx, PLHIP_ERR_UNSUPPORTED, "plhip_pool2d_f32: plane too large");
  plhip::PoolArgs a;
  a.x = (const float*)x; a.y = (float*)y;
  a.planes = d->planes; a.h = d->h; a.w = d->w; a.oh = d->oh; a.ow = d->ow; a.kh = d->kh; a.kw = d->kw;
  a.sh = d->stride[0]; a.sw = d->stride[1]; a.pt = d->pad[0]; a.pb = d->pad[1]; a.pl = d->pad[2]; a.pr = d->pad[3];
  a.is_max = d->is_max ? 1 : 0; a.exclusive = d->exclusive ? 1 : 0;
  if (i8) plhip::launch_pool2d_max_i8(a, ctx->stream);
  else plhip::launch_pool2d(a, ctx->stream);
  LAUNCHCHK(ctx, "pool2d");
  return PLHIP_OK;
}

plhip_status plhip_elementwise_add_f32(plhip_ctx* ctx, const float* x, const float* y, float* out, int64_t count, int relu) {
  if (!ctx || !x || !y || !out || count < 0) return fail(ctx, PLHIP_ERR_INVALID, "plhip_elementwise_add_f32: bad argument");
  if (count == 0) return PLHIP_OK;
  plhip::launch_eltwise_add(x, y, out, count, relu, ctx->stream);
  LAUNCHCHK(ctx, "elementwise_add");
  return PLHIP_OK;
}

plhip_status plhip_hard_act_f32(plhip_ctx* ctx, plhip_hard_act_kind kind, const float* params, const float* x, float* y_f32,
                                int8_t* y_i8, float calib_scale, int64_t count) {
  if (!ctx || !params || !x || (!y_f32 && !y_i8) || count < 0 || (y_i8 && !(calib_scale > 0.f)))
    return fail(ctx, PLHIP_ERR_INVALID, "plhip_hard_act_f32: bad argument");
  if (kind != PLHIP_HARD_SWISH && kind != PLHIP_HARD_SIGMOID) return fail(ctx, PLHIP_ERR_UNSUPPORTED, "plhip_hard_act_f32: unknown kind");
  if (count == 0) return PLHIP_OK;
  plhip::launch_hard_act(kind == PLHIP_HARD_SWISH ? plhip::HARD_ACT_SWISH : plhip::HARD_ACT_SIGMOID, params, x, y_f32, y_i8,
                         calib_scale, count, ctx->stream);
  LAUNCHCHK(ctx, "hard_act");
  return PLHIP_OK;
}

plhip_status plhip_se_scale_f32(plhip_ctx* ctx, const float* x, const float* gate, int n, int c, int hw, float* y_f32, int8_t* y_i8,
                                float calib_scale) {
  if (!ctx || !x || !gate || (!y_f32 && !y_i8) || n < 1 || c < 1 || hw < 1 || (y_i8 && !(calib_scale > 0.f)))
    return fail(ctx, PLHIP_ERR_INVALID, "plhip_se_scale_f32: bad argument");
  const int64_t planes = (int64_t)n * c;
  if (planes > ((int64_t)1 << 30)) return fail(ctx, PLHIP_ERR_UNSUPPORTED, "plhip_se_scale_f32: too many planes");
  plhip::launch_se_scale(x, gate, y_f32, y_i8, calib_scale, planes, hw, ctx->stream);
  LAUNCHCHK(ctx, "se_scale");
  return PLHIP_OK;
}

static bool se_gate_act_ok(int act) { return act == PLHIP_ACT_NONE || act == PLHIP_ACT_RELU || act == PLHIP_ACT_RELU6 || act == PLHIP_ACT_LEAKY_RELU; }
int plhip_se_gate_supported(int c, int cr, int act1, int act2) {
  return c >= 8 && cr >= 8 && c <= plhip::SE_GATE_MAX_C && cr <= plhip::SE_GATE_MAX_C && se_gate_act_ok(act1) && se_gate_act_ok(act2);
}
size_t plhip_se_gate_packed_weight_bytes(int c, int cr) { return c < 1 || cr < 1 ? 0 : plhip::se_gate_packed_bytes(c, cr); }
plhip_status plhip_pack_se_gate_weights(plhip_ctx* ctx, int c, int cr, const int8_t* w1, const int8_t* w2, void* w_packed) {
  if (!ctx || !w1 || !w2 || !w_packed || !aligned(w_packed, 4)) return fail(ctx, PLHIP_ERR_INVALID, "plhip_pack_se_gate_weights: bad argument");
  if (!plhip_se_gate_supported(c, cr, 0, 0)) return fail(ctx, PLHIP_ERR_UNSUPPORTED, "plhip_pack_se_gate_weights: c / cr outside 8..960");
  plhip::launch_se_gate_pack(w1, w2, w_packed, c, cr, ctx->stream);
  LAUNCHCHK(ctx, "se_gate_pack");
  return PLHIP_OK;
}
plhip_status plhip_se_gate_int8(plhip_ctx* ctx, const plhip_se_gate_desc* d, const float* pooled, const void* w_packed,
                                const float* scale1, const float* bias1, const float* scale2, const float* bias2, float* gate) {
  if (!ctx || !d || !pooled || !w_packed || !scale1 || !scale2 || !gate || d->n < 1 || !(d->calib_scale > 0.f) || !aligned(w_packed, 4))
    return fail(ctx, PLHIP_ERR_INVALID, "plhip_se_gate_int8: bad argument");
  if (!plhip_se_gate_supported(d->c, d->cr, d->act1, d->act2)) return fail(ctx, PLHIP_ERR_UNSUPPORTED, "plhip_se_gate_int8: outside the envelope");
  plhip::SeGateArgs a;
  a.pooled = pooled;
  a.inv = 1.f / d->calib_scale;  // type_trans.cc:45, as launch_calib_f32_to_i8
  a.w1 = static_cast<const uint32_t*>(w_packed);
  a.w2 = a.w1 + (size_t)((d->c + 3) / 4) * d->cr;
  a.s1 = scale1; a.b1 = bias1; a.s2 = scale2; a.b2 = bias2;
  a.act1 = d->act1; a.act2 = d->act2; a.alpha1 = d->act1_alpha; a.alpha2 = d->act2_alpha;
  a.slope = d->slope; a.offset = d->offset;
  a.gate = gate; a.c = d->c; a.cr = d->cr;
  plhip::launch_se_gate(a, d->n, ctx->stream);
  LAUNCHCHK(ctx, "se_gate");
  return PLHIP_OK;
}

// ------------------------------------------------------------------ self test
// Known-answer 1x1 conv (M = 70, K = 45, N = 2 x 36) with asymmetric data, int32 accumulators compared with a host
// triple loop: proves the MFMA operand / accumulator lane maps and the in-register transpose on this device.
plhip_status plhip_selftest(plhip_ctx* ctx) {
  if (!ctx) return fail(ctx, PLHIP_ERR_INVALID, "null ctx");
  plhip_conv_desc d;
  memset(&d, 0, sizeof(d));
  d.n = 2; d.cin = 45; d.h = 6; d.w = 6; d.cout = 70; d.kh = 1; d.kw = 1;
  d.stride[0] = d.stride[1] = 1; d.dil[0] = d.dil[1] = 1; d.groups = 1;
  const int N = 36;
  std::vector<int8_t> hx((size_t)d.n * d.cin * N), hw((size_t)d.cout * d.cin);
  for (size_t i = 0; i < hx.size(); ++i) hx[i] = (int8_t)((int)((i * 37 + (i >> 3) * 11 + 5) % 255) - 127);
  for (size_t i = 0; i < hw.size(); ++i) hw[i] = (int8_t)((int)((i * 101 + (i >> 2) * 7 + 13) % 255) - 127);
  std::vector<int32_t> ref((size_t)d.n * d.cout * N), got(ref.size());
  for (int b = 0; b < d.n; ++b)
    for (int m = 0; m < d.cout; ++m)
      for (int n = 0; n < N; ++n) {
        int32_t s = 0;
        for (int k = 0; k < d.cin; ++k) s += (int32_t)hw[(size_t)m * d.cin + k] * (int32_t)hx[((size_t)b * d.cin + k) * N + n];
        ref[((size_t)b * d.cout + m) * N + n] = s;
      }
  void *dx = nullptr, *dw = nullptr, *dwp = nullptr, *dy = nullptr;
  plhip_status st;
  if ((st = plhip_malloc(ctx, hx.size(), &dx)) || (st = plhip_malloc(ctx, hw.size(), &dw)) ||
      (st = plhip_malloc(ctx, plhip_conv_packed_weight_bytes(&d), &dwp)) || (st = plhip_malloc(ctx, ref.size() * 4, &dy)))
    return st;
  st = plhip_memcpy_h2d(ctx, dx, hx.data(), hx.size());
  if (!st) st = plhip_memcpy_h2d(ctx, dw, hw.data(), hw.size());
  if (!st) st = plhip_pack_conv_weights(ctx, &d, (const int8_t*)dw, dwp);
  if (!st) st = plhip_conv2d_int8(ctx, &d, (const int8_t*)dx, dwp, nullptr, nullptr, dy, PLHIP_OUT_I32_ACC, nullptr, 0);
  if (!st) st = plhip_memcpy_d2h(ctx, got.data(), dy, got.size() * 4);
  plhip_free(ctx, dx); plhip_free(ctx, dw); plhip_free(ctx, dwp); plhip_free(ctx, dy);
  if (st) return st;
  size_t bad = 0;
  for (size_t i = 0; i < ref.size(); ++i) bad += ref[i] != got[i];
  if (bad) {
    char msg[64];
    snprintf(msg, sizeof msg, "%zu of %zu", bad, ref.size());
    return fail(ctx, PLHIP_ERR_HIP, "plhip_selftest: MFMA known-answer GEMM mismatched in %s accumulators", msg);
  }
  return PLHIP_OK;
}

}  // extern "C"

// tests / A-B runs: force the wide-tile GEMM's n tiles per block (4, 7, 8), 0 = automatic choice, -1 = environment
extern "C" void plhip_debug_wide_ntt(int v) { plhip::debug_set_wide_ntt(v); }
// Diagnostics switches of the shipped library (declared in include/plhip.h).  NOTHING in the library reads the environment:
// the A/B knobs the kernels' launchers consult (plhip::knob) live in this table and change only through
// plhip_debug_set; an unknown key is refused.  "STAMPS" (timeline stamps) exists in a `make EXPERIMENTS=1` build only.
namespace plhip {
namespace {
struct Knob { const char* name; int value; bool set; };
Knob g_knobs[] = {
    {"STEM_MFMA", 0, false}, {"CONV_PATCH", 0, false}, {"CONV_PATCH_S2", 0, false},
    {"STEM7", 0, false}, {"DW_STAGE", 0, false}, {"DW_STAGE_NP2", 0, false}, {"DW_FASTV", 0, false}, {"DW5_DIRECT", 0, false},
    {"DW_RS1", 0, false}, {"DW_RS2", 0, false}, {"GEMM_VARIANT", 0, false}, {"GEMM_AREG", 0, false}, {"GEMM_MA", 0, false},
    {"SUBSAMPLE_1X1", 0, false}, {"GEMM_TR", 0, false}, {"TR_CFG", 0, false},
    {"GEMM_WIDE", 0, false}, {"WIDE_NTT", 0, false}, {"FC_MFMA", 0, false}, {"IMPLICIT_GEMM", 0, false}, {"FUSED_STREAM", 0, false}, {"FUSED_SMALL", 0, false}, {"DWCONV_FUSED", 0, false},
#ifdef PLHIP_EXPERIMENTS
    {"STAMPS", 0, false},
#endif
};
}  // namespace
int knob(const char* name, int dflt) {
  for (const Knob& k : g_knobs)
    if (!strcmp(k.name, name)) return k.set ? k.value : dflt;
  return dflt;
}
}  // namespace plhip
extern "C" int plhip_debug_set(const char* key, int value) {
  if (!key) return -1;
  for (plhip::Knob& k : plhip::g_knobs)
    if (!strcmp(k.name, key)) { k.value = value; k.set = true; return 0; }
  return -1;
}

#ifdef PLHIP_EXPERIMENTS
// Timeline stamp buffers, one per kernel family, allocated on the first launch that stamps.  Not part of
// include/plhip.h: the timeline tools (tools/*_timeline.py) read them with plhip_debug_read_stamps after the launch.
namespace plhip {
namespace {
struct StampBuf { const char* family; unsigned long long* p; size_t bytes; };
StampBuf g_stamp_bufs[] = {{"gemm", nullptr, 0}, {"tr", nullptr, 0}, {"wide", nullptr, 0}, {"patch", nullptr, 0},
                           {"fw", nullptr, 0}, {"fs", nullptr, 0}, {"f7", nullptr, 0}};
StampBuf* find_stamp_buf(const char* family) {
  for (StampBuf& b : g_stamp_bufs)
    if (!strcmp(b.family, family)) return &b;
  return nullptr;
}
}  // namespace
unsigned long long* stamp_buffer(const char* family, size_t bytes) {
  if (!knob("STAMPS", 0)) return nullptr;
  StampBuf* b = find_stamp_buf(family);
  if (!b->p && hipMalloc((void**)&b->p, bytes) == hipSuccess) {
    b->bytes = bytes;
    (void)hipMemset(b->p, 0, bytes);
  }
  return b->p;
}
}  // namespace plhip
// the stamps of the last stamping launch of `family` ("gemm", "tr", "wide", "patch", "fw", "fs", "f7"): 0, or -1 when that
// family has not stamped yet
extern "C" int plhip_debug_read_stamps(const char* family, void* dst_host, size_t bytes) {
  plhip::StampBuf* b = family && dst_host ? plhip::find_stamp_buf(family) : nullptr;
  if (!b || !b->p || hipDeviceSynchronize() != hipSuccess) return -1;
  return hipMemcpy(dst_host, b->p, bytes < b->bytes ? bytes : b->bytes, hipMemcpyDeviceToHost) == hipSuccess ? 0 : -1;
}
#endif
