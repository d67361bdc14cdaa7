// plhip_capi_ctx.hip — the C ABI (include/plhip.h), part 1 of 4: contexts, device memory, graph capture, events, the self test, and
// the diagnostics knob table (plhip_debug_set).  The compute entry points are in plhip_capi_conv.hip (convolutions),
// plhip_capi_image.hip (uint8 images and frames) and plhip_capi_ops.hip (fc and the glue ops).  No allocation and no
// synchronisation happens inside a compute entry point, so callers may capture them into a hipGraph.
#include "plhip_capi.h"

namespace plhip {
namespace {
thread_local char g_err[512] = "";
}
plhip_status fail(plhip_ctx* c, plhip_status st, const char* fmt, const char* a, const char* b) {
  char* dst = c ? c->err : g_err;
  snprintf(dst, 512, fmt, a, b);
  return st;
}
}  // namespace plhip

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
const char* plhip_last_error(plhip_ctx* ctx) { return ctx ? ctx->err : plhip::g_err; }

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
    {"CONV_GROUPED", 0, false}, {"DECONV_ROUTE", 0, false},
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
