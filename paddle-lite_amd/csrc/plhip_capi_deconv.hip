// plhip_capi_deconv.hip — the C ABI (include/plhip.h), beside part 2 (plhip_capi_conv.hip): conv2d_transpose.  Argument validation,
// the choice between the MFMA phase route and the direct route (deconv_plan.h; knob DECONV_ROUTE = 1 forces the direct one) and the
// launches (deconv_i8.hip).  plhip_deconv_impl_name, the packed-weight size, the packer and the run all go through deconv_route, so
// they cannot disagree.
#include "plhip_capi.h"

namespace {

enum DeconvRoute { DECONV_BAD = 0, DECONV_PHASE, DECONV_DIRECT };

struct DeconvGeom {
  plhip::DeconvProblem p;
  int oh, ow;
  const char* why;  // DECONV_BAD: the text the entry points report
};

// validates the descriptor, computes the output dims and picks the route
DeconvRoute deconv_route(const plhip_deconv_desc* dd, DeconvGeom* g) {
  g->why = "null descriptor";
  if (!dd) return DECONV_BAD;
  const plhip_conv_desc* d = &dd->conv;
  g->why = "a dimension, stride or dilation < 1, a negative padding or output size";
  if (d->n < 1 || d->cin < 1 || d->cout < 1 || d->h < 1 || d->w < 1 || d->kh < 1 || d->kw < 1 || d->groups < 1) return DECONV_BAD;
  if (d->stride[0] < 1 || d->stride[1] < 1 || d->dil[0] < 1 || d->dil[1] < 1 || dd->out_h < 0 || dd->out_w < 0) return DECONV_BAD;
  for (int i = 0; i < 4; ++i)
    if (d->pad[i] < 0) return DECONV_BAD;
  g->why = "groups must divide cin and cout";
  if (d->cin % d->groups || d->cout % d->groups) return DECONV_BAD;
  plhip::DeconvProblem& p = g->p;
  p.n = d->n; p.cin = d->cin; p.cout = d->cout; p.h = d->h; p.w = d->w; p.kh = d->kh; p.kw = d->kw;
  for (int i = 0; i < 4; ++i) p.pad[i] = d->pad[i];
  p.sh = d->stride[0]; p.sw = d->stride[1]; p.dh = d->dil[0]; p.dw = d->dil[1]; p.groups = d->groups;
  p.out_h = dd->out_h; p.out_w = dd->out_w;
  g->why = "non-positive output, or an output size outside [default, default + stride)";
  if (!plhip::deconv_out_dims(p, &g->oh, &g->ow)) return DECONV_BAD;
  g->why = "";
  return plhip::deconv_phase_supported(p) && plhip::knob("DECONV_ROUTE", 0) != 1 ? DECONV_PHASE : DECONV_DIRECT;
}

size_t filter_bytes(const plhip::DeconvProblem& p) { return (size_t)p.cin * (p.cout / p.groups) * p.kh * p.kw; }

}  // namespace

extern "C" {

plhip_status plhip_deconv_out_dims(const plhip_deconv_desc* d, int* out_h, int* out_w) {
  DeconvGeom g;
  if (!out_h || !out_w) return fail(nullptr, PLHIP_ERR_INVALID, "plhip_deconv_out_dims: null argument");
  if (deconv_route(d, &g) == DECONV_BAD) return fail(nullptr, PLHIP_ERR_INVALID, "plhip_deconv_out_dims: %s", g.why);
  *out_h = g.oh;
  *out_w = g.ow;
  return PLHIP_OK;
}

const char* plhip_deconv_impl_name(const plhip_deconv_desc* d) {
  DeconvGeom g;
  switch (deconv_route(d, &g)) {
    case DECONV_PHASE: return "deconv_phase_int8_mfma32x32x32";
    case DECONV_DIRECT: return "deconv_direct_int8";
    default: return "invalid";
  }
}

size_t plhip_deconv_packed_weight_bytes(const plhip_deconv_desc* d) {
  DeconvGeom g;
  switch (deconv_route(d, &g)) {
    case DECONV_PHASE: return plhip::deconv_phase_packed_bytes(g.p);
    case DECONV_DIRECT: return filter_bytes(g.p);
    default: return 0;
  }
}

plhip_status plhip_pack_deconv_weights(plhip_ctx* ctx, const plhip_deconv_desc* d, const int8_t* w_iohw, void* w_packed) {
  DeconvGeom g;
  if (!ctx || !w_iohw || !w_packed) return fail(ctx, PLHIP_ERR_INVALID, "plhip_pack_deconv_weights: null argument");
  const DeconvRoute r = deconv_route(d, &g);
  if (r == DECONV_BAD) return fail(ctx, PLHIP_ERR_INVALID, "plhip_pack_deconv_weights: %s", g.why);
  if (r == DECONV_PHASE) {
    plhip::launch_pack_deconv_phase(w_iohw, (int8_t*)w_packed, g.p, ctx->stream);
    LAUNCHCHK(ctx, "pack_deconv_phase");
  } else {
    HIPCHK(ctx, hipMemcpyAsync(w_packed, w_iohw, filter_bytes(g.p), hipMemcpyDeviceToDevice, ctx->stream));
  }
  return PLHIP_OK;
}

plhip_status plhip_conv2d_transpose_int8(plhip_ctx* ctx, const plhip_deconv_desc* d, const int8_t* x, const void* w_packed,
                                         const float* scale, const float* bias, void* y, plhip_out_kind out) {
  DeconvGeom g;
  if (!ctx || !x || !w_packed || !y) return fail(ctx, PLHIP_ERR_INVALID, "plhip_conv2d_transpose_int8: null argument");
  const DeconvRoute r = deconv_route(d, &g);
  if (r == DECONV_BAD) return fail(ctx, PLHIP_ERR_INVALID, "plhip_conv2d_transpose_int8: %s", g.why);
  if (plhip_status st = check_out_scale_act(ctx, "plhip_conv2d_transpose_int8", out, false, scale, "scale", &d->conv.act)) return st;
  const plhip::DeconvProblem& p = g.p;
  // the kernels index one image's input and output, and the direct kernel all outputs, with 31 bits
  if ((size_t)p.cin * p.h * p.w >= ((size_t)1 << 31) || (size_t)p.n * p.cout * g.oh * g.ow >= ((size_t)1 << 31))
    return fail(ctx, PLHIP_ERR_UNSUPPORTED, "plhip_conv2d_transpose_int8: cin * h * w and n * cout * oh * ow must be below 2^31");
  plhip::DeconvArgs a;
  memset(&a, 0, sizeof(a));
  a.x = x; a.wp = (const int8_t*)w_packed; a.y = y; a.scale = scale; a.bias = bias;
  a.n = p.n; a.cin = p.cin; a.cout = p.cout; a.h = p.h; a.w = p.w; a.oh = g.oh; a.ow = g.ow; a.kh = p.kh; a.kw = p.kw;
  a.pt = p.pad[0]; a.pl = p.pad[2]; a.sh = p.sh; a.sw = p.sw; a.dh = p.dh; a.dw = p.dw; a.groups = p.groups;
  a.act = d->conv.act; a.alpha = d->conv.act_alpha;
  if (r == DECONV_DIRECT) {
    plhip::launch_deconv_direct(a, (int)out, ctx->stream);
    LAUNCHCHK(ctx, "deconv_direct");
    return PLHIP_OK;
  }
  if (!aligned(w_packed, 16)) return fail(ctx, PLHIP_ERR_INVALID, "plhip_conv2d_transpose_int8: packed weights must be 16-byte aligned");
  plhip::DeconvPlan q;
  if (!plhip::deconv_phase_plan(p, g.oh, g.ow, &q)) return fail(ctx, PLHIP_ERR_UNSUPPORTED, "plhip_conv2d_transpose_int8: phase grid too large");
  a.NCH = q.NCH; a.MT = q.MT; a.TY = q.TY; a.TX = q.TX; a.NV = q.NV; a.NUq = q.NUq; a.TR = q.TR; a.CWq = q.CWq;
  a.bands = q.bands; a.nseg = q.nseg; a.IR = q.IR; a.WQ = q.WQ; a.half = q.half;
  a.nblocks = q.nblocks; a.nblocks_per_xcd = q.nblocks_per_xcd; a.lds = q.lds;
  plhip::launch_deconv_phase(a, (int)out, ctx->stream);
  LAUNCHCHK(ctx, "deconv_phase");
  return PLHIP_OK;
}

}  // extern "C"
