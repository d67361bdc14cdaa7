// plhip_capi_conv.hip — the C ABI (include/plhip.h), part 2 of 4: convolutions.  Argument validation, route selection (the analogue of
// ConvCompute<kInt8,*>::PrepareForRun's impl_ choice, lite/kernels/arm/conv_compute.cc:87-185) and launches of conv2d, the calib /
// image stems, depthwise and the two fused depthwise pairs.
//
// A conv2d implementation is ONE row of kRoutes: the predicate that takes a descriptor, the packed-weight and workspace sizes, the
// weight packer and the launch recipe.  The public functions pick the row (pick_route: the first whose predicate holds) and use
// one member of it, so pack and run cannot disagree.  A new route is a new row and its functions.
#include "plhip_capi.h"

namespace {

typedef const plhip_conv_desc* Desc;

struct ConvGeom {
  int oh, ow, G, Mg, Cg, Kg, N, Np, MA, MT, MT32, KS;
  bool is_1x1_s1_p0;
};
typedef const ConvGeom& Geom;

// validates the descriptor and computes the geometry; which implementation runs it is pick_route's business
bool conv_geom(Desc d, ConvGeom* g) {
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
  return true;
}

struct ConvTail {  // fused graph tail of an fp32-output conv (plhip_conv2d_int8_fused)
  const float* residual;
  int residual_relu;
  int8_t* y_i8;
  float calib_scale;
};

struct ConvIo {  // the operands of one conv2d call
  const int8_t* x;
  const void* w_packed;
  const float *scale, *bias;
  void* y;
  plhip_out_kind out;
  void* workspace;
  size_t workspace_bytes;
  const ConvTail* tail;  // or nullptr
};

size_t out_elem_size(plhip_out_kind out) { return out == PLHIP_OUT_I8 ? 1 : 4; }

// the fused tail of the argument structs that spell it alike: GemmArgs, PatchArgs, GroupedArgs, DirectS2Args, DwConvArgs
template <class Args>
void set_tail(Args& a, const ConvTail* t) {
  a.res = t ? t->residual : nullptr;
  a.res_relu = t ? t->residual_relu : 0;
  a.y2 = t ? t->y_i8 : nullptr;
  a.inv_scale2 = (t && t->y_i8) ? 1.f / t->calib_scale : 0.f;  // type_trans.cc:45
}
bool has_tail(const ConvIo& io) { return io.tail && (io.tail->residual || io.tail->y_i8); }
// vector stores: y on 4 elements, the residual on 16 bytes, the int8 copy on 4
bool vec_store_ok(const ConvIo& io) {
  return aligned(io.y, 4 * out_elem_size(io.out)) && aligned(io.tail ? io.tail->residual : nullptr, 16) &&
         aligned(io.tail ? io.tail->y_i8 : nullptr, 4);
}

// ------------------------------------------------------------------ workspaces
size_t no_workspace(Desc, Geom) { return 0; }
size_t im2col_bytes(Desc d, Geom g) { return (size_t)d->n * g.G * g.Kg * g.Np; }
// dims of the padded copy of the implicit-GEMM route: stride 1 the padded plane; stride 2 ONE of the 4 phase planes
// (rows / columns 2y + p, 2x + q of the padded plane), its rows padded to a multiple of 4 columns
void padded_dims(Desc d, int* ph, int* pw) {
  const int PH = d->h + d->pad[0] + d->pad[1], PW = d->w + d->pad[2] + d->pad[3];
  if (d->stride[0] == 2) {
    *ph = (PH + 1) / 2;
    *pw = rup((PW + 1) / 2, 4);
  } else {
    *ph = PH;
    *pw = PW;
  }
}
size_t padded_input_bytes(Desc d, Geom) {  // + slack: the last 16-byte pieces run past the last row
  int ph, pw;
  padded_dims(d, &ph, &pw);
  const size_t b = (size_t)d->n * d->cin * (d->stride[0] == 2 ? 4 : 1) * ph * pw;
  return ((b + 3) & ~(size_t)3) + 64;
}
// the padded copy of the patch route (conv_patch_i8.hip): rows of PWp (a multiple of 8) bytes, + slack for the tiles that run
// past the last plane
size_t patch_input_bytes(Desc d, Geom) {
  const int pwp = plhip::conv_patch_row_pitch(d->w, d->pad[2], d->pad[3]);
  const size_t b = (size_t)d->n * d->cin * (d->h + d->pad[0] + d->pad[1]) * pwp;
  return ((b + 15) & ~(size_t)15) + 4096;
}
// the phase-split copy of the stride-2 patch route: 4 phase planes per channel, rows of PW2p (a multiple of 8) bytes
void patch_s2_dims(Desc d, int* ph2, int* pw2p) {
  *pw2p = plhip::conv_patch_s2_row_pitch(d->w, d->pad[2], d->pad[3]);
  *ph2 = (d->h + d->pad[0] + d->pad[1] + 1) >> 1;
}
size_t patch_s2_input_bytes(Desc d, Geom) {
  int ph2, pw2p;
  patch_s2_dims(d, &ph2, &pw2p);
  const size_t b = (size_t)d->n * d->cin * 4 * ph2 * pw2p;
  return ((b + 15) & ~(size_t)15) + 4096;
}
// the padded-copy kernels' arguments (pad_input, pad_rows8, pad_phase8): planes of ph x pw bytes into the workspace, `total` bytes
plhip::PadArgs pad_args(Desc d, const ConvIo& io, int planes, int ph, int pw, size_t total) {
  plhip::PadArgs pa = plhip::PadArgs();
  pa.stride = d->stride[0];
  pa.x = io.x;
  pa.xp = (int8_t*)io.workspace;
  pa.planes = planes;
  pa.h = d->h; pa.w = d->w; pa.ph = ph; pa.pw = pw; pa.pt = d->pad[0]; pa.pl = d->pad[2];
  pa.total = (long)total;
  return pa;
}

// ------------------------------------------------------------------ 1x1 GEMM and im2col + GEMM
bool takes_gemm_1x1(Desc, Geom g) { return g.is_1x1_s1_p0; }  // GEMM straight on the NCHW slab
bool takes_im2col(Desc, Geom) { return true; }                // everything else (GemmLikeConv)
size_t gemm_packed_bytes(Desc, Geom g) { return (size_t)g.G * g.MT32 * g.KS * 1024; }
plhip_status pack_gemm(plhip_ctx* ctx, Desc, Geom g, const int8_t* w_oihw, void* w_packed) {
  plhip::launch_pack_weights(w_oihw, (int8_t*)w_packed, g.G, g.Mg, g.Kg, g.MT32, g.KS, ctx->stream);
  return PLHIP_OK;
}
// what the GEMM and the implicit-GEMM routes fill alike
plhip::GemmArgs gemm_args(Desc d, Geom g) {
  plhip::GemmArgs a = plhip::GemmArgs();
  a.M = g.Mg; a.K = g.Kg; a.KS = g.KS; a.MT = g.MT;
  a.HWY = g.N;
  a.y_bstride = (size_t)d->cout * g.N;
  a.act = d->act; a.alpha = d->act_alpha;
  a.im_s = 1;
  return a;
}
// One launch_gemm_i8 call without its pointers: the shape half of the arguments, as direct_s2_args for the stems, and what the
// shape alone says about vector stores and aligned rows.  The caller adds the pointers and their alignment.
struct GemmCall {
  plhip::GemmArgs a;
  bool vec_store, aligned_loads;
};
struct GemmB {  // the B operand of the GEMM route: the NCHW slab itself (1x1) or the im2col buffer
  size_t bstride, gstride;
  int xp;
  long bytes;
  bool aligned_rows;
};
GemmB gemm_b_1x1(Desc d, Geom g) { return {(size_t)d->cin * g.N, (size_t)g.Cg * g.N, g.N, (long)d->n * d->cin * g.N, (g.N & 3) == 0}; }
GemmB gemm_b_im2col(Desc d, Geom g) { return {(size_t)g.G * g.Kg * g.Np, (size_t)g.Kg * g.Np, g.Np, (long)im2col_bytes(d, g), true}; }
GemmCall gemm_call(Desc d, Geom g, const GemmB& b, int grp) {  // group grp of the 1x1 / im2col GEMM
  GemmCall c = {gemm_args(d, g), g.Np == g.N, b.aligned_rows};
  c.a.HWX = g.Np; c.a.XP = b.xp; c.a.NB = d->n; c.a.NT = cdiv(d->n * g.Np, 128);
  c.a.x_bytes = b.bytes - (long)grp * (long)b.gstride;
  c.a.x_bstride = b.bstride;
  return c;
}
plhip_status run_gemm_groups(plhip_ctx* ctx, Desc d, Geom g, const ConvIo& io, const GemmB& b, const int8_t* base) {
  const size_t esz = out_elem_size(io.out);
  for (int grp = 0; grp < g.G; ++grp) {
    const size_t yoff = (size_t)grp * g.Mg * g.N;
    GemmCall c = gemm_call(d, g, b, grp);
    plhip::GemmArgs& a = c.a;
    set_tail(a, io.tail);
    a.wp = (const int8_t*)io.w_packed + (size_t)grp * g.MT32 * g.KS * 1024;
    a.x = base + (size_t)grp * b.gstride;
    a.y = io.y ? (char*)io.y + yoff * esz : nullptr;
    if (a.res) a.res += yoff;
    if (a.y2) a.y2 += yoff;
    a.scale = io.scale ? io.scale + (size_t)grp * g.Mg : nullptr;
    a.bias = io.bias ? io.bias + (size_t)grp * g.Mg : nullptr;
    if (plhip::launch_gemm_i8(a, g.MA, (int)io.out, c.vec_store && vec_store_ok(io), c.aligned_loads && aligned(base, 4), ctx->stream) != 0)
      return fail(ctx, PLHIP_ERR_UNSUPPORTED, "conv2d: GEMM shape outside every kernel");
    LAUNCHCHK(ctx, "gemm_i8");
  }
  return PLHIP_OK;
}
plhip_status run_gemm_1x1(plhip_ctx* ctx, Desc d, Geom g, const ConvIo& io) {
  return run_gemm_groups(ctx, d, g, io, gemm_b_1x1(d, g), io.x);
}
plhip_status run_im2col(plhip_ctx* ctx, Desc d, Geom g, const ConvIo& io) {
  const size_t need = im2col_bytes(d, g);
  if (!io.workspace || io.workspace_bytes < need || !aligned(io.workspace, 4))
    return fail(ctx, PLHIP_ERR_WORKSPACE, "plhip_conv2d_int8: im2col workspace missing, too small or unaligned");
  if (g.Kg > 65535 || (size_t)d->n * g.G > 65535)
    return fail(ctx, PLHIP_ERR_UNSUPPORTED, "plhip_conv2d_int8: im2col route needs Kg and batch*groups <= 65535");
  plhip::Im2colArgs ia;
  ia.x = io.x;
  ia.col = (int8_t*)io.workspace;
  ia.cin = d->cin; ia.cin_g = g.Cg; ia.h = d->h; ia.w = d->w; ia.kh = d->kh; ia.kw = d->kw;
  ia.pt = d->pad[0]; ia.pl = d->pad[2]; ia.sh = d->stride[0]; ia.sw = d->stride[1]; ia.dh = d->dil[0]; ia.dw = d->dil[1];
  ia.oh = g.oh; ia.ow = g.ow; ia.G = g.G; ia.Kg = g.Kg; ia.N = g.N; ia.Np = g.Np;
  ia.rows = (size_t)d->n * g.G * g.Kg;
  plhip::launch_im2col(ia, ctx->stream);
  LAUNCHCHK(ctx, "im2col");
  return run_gemm_groups(ctx, d, g, io, gemm_b_im2col(d, g), (const int8_t*)io.workspace);
}

// ------------------------------------------------------------------ the direct stems: 3x3 stride 2 (small Cin) and ResNet50's 7x7 stride 2
bool takes_direct_s2(Desc d, Geom) {  // reference: DirectConv / conv3x3s2_direct_int8.cc
  return plhip::conv3x3s2_direct_supported(d->cin, d->cout, d->kh, d->kw, d->stride[0], d->stride[1], d->dil[0], d->dil[1], d->groups,
                                           d->pad[2]);
}
bool takes_stem7(Desc d, Geom g) {  // direct (conv_stem7_i8.hip), no padded copy
  return plhip::conv7x7s2_stem_supported(d->cin, d->cout, d->kh, d->kw, d->stride[0], d->stride[1], d->dil[0], d->dil[1], d->groups,
                                         d->n, d->h, d->w, g.oh, g.ow, d->pad[2]);
}
size_t direct_s2_packed_bytes(Desc d, Geom) { return plhip::conv3x3s2_direct_packed_bytes(d->cin, d->cout); }
size_t stem7_packed_bytes(Desc d, Geom) { return plhip::conv7x7s2_stem_packed_bytes(d->cout); }
plhip_status pack_direct_s2(plhip_ctx* ctx, Desc d, Geom, const int8_t* w_oihw, void* w_packed) {
  if (!aligned(w_packed, 4)) return fail(ctx, PLHIP_ERR_INVALID, "plhip_pack_conv_weights: packed buffer must be 4-byte aligned");
  plhip::launch_pack_conv3x3s2_direct(w_oihw, (uint32_t*)w_packed, d->cin, d->cout, ctx->stream);
  return PLHIP_OK;
}
plhip_status pack_stem7(plhip_ctx* ctx, Desc d, Geom, const int8_t* w_oihw, void* w_packed) {
  plhip::launch_pack_conv7x7s2_stem(w_oihw, (int8_t*)w_packed, d->cin, d->cout, ctx->stream);
  return PLHIP_OK;
}
// the shape half of a stem kernel's arguments; the pointers and the fused front / tail are the caller's
plhip::DirectS2Args direct_s2_args(Desc d, Geom g) {
  plhip::DirectS2Args a = plhip::DirectS2Args();
  a.n = d->n; a.cin = d->cin; a.h = d->h; a.w = d->w; a.cout = d->cout; a.coutp = rup(d->cout, 4);
  a.oh = g.oh; a.ow = g.ow; a.pt = d->pad[0]; a.pl = d->pad[2]; a.act = d->act; a.alpha = d->act_alpha;
  return a;
}
plhip::DirectS2Args direct_s2_args(Desc d, Geom g, const ConvIo& io) {
  plhip::DirectS2Args a = direct_s2_args(d, g);
  a.x = io.x; a.wp = (const uint32_t*)io.w_packed; a.y = io.y; a.scale = io.scale; a.bias = io.bias;
  return a;
}
plhip_status run_direct_s2(plhip_ctx* ctx, Desc d, Geom g, const ConvIo& io) {
  if (has_tail(io)) return fail(ctx, PLHIP_ERR_UNSUPPORTED, "plhip_conv2d_int8_fused: the direct 3x3 s2 stem has no fused tail");
  plhip::launch_conv3x3s2_direct(direct_s2_args(d, g, io), (int)io.out, ctx->stream);
  LAUNCHCHK(ctx, "conv3x3s2_direct");
  return PLHIP_OK;
}
plhip_status run_stem7(plhip_ctx* ctx, Desc d, Geom g, const ConvIo& io) {
  if (!aligned(io.w_packed, 16)) return fail(ctx, PLHIP_ERR_INVALID, "plhip_conv2d_int8: packed weights must be 16-byte aligned");
  plhip::DirectS2Args a = direct_s2_args(d, g, io);
  set_tail(a, io.tail);
  plhip::launch_conv7x7s2_stem(a, (int)io.out, vec_store_ok(io), ctx->stream);
  LAUNCHCHK(ctx, "conv7x7s2_stem");
  return PLHIP_OK;
}

// ------------------------------------------------------------------ the patch kernel (conv_patch_i8.hip)
// dense 3x3 stride 1 with Cin % 32 == 0: 3 shifted copies of the input rows per 32-channel chunk in LDS instead of 9 K rows per
// channel; dense 3x3 stride 2 (ResNet50's downsampling convs): the same kernel as a 2x2 stride-1 conv over the 4 phase planes of
// every channel
bool takes_patch(Desc d, Geom g) {
  return plhip::conv_patch_supported(d->cin, d->cout, d->kh, d->kw, d->stride[0], d->stride[1], d->dil[0], d->dil[1], d->groups, d->w,
                                     d->pad[2], d->pad[3]) &&
         patch_input_bytes(d, g) < ((size_t)1 << 31) - 4096 && g.oh >= 1 &&
         // (global mode, planes smaller than a tile: a 16-byte output piece may end in the NEXT image, not beyond it)
         !(plhip::conv_patch_global(plhip::conv_patch_row_pitch(d->w, d->pad[2], d->pad[3])) && g.oh * g.ow < 16);
}
bool takes_patch_s2(Desc d, Geom g) {
  return plhip::conv_patch_s2_supported(d->cin, d->cout, d->kh, d->kw, d->stride[0], d->stride[1], d->dil[0], d->dil[1], d->groups,
                                        d->w, d->pad[2], d->pad[3]) &&
         patch_s2_input_bytes(d, g) < ((size_t)1 << 31) - 4096 &&
         !(plhip::conv_patch_global(plhip::conv_patch_s2_row_pitch(d->w, d->pad[2], d->pad[3])) && g.oh * g.ow < 16);
}
size_t patch_packed_bytes(Desc d, Geom) { return plhip::conv_patch_packed_bytes(d->cin, d->cout); }
size_t patch_s2_packed_bytes(Desc d, Geom) { return plhip::conv_patch_s2_packed_bytes(d->cin, d->cout); }
plhip_status pack_patch(plhip_ctx* ctx, Desc d, Geom, const int8_t* w_oihw, void* w_packed) {
  plhip::launch_pack_conv_patch(w_oihw, (int8_t*)w_packed, d->cin, d->cout, ctx->stream);
  return PLHIP_OK;
}
plhip_status pack_patch_s2(plhip_ctx* ctx, Desc d, Geom, const int8_t* w_oihw, void* w_packed) {
  plhip::launch_pack_conv_patch_s2(w_oihw, (int8_t*)w_packed, d->cin, d->cout, ctx->stream);
  return PLHIP_OK;
}
// the shape half of the patch kernel's arguments (what conv_patch_plan reads); *ph: the rows of a plane of the padded copy
plhip::PatchArgs patch_args(Desc d, Geom g, bool s2, int* ph) {
  int PWp = plhip::conv_patch_row_pitch(d->w, d->pad[2], d->pad[3]), PH = d->h + d->pad[0] + d->pad[1];
  if (s2) patch_s2_dims(d, &PH, &PWp);
  plhip::PatchArgs a;
  memset(&a, 0, sizeof(a));
  a.B = d->n; a.M = d->cout; a.OH = g.oh; a.OW = g.ow;
  a.C = s2 ? 4 * d->cin : d->cin;  // the kernel's channels: stride 2 = (channel, row phase, column phase)
  a.PWp = PWp; a.PLANE = PH * PWp; a.s2 = s2 ? 1 : 0;
  a.act = d->act; a.alpha = d->act_alpha;
  *ph = PH;
  return a;
}
plhip_status run_patch_any(plhip_ctx* ctx, Desc d, Geom g, const ConvIo& io, bool s2) {
  const size_t need = s2 ? patch_s2_input_bytes(d, g) : patch_input_bytes(d, g);
  if (!io.workspace || io.workspace_bytes < need || !aligned(io.workspace, 16))
    return fail(ctx, PLHIP_ERR_WORKSPACE, "plhip_conv2d_int8: padded-input workspace missing, too small or unaligned (16 bytes)");
  int PH;
  plhip::PatchArgs a = patch_args(d, g, s2, &PH);
  const int PWp = a.PWp, CE = a.C;
  plhip::PadArgs pa = pad_args(d, io, d->n * CE, PH, PWp, need);
  pa.tb = plhip::conv_patch_global(PWp) ? d->n : 0;  // planes smaller than a tile: channel-major copy
  pa.tc = CE;
  if (s2) plhip::launch_pad_phase8(pa, ctx->stream);
  else plhip::launch_pad_rows8(pa, ctx->stream);
  LAUNCHCHK(ctx, "pad_rows8");
  a.xp = (const int8_t*)io.workspace; a.wp = (const int8_t*)io.w_packed; a.y = io.y; a.scale = io.scale; a.bias = io.bias;
  set_tail(a, io.tail);
  plhip::launch_conv_patch(a, (int)io.out, ctx->stream);
  LAUNCHCHK(ctx, "conv_patch");
  return PLHIP_OK;
}
plhip_status run_patch(plhip_ctx* ctx, Desc d, Geom g, const ConvIo& io) { return run_patch_any(ctx, d, g, io, false); }
plhip_status run_patch_s2(plhip_ctx* ctx, Desc d, Geom g, const ConvIo& io) { return run_patch_any(ctx, d, g, io, true); }

// ------------------------------------------------------------------ grouped 3x3 (conv_grouped_i8.hip)
// Cg == Mg in {4, 8, 16, 32}, groups >= 4, Cin % 32 == 0, stride 1 | 2: cin / 32 block-diagonal dense 32 -> 32 convs in ONE launch
// on the input itself (no im2col buffer, no padded copy) instead of an im2col launch and one GEMM launch per group
bool takes_grouped3x3(Desc d, Geom) {
  return plhip::conv_grouped3x3_supported(d->cin, d->cout, d->kh, d->kw, d->stride[0], d->stride[1], d->dil[0], d->dil[1], d->groups,
                                          d->pad) &&
         plhip::knob("CONV_GROUPED", 1) != 0;  // knob CONV_GROUPED = 0: A/B runs against the im2col route
}
size_t grouped3x3_packed_bytes(Desc d, Geom) { return plhip::conv_grouped3x3_packed_bytes(d->cin); }
plhip_status pack_grouped3x3(plhip_ctx* ctx, Desc d, Geom, const int8_t* w_oihw, void* w_packed) {
  plhip::launch_pack_conv_grouped3x3(w_oihw, (int8_t*)w_packed, d->cin, d->groups, ctx->stream);
  return PLHIP_OK;
}
plhip_status run_grouped3x3(plhip_ctx* ctx, Desc d, Geom g, const ConvIo& io) {
  if (!aligned(io.w_packed, 16)) return fail(ctx, PLHIP_ERR_INVALID, "plhip_conv2d_int8: packed weights must be 16-byte aligned");
  plhip::GroupedArgs a;
  memset(&a, 0, sizeof(a));
  a.x = io.x; a.wp = (const int8_t*)io.w_packed; a.y = io.y; a.scale = io.scale; a.bias = io.bias;
  a.n = d->n; a.cin = d->cin; a.cout = d->cout; a.h = d->h; a.w = d->w; a.oh = g.oh; a.ow = g.ow;
  a.pt = d->pad[0]; a.pl = d->pad[2]; a.stride = d->stride[0];
  a.act = d->act; a.alpha = d->act_alpha;
  set_tail(a, io.tail);
  if (!plhip::conv_grouped3x3_plan(&a)) return fail(ctx, PLHIP_ERR_UNSUPPORTED, "plhip_conv2d_int8: grouped 3x3 grid too large");
  plhip::launch_conv_grouped3x3(a, (int)io.out, ctx->stream);
  LAUNCHCHK(ctx, "conv_grouped3x3");
  return PLHIP_OK;
}

// ------------------------------------------------------------------ implicit GEMM on a zero-padded copy of the input
// dense k x k convs skip the im2col buffer: 1.08x the input instead of kh*kw x (BASELINE config #2 spent 128 of 149 us writing its
// 57.8 MB im2col buffer)
GemmCall implicit_call(Desc d, Geom g) {
  int PH, PW;
  padded_dims(d, &PH, &PW);
  GemmCall c = {gemm_args(d, g), (g.ow & 3) == 0, true};
  plhip::GemmArgs& a = c.a;
  a.HWX = g.ow;  // an "image" of the column space is one output row
  a.x_bytes = (long)padded_input_bytes(d, g);
  a.NB = d->n * g.oh;
  a.NT = 0;      // the plan's; XP and x_bstride stay 0
  a.im_kw = d->kw; a.im_khkw = d->kh * d->kw; a.im_c = d->cin; a.im_ph = PH; a.im_pw = PW; a.im_oh = g.oh;
  a.im_s = d->stride[0];
  return c;
}
// The route takes what the GEMM plan of its own launch runs on the transposed-read ring kernel (any M > 32, K >= 97, stride 2 on
// a phase-split padded copy: ResNet50's 7x7 stem and its three 3x3 downsampling convs), or -- GEMM_TR = 0 -- what the
// first-generation ring kernel's own thresholds choose.  So run_implicit cannot meet a plan that declines.
bool takes_implicit(Desc d, Geom g) {
  const bool s1 = d->stride[0] == 1 && d->stride[1] == 1, s2 = d->stride[0] == 2 && d->stride[1] == 2;
  if (!(d->groups == 1 && (s1 || s2) && d->dil[0] == 1 && d->dil[1] == 1 && d->kw <= 11 && d->kh * d->kw <= 121 &&
        plhip::knob("IMPLICIT_GEMM", 1) != 0))  // knob IMPLICIT_GEMM = 0: A/B runs against the im2col route
    return false;
  // output rows down to 7 columns (one start-aligned 16-byte chunk per row: the 14x14 and 7x7 planes of ResNet50's last
  // stages); a 1x1 stride-2 conv would use one phase plane of four: it keeps the (strided-copy) im2col route
  if (padded_input_bytes(d, g) >= ((size_t)1 << 31) - 4096 || g.ow < 7 || (s2 && d->kh * d->kw == 1)) return false;
  const GemmCall c = implicit_call(d, g);
  plhip::GemmKnobs kn = plhip::gemm_knobs();
  kn.variant = kn.ma = 0;  // these two pick a kernel for A/B runs; they never moved a conv to another route
  const plhip::GemmPlan p = plhip::gemm_plan(plhip::gemm_problem(c.a, g.MA, plhip::GEMM_OUT_I8, c.vec_store, c.aligned_loads), kn);
  return p.family == plhip::GEMM_TR || (p.family == plhip::GEMM_RING && p.on_merit);
}
plhip_status run_implicit(plhip_ctx* ctx, Desc d, Geom g, const ConvIo& io) {
  const size_t need = padded_input_bytes(d, g);
  if (!io.workspace || io.workspace_bytes < need || !aligned(io.workspace, 4))
    return fail(ctx, PLHIP_ERR_WORKSPACE, "plhip_conv2d_int8: padded-input workspace missing, too small or unaligned");
  int PH, PW;
  padded_dims(d, &PH, &PW);
  plhip::launch_pad_input(pad_args(d, io, d->n * d->cin, PH, PW, need), ctx->stream);
  LAUNCHCHK(ctx, "pad_input");
  GemmCall c = implicit_call(d, g);
  plhip::GemmArgs& a = c.a;
  set_tail(a, io.tail);
  a.wp = (const int8_t*)io.w_packed; a.x = (const int8_t*)io.workspace; a.y = io.y; a.scale = io.scale; a.bias = io.bias;
  if (plhip::launch_gemm_i8(a, g.MA, (int)io.out, c.vec_store && vec_store_ok(io), c.aligned_loads, ctx->stream) != 0)
    return fail(ctx, PLHIP_ERR_UNSUPPORTED, "conv2d: implicit GEMM outside the transposed-read kernel's column space");
  LAUNCHCHK(ctx, "gemm_i8_implicit");
  return PLHIP_OK;
}

// ------------------------------------------------------------------ the route table
const char* name_gemm_1x1(Desc, Geom) { return "conv1x1s1_gemm_int8_mfma32x32x32"; }
const char* name_direct_s2(Desc d, Geom g) {  // one MFMA K-step when the taps fit (Cin <= 3, OW % 4 == 0), v_dot4 otherwise
  return (d->cin * 3 <= 9 && (g.ow & 3) == 0) ? "conv_3x3s2_direct_int8_mfma32x32x32" : "conv_3x3s2_direct_int8_dot4";
}
const char* name_stem7(Desc, Geom) { return "conv_7x7s2_direct_int8_mfma32x32x32"; }
const char* name_patch(Desc, Geom) { return "conv_patch_gemm_int8_mfma32x32x32"; }
const char* name_patch_s2(Desc, Geom) { return "conv_patch_s2_gemm_int8_mfma32x32x32"; }
const char* name_grouped3x3(Desc, Geom) { return "conv_grouped3x3_int8_mfma32x32x32"; }
const char* name_implicit(Desc, Geom) { return "conv_implicit_gemm_int8_mfma32x32x32"; }
const char* name_im2col(Desc, Geom) { return "conv_im2col_gemm_int8_mfma32x32x32"; }

enum ConvImpl { IMPL_GEMM_1X1, IMPL_DIRECT_3X3S2, IMPL_STEM_7X7S2, IMPL_PATCH_GEMM, IMPL_PATCH_S2, IMPL_GROUPED_3X3, IMPL_IMPLICIT_GEMM, IMPL_IM2COL_GEMM };

struct ConvRoute {
  ConvImpl impl;
  bool (*takes)(Desc d, Geom g);
  size_t (*packed_bytes)(Desc d, Geom g);
  size_t (*workspace_bytes)(Desc d, Geom g);
  plhip_status (*pack)(plhip_ctx* ctx, Desc d, Geom g, const int8_t* w_oihw, void* w_packed);
  plhip_status (*run)(plhip_ctx* ctx, Desc d, Geom g, const ConvIo& io);
  const char* (*name)(Desc d, Geom g);
  bool fused_tail;  // run() takes a residual operand / an int8 copy (plhip_conv2d_int8_fused); plhip_conv2d_fused_supported answers from it
};
// In priority order: the first row whose predicate holds runs the conv (the stem kernel wins over patch / implicit; the im2col
// route takes what is left).  Every predicate is a pure function of the descriptor and the knobs.
const ConvRoute kRoutes[] = {
    {IMPL_GEMM_1X1, takes_gemm_1x1, gemm_packed_bytes, no_workspace, pack_gemm, run_gemm_1x1, name_gemm_1x1, true},
    {IMPL_DIRECT_3X3S2, takes_direct_s2, direct_s2_packed_bytes, no_workspace, pack_direct_s2, run_direct_s2, name_direct_s2, false},
    {IMPL_STEM_7X7S2, takes_stem7, stem7_packed_bytes, no_workspace, pack_stem7, run_stem7, name_stem7, true},
    {IMPL_PATCH_GEMM, takes_patch, patch_packed_bytes, patch_input_bytes, pack_patch, run_patch, name_patch, true},
    {IMPL_PATCH_S2, takes_patch_s2, patch_s2_packed_bytes, patch_s2_input_bytes, pack_patch_s2, run_patch_s2, name_patch_s2, true},
    {IMPL_GROUPED_3X3, takes_grouped3x3, grouped3x3_packed_bytes, no_workspace, pack_grouped3x3, run_grouped3x3, name_grouped3x3, true},
    {IMPL_IMPLICIT_GEMM, takes_implicit, gemm_packed_bytes, padded_input_bytes, pack_gemm, run_implicit, name_implicit, true},
    {IMPL_IM2COL_GEMM, takes_im2col, gemm_packed_bytes, im2col_bytes, pack_gemm, run_im2col, name_im2col, true},
};

// the route of a descriptor and its geometry; nullptr: a bad descriptor
const ConvRoute* pick_route(Desc d, ConvGeom* g) {
  if (!conv_geom(d, g)) return nullptr;
  for (const ConvRoute& r : kRoutes)
    if (r.takes(d, *g)) return &r;
  return nullptr;  // (not reached: the last row takes everything)
}

}  // namespace

extern "C" {

// ------------------------------------------------------------------ conv2d
size_t plhip_conv_packed_weight_bytes(const plhip_conv_desc* d) {
  ConvGeom g;
  const ConvRoute* r = pick_route(d, &g);
  return r ? r->packed_bytes(d, g) : 0;
}

plhip_status plhip_pack_conv_weights(plhip_ctx* ctx, const plhip_conv_desc* d, const int8_t* w_oihw, void* w_packed) {
  ConvGeom g;
  if (!ctx || !w_oihw || !w_packed) return fail(ctx, PLHIP_ERR_INVALID, "plhip_pack_conv_weights: null argument");
  const ConvRoute* r = pick_route(d, &g);
  if (!r) return fail(ctx, PLHIP_ERR_INVALID, "plhip_pack_conv_weights: bad conv descriptor");
  if (plhip_status st = r->pack(ctx, d, g, w_oihw, w_packed)) return st;
  LAUNCHCHK(ctx, "pack_weights");
  return PLHIP_OK;
}

size_t plhip_conv_workspace_bytes(const plhip_conv_desc* d) {
  ConvGeom g;
  const ConvRoute* r = pick_route(d, &g);
  return r ? r->workspace_bytes(d, g) : 0;
}

int plhip_conv2d_fused_supported(const plhip_conv_desc* d) {
  ConvGeom g;
  const ConvRoute* r = pick_route(d, &g);
  return r && r->fused_tail ? 1 : 0;
}

const char* plhip_conv_impl_name(const plhip_conv_desc* d) {
  ConvGeom g;
  const ConvRoute* r = pick_route(d, &g);
  return r ? r->name(d, g) : "invalid";
}

// Diagnostics, host only (not in include/plhip.h; paddle-lite_amd/capi.py declares it): the GEMM launch plan (gemm_plan.h) of a
// conv on one of the three GEMM routes, as text, from the route's own argument builder and the knobs in force, assuming aligned
// pointers.  out: the output kind; tail: bit 0 a residual, bit 1 the int8 copy, bit 2 the fp32 output dropped, bit 3 an output or
// residual pointer is off its vector alignment (what vec_store_ok answers for the call's pointers), bit 4 the 1x1 route's x is
// off a dword (what run_gemm_groups answers for its base).  A non-GEMM route answers the
// empty string.  Returns the text's length, or -1 for a bad descriptor or buffer.
int plhip_debug_gemm_plan(const plhip_conv_desc* d, int out, int tail, char* buf, size_t cap) {
  ConvGeom g;
  const ConvRoute* r = pick_route(d, &g);
  if (!r || !buf || cap == 0) return -1;
  buf[0] = 0;
  GemmCall c;
  if (r->impl == IMPL_GEMM_1X1) c = gemm_call(d, g, gemm_b_1x1(d, g), 0);
  else if (r->impl == IMPL_IM2COL_GEMM) c = gemm_call(d, g, gemm_b_im2col(d, g), 0);
  else if (r->impl == IMPL_IMPLICIT_GEMM) c = implicit_call(d, g);
  else return 0;
  const bool x_aligned = r->impl != IMPL_GEMM_1X1 || (tail & 16) == 0;  // (the other two routes read their own workspace copy)
  plhip::GemmProblem p = plhip::gemm_problem(c.a, g.MA, out, c.vec_store && (tail & 8) == 0, c.aligned_loads && x_aligned);
  p.res = (tail & 1) != 0;
  p.y2 = (tail & 2) != 0;
  p.y = (tail & 4) == 0;
  return plhip::gemm_plan_text(plhip::gemm_plan(p, plhip::gemm_knobs()), buf, cap);
}

// Diagnostics, host only: the patch kernel's launch plan (conv_patch_plan, the function launch_conv_patch executes) of a conv on
// one of the two patch routes, as one line of text: the launcher, global mode, tiles, blocks and the LDS pitch.  Another route
// answers the empty string.  Returns the text's length, or -1 for a bad descriptor or buffer.
int plhip_debug_patch_plan(const plhip_conv_desc* d, char* buf, size_t cap) {
  ConvGeom g;
  const ConvRoute* r = pick_route(d, &g);
  if (!r || !buf || cap == 0) return -1;
  buf[0] = 0;
  if (r->impl != IMPL_PATCH_GEMM && r->impl != IMPL_PATCH_S2) return 0;
  int PH;
  plhip::PatchArgs a = patch_args(d, g, r->impl == IMPL_PATCH_S2, &PH);
  const int launcher = plhip::conv_patch_plan(&a);
  return plhip::conv_patch_plan_text(a, launcher, buf, cap);
}

static plhip_status conv2d_impl(plhip_ctx* ctx, const plhip_conv_desc* d, const ConvIo& io) {
  ConvGeom g;
  const bool y_opt = io.tail && io.tail->y_i8;  // the fp32 tensor itself may be dropped when only the int8 copy is consumed
  if (!ctx || !io.x || !io.w_packed || (!io.y && !y_opt)) return fail(ctx, PLHIP_ERR_INVALID, "plhip_conv2d_int8: null argument");
  const ConvRoute* r = pick_route(d, &g);
  if (!r) return fail(ctx, PLHIP_ERR_INVALID, "plhip_conv2d_int8: bad conv descriptor");
  if (plhip_status st = check_out_scale_act(ctx, "plhip_conv2d_int8", io.out, false, io.scale, "scale", &d->act)) return st;
  if ((size_t)d->n * g.Np >= ((size_t)1 << 31) - 256 || (size_t)d->cin * d->h * d->w >= ((size_t)1 << 31) ||
      (size_t)d->cout * g.N >= ((size_t)1 << 31))
    return fail(ctx, PLHIP_ERR_UNSUPPORTED, "plhip_conv2d_int8: tensor too large for 32-bit column index");
  return r->run(ctx, d, g, io);
}

plhip_status plhip_conv2d_int8(plhip_ctx* ctx, const plhip_conv_desc* d, const int8_t* x, const void* w_packed,
                               const float* scale, const float* bias, void* y, plhip_out_kind out, void* workspace,
                               size_t workspace_bytes) {
  return conv2d_impl(ctx, d, ConvIo{x, w_packed, scale, bias, y, out, workspace, workspace_bytes, nullptr});
}

plhip_status plhip_conv2d_int8_fused(plhip_ctx* ctx, const plhip_conv_desc* d, const int8_t* x, const void* w_packed,
                                     const float* scale, const float* bias, float* y_f32, const float* residual,
                                     int residual_relu, int8_t* y_i8, float calib_scale, void* workspace,
                                     size_t workspace_bytes) {
  if (!y_f32 && !y_i8) return fail(ctx, PLHIP_ERR_INVALID, "plhip_conv2d_int8_fused: no output");
  if (y_i8 && !(calib_scale > 0.f)) return fail(ctx, PLHIP_ERR_INVALID, "plhip_conv2d_int8_fused: calib scale must be > 0");
  if (residual_relu && !residual) return fail(ctx, PLHIP_ERR_INVALID, "plhip_conv2d_int8_fused: residual_relu without a residual");
  const ConvTail t{residual, residual_relu, y_i8, calib_scale};
  return conv2d_impl(ctx, d, ConvIo{x, w_packed, scale, bias, y_f32, PLHIP_OUT_F32, workspace, workspace_bytes, &t});
}

// ------------------------------------------------------------------ calib[fp32_to_int8] + conv in one launch
static bool calib_conv_args(const plhip_conv_desc* d, plhip::DirectS2Args* a) {
  ConvGeom g;
  const ConvRoute* r = pick_route(d, &g);
  if (!r || r->impl != IMPL_DIRECT_3X3S2) return false;
  *a = direct_s2_args(d, g);
  return plhip::conv3x3s2_f32in_supported(*a);
}

// The calib and image stems behind their envelope checks.  false: a pointer is misaligned (in: in_align bytes, w_packed: 16, y: 4
// elements); else a's pointers and quantiser are set and *afrag = the MFMA A fragments inside the packed block.
static bool fused_stem_tail(plhip::DirectS2Args* a, const void* in, size_t in_align, float calib_scale, const void* w_packed,
                            const float* scale, const float* bias, void* y, plhip_out_kind out, const int8_t** afrag) {
  if (!aligned(in, in_align) || !aligned(y, 4 * out_elem_size(out)) || !aligned(w_packed, 16)) return false;
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

// ------------------------------------------------------------------ depthwise and the fused depthwise -> 1x1 pairs
// what the plans of dw_plan.h read of a depthwise descriptor (pw_cout, x_aligned: the fused kinds)
static plhip::DwProblem dw_problem(const plhip_conv_desc* d, const ConvGeom& g, int out, int pw_cout = 0, bool x_aligned = true) {
  plhip::DwProblem p{d->n, d->cin, d->h, d->w, g.oh, g.ow, d->kh, d->kw, d->pad[0], d->pad[2], d->stride[0], d->stride[1],
                     d->dil[0], d->dil[1], out};
  p.pw_M = pw_cout;
  p.x_aligned = x_aligned;
  return p;
}

plhip_status plhip_depthwise_conv_int8(plhip_ctx* ctx, const plhip_conv_desc* d, const int8_t* x, const int8_t* w_oihw,
                                       const float* scale, const float* bias, void* y, plhip_out_kind out) {
  ConvGeom g;
  if (!ctx || !x || !w_oihw || !y) return fail(ctx, PLHIP_ERR_INVALID, "plhip_depthwise_conv_int8: null argument");
  if (!conv_geom(d, &g)) return fail(ctx, PLHIP_ERR_INVALID, "plhip_depthwise_conv_int8: bad conv descriptor");
  if (d->groups != d->cin || d->cin != d->cout)
    return fail(ctx, PLHIP_ERR_UNSUPPORTED, "plhip_depthwise_conv_int8: needs groups == cin == cout");
  if (plhip_status st = check_out_scale_act(ctx, "plhip_depthwise_conv_int8", out, false, scale, "scale", &d->act)) return st;
  if (!aligned(y, 4 * out_elem_size(out)) && (g.ow & 3) == 0)
    return fail(ctx, PLHIP_ERR_UNSUPPORTED, "plhip_depthwise_conv_int8: output pointer must be 4-element aligned");
  const plhip::DwPlan p = plhip::depthwise_launch_plan(dw_problem(d, g, (int)out), plhip::dw_knobs());
  if (p.family == plhip::DW_NONE) return fail(ctx, PLHIP_ERR_UNSUPPORTED, "plhip_depthwise_conv_int8: %s", p.why);

  plhip::DwArgs a{};
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
  plhip::launch_depthwise(a, p, (int)out, ctx->stream);
  LAUNCHCHK(ctx, "depthwise_i8");
  return PLHIP_OK;
}

// ------------------------------------------------------------------ fused depthwise -> pointwise (fusion D)
// geometry + launch plan of the fused pair; false: not a depthwise 3x3 the fused kernels take (the caller runs two kernels)
static bool dwpw_plan(const plhip_conv_desc* dw, int pw_cout, plhip_out_kind out, ConvGeom* g, plhip::DwPlan* p, const char** why) {
  *why = "bad depthwise descriptor";
  if (!dw || pw_cout < 1 || !conv_geom(dw, g)) return false;
  *why = "first conv must be depthwise";
  if (dw->groups != dw->cin || dw->cin != dw->cout) return false;
  *why = "tensor too large";
  if ((size_t)pw_cout * g->N >= ((size_t)1 << 31) || (size_t)dw->cin * dw->h * dw->w >= ((size_t)1 << 31)) return false;
  *p = plhip::dwpw_launch_plan(dw_problem(dw, *g, (int)out, pw_cout), plhip::dw_knobs());
  *why = p->why;
  return p->family != plhip::DW_NONE;
}

int plhip_dwpw_fused_supported(const plhip_conv_desc* dw, int pw_cout, plhip_out_kind out) {
  ConvGeom g;
  plhip::DwPlan p;
  const char* why;
  return dwpw_plan(dw, pw_cout, out, &g, &p, &why) ? 1 : 0;
}

plhip_status plhip_dwpw_fused_int8(plhip_ctx* ctx, const plhip_conv_desc* dw, const int8_t* x, const int8_t* dw_w_oihw,
                                   const float* dw_scale, const float* dw_bias, int pw_cout, const void* pw_w_packed,
                                   const float* pw_scale, const float* pw_bias, int pw_act, float pw_alpha, void* y,
                                   plhip_out_kind out) {
  if (!ctx || !dw || !x || !dw_w_oihw || !dw_scale || !pw_w_packed || !y || pw_cout < 1)
    return fail(ctx, PLHIP_ERR_INVALID, "plhip_dwpw_fused_int8: null / bad argument");
  if (plhip_status st = check_out_scale_act(ctx, "plhip_dwpw_fused_int8", out, true, pw_scale, "pw_scale", nullptr)) return st;
  ConvGeom g;
  plhip::DwPlan p;
  const char* why;
  if (!dwpw_plan(dw, pw_cout, out, &g, &p, &why)) return fail(ctx, PLHIP_ERR_UNSUPPORTED, "plhip_dwpw_fused_int8: %s", why);
  plhip::FusedArgs a;
  memset(&a, 0, sizeof(a));
  a.x = x;
  a.dw_w = dw_w_oihw;
  a.dw_scale = dw_scale;
  a.dw_bias = dw_bias;
  a.dw_act = dw->act;
  a.dw_alpha = dw->act_alpha;
  a.n = dw->n; a.C = dw->cin; a.h = dw->h; a.w = dw->w; a.oh = g.oh; a.ow = g.ow;
  a.pt = dw->pad[0]; a.pl = dw->pad[2]; a.stride = dw->stride[0];
  a.pw.M = pw_cout;
  a.pw.K = dw->cin;
  a.pw.KS = cdiv(dw->cin, 32);
  a.pw.HWY = g.N;
  a.pw.y_bstride = (size_t)pw_cout * g.N;
  a.pw.wp = (const int8_t*)pw_w_packed;
  a.pw.y = y;
  a.pw.scale = pw_scale;
  a.pw.bias = pw_bias;
  a.pw.act = pw_act;
  a.pw.alpha = pw_alpha;
  plhip::launch_fused_dwpw(a, p, (int)out, ctx->stream);
  LAUNCHCHK(ctx, "fused_dwpw");
  return PLHIP_OK;
}

// ------------------------------------------------------------------ fused depthwise -> 1x1 conv with the conv's tail (fusion G)
// geometry + launch plan; false: outside the kernel's envelope (the caller runs the two instructions).  Host logic only.
static bool dw_conv1x1_plan(const plhip_conv_desc* dw, int pw_cout, plhip_out_kind out, int has_tail, bool x_aligned, ConvGeom* g,
                            plhip::DwPlan* p, const char** why) {
  *why = "bad depthwise descriptor";
  if (!dw || !conv_geom(dw, g)) return false;
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
  *p = plhip::dw_conv1x1_launch_plan(dw_problem(dw, *g, (int)out, pw_cout, x_aligned), plhip::dw_knobs());
  *why = p->why;
  return p->family != plhip::DW_NONE;
}

int plhip_dw_conv1x1_fused_supported(const plhip_conv_desc* dw, int pw_cout, plhip_out_kind out, int has_tail) {
  ConvGeom g;
  plhip::DwPlan p;
  const char* why;
  return dw_conv1x1_plan(dw, pw_cout, out, has_tail, true, &g, &p, &why) ? 1 : 0;
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
  ConvGeom g;
  plhip::DwPlan p;
  const char* why;
  if (!dw_conv1x1_plan(dw, pw_cout, out, has_tail, aligned(x, 4), &g, &p, &why))
    return fail(ctx, PLHIP_ERR_UNSUPPORTED, "plhip_dw_conv1x1_fused_int8: %s", why);
  if (!y && out != PLHIP_OUT_F32) return fail(ctx, PLHIP_ERR_INVALID, "plhip_dw_conv1x1_fused_int8: y required");
  if (y_i8 && !(calib_scale > 0.f)) return fail(ctx, PLHIP_ERR_INVALID, "plhip_dw_conv1x1_fused_int8: calib scale must be > 0");
  if (residual_relu && !residual) return fail(ctx, PLHIP_ERR_INVALID, "plhip_dw_conv1x1_fused_int8: residual_relu without a residual");
  if (!aligned(pw_w_packed, 16)) return fail(ctx, PLHIP_ERR_INVALID, "plhip_dw_conv1x1_fused_int8: packed weights must be 16-byte aligned");
  plhip::DwConvArgs a;
  memset(&a, 0, sizeof(a));
  a.x = x;
  a.dw_w = dw_w_oihw;
  a.dw_scale = dw_scale;
  a.dw_bias = dw_bias;
  a.dw_act = dw->act;
  a.dw_alpha = dw->act_alpha;
  a.n = dw->n; a.C = dw->cin; a.h = dw->h; a.w = dw->w; a.oh = g.oh; a.ow = g.ow;
  a.pt = dw->pad[0]; a.pl = dw->pad[2]; a.stride = dw->stride[0];
  a.M = pw_cout;
  a.wp = (const int8_t*)pw_w_packed;
  a.y = y;
  a.scale = pw_scale;
  a.bias = pw_bias;
  a.act = pw_act;
  a.alpha = pw_alpha;
  const ConvTail t{residual, residual_relu, y_i8, calib_scale};
  set_tail(a, &t);
  plhip::launch_dw_conv1x1(a, p, (int)out, ctx->stream);
  LAUNCHCHK(ctx, "dw_conv1x1_fused");
  return PLHIP_OK;
}

// Diagnostics, host only: the launch plan (dw_plan.h) of a depthwise conv (kind 0), of a fused depthwise -> pointwise pair (1,
// fusion D) or of a fused depthwise -> 1x1 conv (2, fusion G) as one line of text under the knobs in force, made by the function
// the entry point's launch executes after the entry point's own descriptor checks; a refusal reads "none why=<the error text>".
// Returns the text's length, or -1 for a bad kind or buffer.
int plhip_debug_dw_plan(const plhip_conv_desc* dw, int kind, int pw_cout, int out, int has_tail, int x_aligned, char* buf, size_t cap) {
  if (!buf || cap == 0 || kind < 0 || kind > 2) return -1;
  ConvGeom g;
  plhip::DwPlan p;
  const char* why = "";
  if (kind == 0) {
    if (!dw || !conv_geom(dw, &g)) why = "bad conv descriptor";
    else if (dw->groups != dw->cin || dw->cin != dw->cout) why = "needs groups == cin == cout";
    else why = (p = plhip::depthwise_launch_plan(dw_problem(dw, g, out), plhip::dw_knobs())).why;
  } else if (kind == 1) {
    dwpw_plan(dw, pw_cout, (plhip_out_kind)out, &g, &p, &why);
  } else {
    dw_conv1x1_plan(dw, pw_cout, (plhip_out_kind)out, has_tail, x_aligned != 0, &g, &p, &why);
  }
  if (p.family == plhip::DW_NONE) p.why = why;
  return plhip::dw_plan_text(p, buf, cap);
}

}  // extern "C"
