// plhip_kernels.h — argument blocks and host launchers of the gfx950 kernels (internal to libplhip.so).
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include <type_traits>

#include "deconv_plan.h"
#include "dw_plan.h"
#include "gemm_plan.h"
#include "plhip_device.h"

namespace plhip {

// A/B knobs of the launchers: name -> value set through plhip_debug_set (include/plhip.h), else the
// default.  The library never reads the environment.
int knob(const char* name, int dflt);
#ifdef PLHIP_EXPERIMENTS
// timeline stamps (plhip_device.h): the stamp buffer of `family` ("gemm", "tr", "wide", "patch", "fw", "fs", "f7"), allocated
// on first use with `bytes`, when plhip_debug_set("STAMPS", 1) is in force; else nullptr
unsigned long long* stamp_buffer(const char* family, size_t bytes);
#define PLHIP_SET_STAMPS(args, family, bytes) ((args).stamps = ::plhip::stamp_buffer(family, bytes))
#else
#define PLHIP_SET_STAMPS(args, family, bytes) ((void)0)
#endif

struct GemmArgs {
  const int8_t* wp;    // packed weights of this group: [MT32][KS][64][16]
  const int8_t* x;     // B operand base for this group: row k of image b at x + b*x_bstride + k*HWX
  void* y;             // output base for this group: row m of image b at y + (b*y_bstride + m*HWY) elements
  const float* scale;  // [M] folded per-channel scale (unused for I32)
  const float* bias;   // [M] folded bias or nullptr
  int M, K, KS;        // rows, reduction length, K-steps of 32
  int HWX, HWY;        // columns per image in n-space (multiple of 4) / valid columns per image in y (= y row pitch)
  int XP;              // x row pitch in bytes (HWX for the im2col buffer, HW for a dense NCHW slab)
  long x_bytes;        // bytes readable from x (guards the last partial dword when XP % 4 != 0)
  int NB;              // images
  size_t x_bstride, y_bstride;
  int MT, NT;          // wave tiles along M (32*MA rows) and N (128 columns)
  int act;
  float alpha;
  // fused graph tail of an fp32-output conv (OUT_F32 only; all optional, zero = plain conv):
  //   v = act(fma(acc, s, b));  if (res) v = v + res[same offset];  if (res_relu) v = max(v, 0);
  //   if (y) y = v;  if (y2) y2 = round_sat_i8(v * inv_scale2)          (calib, type_trans.cc:45,183-184)
  // i.e. conv2d[fp32_out] -> elementwise_add / fusion_elementwise_add_activation -> calib of the reference program
  // in one launch, every value rounded exactly as the three instructions round it.  y may be nullptr when y2 is set.
  const float* res;
  int res_relu;
  int8_t* y2;
  float inv_scale2;
  // implicit GEMM (dense kh x kw, stride 1, dilation 1) on a zero-PADDED copy of the input [b][c][PH][PW]: im_kw > 0.
  // Then an "image" of the column space is one output row (NB = batch * OH, HWX = OW) and K-row k = (c, r, s) of it
  // starts at  x + ((b*C + c)*PH + oh + r)*PW + s : contiguous bytes, so the B tile still moves as 16-byte pieces.
  int im_kw, im_khkw, im_c, im_ph, im_pw, im_oh;
  // stride of the implicit conv (1 or 2; transposed-read kernel only).  Stride 2: the padded copy is PHASE-SPLIT, plane
  // (c, p, q) holds padded[c][2y + p][2x + q] (im_ph x im_pw each), so that tap (r, s) of output (oh, ow) is byte
  // ((c*4 + (r&1)*2 + (s&1)) * im_ph + oh + (r>>1)) * im_pw + ow + (s>>1): contiguous in ow again.
  int im_s;
  // wide-tile kernel (gemm_wide_i8.hip): fastdiv_u31's (magic, shift) for the chunks per image, set by its launcher
  unsigned cpi_m;
  int cpi_s;
#ifdef PLHIP_EXPERIMENTS
  unsigned long long* stamps;  // timeline stamp buffer of the launch, or nullptr
#endif
};

struct PadArgs {
  const int8_t* x;  // [planes][h][w]
  int8_t* xp;       // [planes][ph][pw] + slack, zero border; stride 2: [planes][2][2][ph][pw] phase planes
  int planes, h, w, ph, pw, pt, pl;
  int stride;       // 1, or 2 = phase-split copy (ph, pw are then the phase plane's dims)
  int tb, tc;       // pad_rows8 only, tb > 0: CHANNEL-major output: plane c * tb + b of xp <- plane b * tc + c of x
  long total;       // bytes of xp to write (multiple of 4: planes*ph*pw rounded up + slack)
  // exact division of a 31-bit index by ph*pw and by pw without a divide sequence (launch_pad_input fills them; same
  // (magic, shift) form as DwArgs: magic == 0 -> power of two)
  unsigned div_plane_m, div_pw_m, div_pwq_m, div_ph_m;  // pwq = pw / 4 and ph: the phase-split copy's divisors
  int div_plane_s, div_pw_s, div_pwq_s, div_ph_s;
};
void launch_pad_input(const PadArgs& a, hipStream_t s);
void launch_pad_rows8(PadArgs a, hipStream_t s);  // conv_patch_i8.hip: rows of pw % 8 == 0 bytes, 16 bytes per thread

// dense 3x3 stride-1 convolution on input patches (conv_patch_i8.hip)
struct PatchArgs {
  const int8_t* xp;    // zero-padded copy [B][C][PH][PWp] (+ slack): padded[ih + pt][iw + pl] = x[ih][iw]
  const int8_t* wp;    // packed weights [MT32][NCH][3 s][3 r][64 lanes][16 B] (launch_pack_conv_patch)
  void* y;             // [B][M][OH][OW] int8 / fp32 / int32 (may be nullptr with y2)
  const float* scale;  // [M] folded per-channel scale (unused for I32)
  const float* bias;   // [M] or nullptr
  int B, C, M, OH, OW;
  int PWp, PLANE;      // row pitch (multiple of 8) and plane size PH * PWp of the padded copy
  int NCH;             // 32-channel chunks: C / 32
  int pitch, pps;      // LDS bytes per channel row of a slab (odd multiple of 32, >= tile + 2 PWp), pitch / 32
  int TPI, T, T8;      // tiles per image, tiles in all, tiles per XCD (ceil(T / 8))
  int MB, NQ, rounds;  // M blocks, blocks per XCD and M block, tiles per stream
  int HWY;             // OH * OW
  size_t y_bstride;    // M * OH * OW
  int act;
  float alpha;
  unsigned pw_m, tpi_m, pitch_m;  // fastdiv_u31 (magic, shift) for PWp, TPI, pitch
  int pw_s, tpi_s, pitch_s;
  // fused tail of an fp32-output conv (OUT_F32 only), as GemmArgs
  const float* res;
  int res_relu;
  int8_t* y2;
  float inv_scale2;
  // global mode (planes smaller than a tile: 7-wide): the padded copy is [c][image][PH][PWp], p runs over all images
  int s2;              // 3x3 stride 2 as a 2x2 conv over phase planes: C = 4 Cin, the slabs are walked with 2 taps per side
  int glob, nimg, IMGP;  // nimg = the real image count; IMGP = PH * PWp pixels per image (PLANE is then the CHANNEL stride B * IMGP, B = 1, TPI = T)
  unsigned imgp_m, hwy_m;
  int imgp_s, hwy_s;
#ifdef PLHIP_EXPERIMENTS
  unsigned long long* stamps;  // as GemmArgs::stamps
#endif
};
// row pitch of the padded copy for (w, pl, pr), 0 = outside the route
int conv_patch_row_pitch(int w, int pl, int pr);
bool conv_patch_global(int pwp);  // planes smaller than a tile: channel-major padded copy, p across images
bool conv_patch_supported(int cin, int cout, int kh, int kw, int sh, int sw, int dh, int dw, int groups, int w, int pl, int pr);
size_t conv_patch_packed_bytes(int cin, int cout);
void launch_pack_conv_patch(const int8_t* w_oihw, int8_t* wp, int cin, int cout, hipStream_t s);
// the launch plan of `a` (B, C, M, OH, OW, PWp, PLANE, s2 set by the caller): fills the plan's fields, returns the launcher
enum PatchLauncher { PATCH_STAT_A = 0, PATCH_STAT_B, PATCH_STREAM_A, PATCH_S2 };
int conv_patch_plan(PatchArgs* a);
int conv_patch_plan_text(const PatchArgs& a, int launcher, char* buf, size_t cap);  // one line of text
// makes the plan of `a` and launches it
void launch_conv_patch(PatchArgs a, int out, hipStream_t s);
void launch_patch_stat_a(const PatchArgs& a, int out, hipStream_t s);    // per-variant translation units
void launch_patch_stat_b(const PatchArgs& a, int out, hipStream_t s);
void launch_patch_stream_a(const PatchArgs& a, int out, hipStream_t s);
void launch_patch_s2(const PatchArgs& a, int out, hipStream_t s);
int conv_patch_s2_row_pitch(int w, int pl, int pr);
bool conv_patch_s2_supported(int cin, int cout, int kh, int kw, int sh, int sw, int dh, int dw, int groups, int w, int pl, int pr);
size_t conv_patch_s2_packed_bytes(int cin, int cout);
void launch_pack_conv_patch_s2(const int8_t* w_oihw, int8_t* wp, int cin, int cout, hipStream_t s);
void launch_pad_phase8(PadArgs a, hipStream_t s);

// grouped 3x3 convolution, Cg == Mg in {4, 8, 16, 32}, Cin % 32 == 0, stride 1 | 2 (conv_grouped_i8.hip)
struct GroupedArgs {
  const int8_t* x;     // [n][cin][h][w]: the kernel stages its rows itself, zero borders included
  const int8_t* wp;    // packed weights [cin / 32 chunks][9 taps][64 lanes][16 B], block-diagonal (launch_pack_conv_grouped3x3)
  void* y;             // [n][cout][oh][ow] int8 / fp32 / int32 (may be nullptr with y2)
  const float* scale;  // [cout] folded per-channel scale (unused for I32)
  const float* bias;   // [cout] or nullptr
  int n, cin, cout, h, w, oh, ow, pt, pl, stride;
  int act;
  float alpha;
  // fused tail of an fp32-output conv (OUT_F32 only), as GemmArgs
  const float* res;
  int res_relu;
  int8_t* y2;
  float inv_scale2;
  // launch plan (conv_grouped3x3_plan): 32-channel chunks; a block = TR output rows x CWq column quads of one (image, chunk);
  // bands of TR rows and segments of CWq quads per plane; staged input rows IR of 4 * stride * WQ pixels; bytes between the LDS
  // images of channels 0..15 and 16..31; LDS bytes
  int NCH, TR, CWq, bands, nseg, IR, WQ, half;
  unsigned nblocks, nblocks_per_xcd;
  size_t lds;
};
bool conv_grouped3x3_supported(int cin, int cout, int kh, int kw, int sh, int sw, int dh, int dw, int groups, const int pad[4]);
size_t conv_grouped3x3_packed_bytes(int cin);
void launch_pack_conv_grouped3x3(const int8_t* w_oihw, int8_t* wp, int cin, int groups, hipStream_t s);
// fills the plan from (n, cin, oh, ow, stride); false = more blocks than a grid holds
bool conv_grouped3x3_plan(GroupedArgs* a);
void launch_conv_grouped3x3(const GroupedArgs& a, int out, hipStream_t s);

// conv2d_transpose (deconv_i8.hip): the MFMA phase kernel and the direct kernel share the argument block
struct DeconvArgs {
  const int8_t* x;     // [n][cin][h][w]: the phase kernel stages its rows itself, zero borders included
  const int8_t* wp;    // phase: packed A fragments [cout / 32 M tiles][cin / 32 chunks][kh * kw taps][64 lanes][16 B]
                       // (launch_pack_deconv_phase); direct: the filter itself, [cin][cout / groups][kh][kw]
  void* y;             // [n][cout][oh][ow] int8 / fp32 / int32
  const float* scale;  // [cout] folded per-channel scale (unused for I32)
  const float* bias;   // [cout] or nullptr
  int n, cin, cout, h, w, oh, ow, kh, kw, pt, pl, sh, sw, dh, dw, groups;
  int act;
  float alpha;
  // launch plan of the phase kernel (deconv_phase_plan, deconv_plan.h; launch_deconv_phase's caller copies it in)
  int NCH, MT, TY, TX, NV, NUq, TR, CWq, bands, nseg, IR, WQ, half;
  unsigned nblocks, nblocks_per_xcd;
  size_t lds;
};
void launch_pack_deconv_phase(const int8_t* w_iohw, int8_t* wp, const DeconvProblem& p, hipStream_t s);
void launch_deconv_phase(const DeconvArgs& a, int out, hipStream_t s);
void launch_deconv_direct(const DeconvArgs& a, int out, hipStream_t s);

struct Im2colArgs {
  const int8_t* x;
  int8_t* col;
  int cin, cin_g, h, w, kh, kw, pt, pl, sh, sw, dh, dw, oh, ow;
  int G, Kg, N, Np;
  size_t rows;  // B*G*Kg
};

struct DwArgs {
  const int8_t* x;
  const int8_t* wt;  // [C][kh*kw]
  void* y;
  const float* scale;
  const float* bias;
  int planes, C, h, w, oh, ow, kh, kw, pt, pl, sh, sw, dh, dw;
  // launch plan (depthwise_launch_plan, dw_plan.h; launch_depthwise copies it in).  LDS-band kernel:
  int PB;       // planes per block
  int OB;       // output rows per block band
  int bands;    // bands per plane
  int in_rows;  // staged input rows per band
  int pitch;    // LDS row pitch in bytes (multiple of 4)
  long total_lanes;               // direct kernel: planes * strips * quads
  int owq_log2, spp_log2, fast_div;  // direct kernel: power-of-two index split
  // exact division of a 31-bit index by a run-time constant without a divide: q = d is a power of two ? n >> sh
  // : mulhi(n, magic) >> sh  (magic = floor(2^(31+s)/d) + 1, s = ceil(log2 d), sh = s - 1; exact for n < 2^31)
  unsigned div_owq_m, div_spp_m, div_c_m;
  int div_owq_s, div_spp_s, div_c_s;
  int stage_bytes;                // direct kernel: LDS bytes per wave for output staging (0 = off)
  int lw, nblocks;                // direct kernel: lanes of a wave that own work (staging: whole strips), workgroups of work
  int act;
  float alpha;
  // direct kernels: the int8 clamp's upper bound on doubled values (relu6: min(2 alpha, 254); follows the activation, so the
  // launcher sets it, not the plan) and the byte-wise +1 of the packed rounding, as kernel arguments = scalar operands (the
  // compiler re-made both per output row)
  float hi2 = 254.f;
  unsigned ones = 0x01010101u;
};

// fused depthwise 3x3 (int8 out) -> pointwise 1x1 (fused_dwpw_i8.hip)
struct FusedArgs {
  const int8_t* x;        // [n, C, h, w]
  const int8_t* dw_w;     // [C, 1, 3, 3]
  const float* dw_scale;  // folded depthwise scale / bias (int8-out folding), per channel
  const float* dw_bias;   // or nullptr
  int dw_act;
  float dw_alpha;
  int n, C, h, w, oh, ow, pt, pl, stride;
  // launch plan (dwpw_launch_plan, dw_plan.h; launch_fused_dwpw copies it in): tiles = blocks of work: (image, half-plane) = 2 n
  // on the 14 x 14 kernel, n * pw.NT row tiles on the streaming kernel (pw.NT = tiles per image), n * MB on the 7 x 7 kernel
  int tiles;
  unsigned ones;          // 0x01010101 as a scalar operand (the byte-wise +1 of the packed rounding); launch_fused_dwpw sets it
  int unused_;            // no kernel reads it (once the kernel selector, now DwPlan::family); it keeps the argument block's layout
  GemmArgs pw;            // wp, y, scale, bias, M, KS, HWY (= oh*ow), y_bstride, act, alpha
};

// fused depthwise 3x3 (int8 out) -> 1x1 conv with the conv's graph tail (fused_dwconv_i8.hip, fusion G)
struct DwConvArgs {
  const int8_t* x;        // [n, C, h, w]
  const int8_t* dw_w;     // [C, 1, 3, 3]
  const float* dw_scale;  // folded depthwise scale / bias (int8-out folding), per channel
  const float* dw_bias;   // or nullptr
  int dw_act;
  float dw_alpha;
  int n, C, h, w, oh, ow, pt, pl, stride;
  int M;                  // 1x1 conv output channels
  const int8_t* wp;       // its weights as plhip_pack_conv_weights packs them: [MT32][KS][64][16]
  void* y;                // [n, M, oh, ow] of the output kind (fp32: may be nullptr when y2 is set)
  const float* scale;     // [M] folded scale (unused for I32)
  const float* bias;      // [M] or nullptr
  int act;
  float alpha;
  const float* res;       // fp32 tail, as GemmArgs: residual (+ relu), calib copy y2 = round_sat_i8(v * inv_scale2)
  int res_relu;
  int8_t* y2;
  float inv_scale2;
  // launch plan (dw_conv1x1_launch_plan, dw_plan.h; launch_dw_conv1x1 copies it in): K-steps of 32 channels; 32-row m tiles in all / per block (grid.y = m groups); tile = TR
  // output rows x CW columns of one image (CW = ow, or 128-column segments of wider rows) = NT 32-pixel n tiles; tiles per
  // image (tr_tiles x cw_tiles); staged input rows IR of WP bytes (LDS column = input column - CW-segment start + 4); stage
  // units per row (dwords when w % 4 == 0 and x sits on 4 bytes, else bytes) and rows per wave pass; accumulators per wave; LDS bytes
  int KS, mt32, mtpb, mgroups, TR, CW, NT, tr_tiles, cw_tiles, tpi, IR, WP, dword_stage, wu, rpp, nacc;
  unsigned ir_m, owq_m, tr_m, cw_m, tpi_m, ctl_m;  // fastdiv_u31 (magic, shift) for IR, CW / 4 quads, TR, CW, tpi, cw_tiles
  int ir_s, owq_s, tr_s, cw_s, tpi_s, ctl_s;
  size_t lds;
};

// ---- the GEMM kernels.  gemm_plan (gemm_plan.h) decides the whole launch; the three files below only execute a plan.
inline GemmProblem gemm_problem(const GemmArgs& g, int ma, int out, bool vec_store, bool aligned_loads) {
  return GemmProblem{g.M, g.K, g.KS, g.HWX, g.HWY, g.XP, g.NB, g.im_kw, g.im_s, g.res != nullptr, g.y2 != nullptr, g.y != nullptr,
                     out, ma, vec_store, aligned_loads};
}
// the knobs the plan reads, the two ways to force the wide tile resolved (gemm_i8.hip).  Host only.
GemmKnobs gemm_knobs();
void debug_set_wide_ntt(int v);  // plhip_debug_wide_ntt: 4 / 7 / 8 force that tile, 0 = automatic, -1 = back to the knob WIDE_NTT
int gemm_tr_stamp_lds();         // LDS bytes of the timeline stamps (EXPERIMENTS=1 builds, else 0)
int gemm_wide_stamp_lds();
// plans and launches; 0, or -3 when the operand exists on one kernel only and that kernel declines it (nothing is launched)
int launch_gemm_i8(const GemmArgs& g, int ma, int out, bool vec_store, bool aligned_loads, hipStream_t s);
// executors: g carries the plan's HWX / MT / NT already
void run_gemm_tr(const GemmPlan& p, GemmArgs g, hipStream_t s);    // gemm_tr_i8.hip
void run_gemm_wide(const GemmPlan& p, GemmArgs g, hipStream_t s);  // gemm_wide_i8.hip
void launch_wide_n4(const GemmPlan& p, const GemmArgs& g, hipStream_t s);  // per-tile translation units (gemm_wide_n*.hip)
void launch_wide_n7(const GemmPlan& p, const GemmArgs& g, hipStream_t s);
void launch_wide_n8(const GemmPlan& p, const GemmArgs& g, hipStream_t s);
// A run-time value as a template argument: calls f(std::integral_constant<int, V>{}) for the V of Vs... that equals v (bools
// as 0 / 1); false when none does.  Only the listed values are instantiated.
template <int... Vs, class F>
inline bool with_const(int v, F&& f) {
  return ((v == Vs ? (f(std::integral_constant<int, Vs>{}), true) : false) || ...);
}
void launch_pack_weights(const int8_t* w, int8_t* wp, int G, int Mg, int Kg, int MT32, int KS, hipStream_t s);
void launch_im2col(const Im2colArgs& a, hipStream_t s);

// ---- the depthwise and fused depthwise -> 1x1 kernels.  The three plan functions of dw_plan.h decide the whole launch; the five
// files below only execute a plan: they copy its fields into the argument block and pick the instance it names.
DwKnobs dw_knobs();  // the knobs the plans read (depthwise_i8.hip).  Host only.
void launch_depthwise(const DwArgs& a, const DwPlan& p, int out, hipStream_t s);        // depthwise_i8.hip
void launch_fused_dwpw(const FusedArgs& a, const DwPlan& p, int out, hipStream_t s);    // fused_dwpw_i8.hip: every dwpw_* plan
void run_fused_stream(const DwPlan& p, FusedArgs a, int out, hipStream_t s);            // fused_dwpw_stream.hip
void run_fused_small(const DwPlan& p, FusedArgs a, int out, hipStream_t s);             // fused_dwpw_small.hip
void launch_dw_conv1x1(const DwConvArgs& a, const DwPlan& p, int out, hipStream_t s);   // fused_dwconv_i8.hip
// fusion D's kernels: raises the kernel's dynamic-LDS limit to the plan's bytes and launches it on the plan's grid
template <class Kernel, class Args>
inline void launch_max_lds(Kernel kfn, const DwPlan& p, hipStream_t s, const Args& a) {
  (void)hipFuncSetAttribute((const void*)kfn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)p.lds);
  hipLaunchKernelGGL(kfn, dim3(p.grid_x), dim3(p.block), p.lds, s, a);
}
// fusion D's instance split that no plan decides: calls f(OUT, DWNN, PWNN) as integral constants: OUT = `out` of Outs...; DWNN: the
// depthwise activation is relu / relu6 (its int8 values are non-negative); PWNN: so is the pointwise one and the output is int8
template <int... Outs, class F>
inline void with_out_nonneg(int out, int dw_act, int pw_act, F&& f) {
  const bool dwnn = dw_act == ACT_RELU || dw_act == ACT_RELU6;
  const bool pwnn = out == OUT_I8 && (pw_act == ACT_RELU || pw_act == ACT_RELU6);
  with_const<Outs...>(out, [&](auto o) {
    with_const<0, 1>(dwnn, [&](auto dn) { with_const<0, 1>(pwnn, [&](auto pn) { f(o, dn, pn); }); });
  });
}

// direct 3x3 stride-2 convolution for small Cin (network stems)
struct DirectS2Args {
  const int8_t* x;
  const uint32_t* wp;  // packed [cin*3 + r][coutp] dwords (w0, w1, w2, 0)
  void* y;
  const float* scale;
  const float* bias;
  int n, cin, h, w, cout, coutp, oh, ow, pt, pl;
  int act;
  float alpha;
  // fused tail of an fp32-output conv (the 7x7 stem only), as GemmArgs
  const float* res = nullptr;
  int res_relu = 0;
  int8_t* y2 = nullptr;
  float inv_scale2 = 0.f;
  // fused calib[fp32_to_int8] in front (conv_stem_f32in.hip): the fp32 image and 1 / its quantisation scale
  const float* xf = nullptr;
  float x_inv_scale = 0.f;
};
// conv_stem7_i8.hip: 7x7 stride 2, Cin <= 3 (ResNet50's stem); wp = its A fragments
bool conv7x7s2_stem_supported(int cin, int cout, int kh, int kw, int sh, int sw, int dh, int dw, int groups, int n, int h, int w,
                              int oh, int ow, int pl);
size_t conv7x7s2_stem_packed_bytes(int cout);
void launch_pack_conv7x7s2_stem(const int8_t* w_oihw, int8_t* wp, int cin, int cout, hipStream_t s);
void launch_conv7x7s2_stem(const DirectS2Args& a, int out, bool vec_store, hipStream_t s);
bool conv3x3s2_direct_supported(int cin, int cout, int kh, int kw, int sh, int sw, int dh, int dw, int groups, int pl);
size_t conv3x3s2_direct_packed_bytes(int cin, int cout);
void launch_pack_conv3x3s2_direct(const int8_t* w_oihw, uint32_t* wp, int cin, int cout, hipStream_t s);
void launch_conv3x3s2_direct(const DirectS2Args& a, int out, hipStream_t s);
size_t conv3x3s2_dot4_bytes(int cin, int cout);              // offset of the MFMA A fragments inside the packed block
bool conv3x3s2_f32in_supported(const DirectS2Args& a);      // conv_stem_f32in.hip: calib[fp32_to_int8] + this conv in one launch
void launch_conv3x3s2_f32in(const DirectS2Args& a, const int8_t* afrag, int out, hipStream_t s);

// uint8 interleaved image [n, h, w, cs] (cs 1 / 3 / 4) -> c = (cs == 1 ? 1 : 3) normalised channels (image_to_tensor.hip)
struct ImageArgs {
  const uint8_t* src;
  int n, h, w, cs, c;
  float mean[3], scale[3];  // indexed by the source byte of the pixel (image2tensor.cc:279-284)
};
void launch_image_to_tensor_f32(const ImageArgs& a, float* y, hipStream_t s);
void launch_image_to_tensor_i8(const ImageArgs& a, int8_t* y, float calib_scale, hipStream_t s);
// conv_stem_u8in.hip: image_to_tensor + calib[fp32_to_int8] + the 3x3 stride-2 stem in one launch; a.x_inv_scale = 1 / calib scale
bool conv3x3s2_u8in_supported(const DirectS2Args& a, const ImageArgs& im);
void launch_conv3x3s2_u8in(const DirectS2Args& a, const ImageArgs& im, const int8_t* afrag, int out, hipStream_t s);

// NV12 / NV21 frame [n][h * 3 / 2][w] -> interleaved BGR / BGRA [n, h, w, 3 | 4] (image_convert.hip); w, h even
struct NvArgs {
  const uint8_t* src;
  int n, h, w;
  int nv21;  // chroma pair order: 0 = (u, v) NV12, 1 = (v, u) NV21
};
void launch_nv_to_bgr(const NvArgs& a, uint8_t* y, int dst_cs, hipStream_t s);
#ifdef __HIPCC__
// one pixel of image_convert.cc:451-514: p = {b, g, r}.  Shared by the convert kernel and the fused frame kernel, so that a tap
// converted while it is fetched is the converted image's byte, bit for bit.
__device__ __forceinline__ void nv_pixel_bgr(int y, int u, int v, int (&p)[3]) {
  const int ra = (179 * (v - 128)) >> 7, ga = (44 * (u - 128) + 91 * (v - 128)) >> 7, ba = (227 * (u - 128)) >> 7;
  const int b = y + ba, g = y - ga, r = y + ra;
  p[0] = b < 0 ? 0 : (b > 255 ? 255 : b);
  p[1] = g < 0 ? 0 : (g > 255 ? 255 : g);
  p[2] = r < 0 ? 0 : (r > 255 ? 255 : r);
}
#endif

// bilinear resize of a frame (image_resize.hip): interleaved [n, h_in, w_in, cs] or (nv != 0) an NV12 / NV21 frame converted tap
// by tap (cs = 3, b g r) -> the uint8 image [n, h_out, w_out, cs], or the normalised NCHW tensor made from it (fp32 / int8)
struct ResizeArgs {
  const uint8_t* src;
  int n, h_in, w_in, h_out, w_out;
  int cs;  // bytes per pixel of the image that is resized: 1 / 3 / 4
  int nv;  // 0 = interleaved source, 1 = NV12, 2 = NV21
  // host-made tables in device memory (plhip_image_resize_tables): per output column source column and (a0, a1), per output row
  // source row and (b0, b1)
  const int32_t* xofs;
  const int16_t* xcoef;
  const int32_t* yofs;
  const int16_t* ycoef;
  float mean[3], scale[3];  // tensor forms: as ImageArgs
};
enum { RESIZE_OUT_U8 = 0, RESIZE_OUT_F32 = 1, RESIZE_OUT_I8 = 2 };
// y: uint8 [n, h_out, w_out, cs] | fp32 / int8 NCHW [n, cs == 1 ? 1 : 3, h_out, w_out]; calib_scale: RESIZE_OUT_I8 only
void launch_image_resize(const ResizeArgs& a, void* y, int out, float calib_scale, hipStream_t s);

size_t fc_packed_bytes(int k, int n);
void launch_pack_fc(const int8_t* w_kn, int8_t* wp, int k, int n, hipStream_t s);
void launch_fc(const int8_t* x, const int8_t* wp, const float* scale, const float* bias, void* y, int m, int k, int n,
               int relu, int out, hipStream_t s);
void launch_calib_f32_to_i8(const float* x, int8_t* y, float scale, int64_t count, hipStream_t s);
void launch_calib_i8_to_f32(const int8_t* x, float* y, float scale, int64_t count, hipStream_t s);
void launch_global_avg_pool(const float* x, int nc, int spatial, float* y, hipStream_t s);
void launch_softmax(const float* x, int rows, int cols, float* y, hipStream_t s);

// fp32 window pooling (max / avg) and elementwise add (+relu): eltwise_pool.hip
struct PoolArgs {
  const float* x;  // [planes][h][w]
  float* y;        // [planes][oh][ow]
  int planes, h, w, oh, ow, kh, kw, sh, sw, pt, pb, pl, pr;
  int is_max, exclusive;
};
void launch_pool2d(const PoolArgs& a, hipStream_t s);
void launch_pool2d_max_i8(const PoolArgs& a, hipStream_t s);  // x / y are int8 planes behind the float pointers
void launch_eltwise_add(const float* x, const float* y, float* o, int64_t count, int relu, hipStream_t s);

// hard_swish / hard_sigmoid and the squeeze-excite multiply, fp32 in, fp32 and / or int8 (calib form) out: hard_act.hip
enum { HARD_ACT_SWISH = 0, HARD_ACT_SIGMOID = 1 };
// params: hard_swish {threshold, scale, offset}, hard_sigmoid {slope, offset}; yf / yq: either may be null
void launch_hard_act(int kind, const float* params, const float* x, float* yf, int8_t* yq, float calib_scale, int64_t count,
                     hipStream_t s);
// out[p][i] = x[p][i] * g[p], p < planes, i < hw
void launch_se_scale(const float* x, const float* g, float* yf, int8_t* yq, float calib_scale, int64_t planes, int hw, hipStream_t s);

// the excite stage of a squeeze-excite block in one launch: se_gate.hip
constexpr int SE_GATE_MAX_C = 960;
struct SeGateArgs {
  const float* pooled;   // [n][c]
  float inv;             // 1 / calib scale
  const uint32_t* w1;    // packed [(c + 3) / 4][cr]
  const uint32_t* w2;    // packed [(cr + 3) / 4][c]
  const float *s1, *b1;  // folded scale / bias of conv 1 [cr] (b may be null)
  const float *s2, *b2;  // ... of conv 2 [c]
  int act1, act2;
  float alpha1, alpha2;
  float slope, offset;   // hard_sigmoid
  float* gate;           // [n][c]
  int c, cr;
};
size_t se_gate_packed_bytes(int c, int cr);
void launch_se_gate_pack(const int8_t* w1, const int8_t* w2, void* packed, int c, int cr, hipStream_t s);
void launch_se_gate(const SeGateArgs& a, int n, hipStream_t s);

// concat / split / shuffle_channel and the one-launch tail of a ShuffleNetV2 unit, fp32 moves (int8: the calib form): shuffle_ops.hip
constexpr int CONCAT_MAX_PARTS = 8;  // operand pointers of one launch (they travel in the argument struct)
struct ConcatArgs {
  float* part[CONCAT_MAX_PARTS];    // [outer][len[p]]; read by concat, written by split
  int64_t len[CONCAT_MAX_PARTS];    // c_p * inner floats
  int64_t off[CONCAT_MAX_PARTS];    // where part p's row starts inside a row of `whole`
  float* whole;                     // [outer][stride]
  int64_t stride, outer;
  int vec;
};
// parts[i]: [outer][extents[i]][inner]; whole: [outer][sum extents][inner]; split != 0 copies whole -> parts.  One launch per
// CONCAT_MAX_PARTS parts.
void launch_concat_split(float* const* parts, const int64_t* extents, int count, int64_t outer, int64_t inner, float* whole, int split,
                         hipStream_t s);
// concat -> calib[fp32_to_int8] in one launch per CONCAT_MAX_PARTS parts: yq the int8 tensor, yf (may be null) the fp32 one
struct ConcatCalibArgs {
  const float* part[CONCAT_MAX_PARTS];  // [outer][len[p]]
  int64_t len[CONCAT_MAX_PARTS];        // c_p * inner floats
  int64_t off[CONCAT_MAX_PARTS];        // where part p's row starts inside an output row
  float* yf;                            // [outer][stride] or null
  int8_t* yq;                           // [outer][stride]
  int64_t stride, outer;
  float inv;                            // 1 / calib scale
};
void launch_concat_calib(const float* const* parts, const int64_t* extents, int count, int64_t outer, int64_t inner, float* yf,
                         int8_t* yq, float calib_scale, hipStream_t s);
// out[b][j * group + i] = in[b][i * (c / group) + j]; yf / yq: either may be null
void launch_shuffle_channel(const float* x, float* yf, int8_t* yq, float calib_scale, int n, int c, int hw, int group, hipStream_t s);
// shuffled channel c' = 2 j + side of (side ? b : a) [n][h][hw]: c' < split_at -> lo [n][split_at][hw], else hf / hq [n][2 h - split_at][hw]
void launch_shuffle_unit(const float* a, const float* b, float* lo, float* hf, int8_t* hq, float calib_scale, int n, int h, int hw,
                         int split_at, hipStream_t s);

// bilinear_interp / nearest_interp of fp32 NCHW planes, arg_max along an axis, and interp -> arg_max(axis 1) in one launch: interp_ops.hip
struct InterpArgs {
  const float* x;   // [planes][ih][iw]
  int ih, iw, oh, ow;
  float ry, rx;     // the source step per output index of each axis (an fp32 division, done on the host)
  int bilinear;     // 0: one source pixel (nearest_interp, and the copy that in == out on both axes is)
  int half;         // bilinear: f = r * (l + 0.5) - 0.5 clamped at 0 (align_mode 0 without align_corners); else f = l * r
  int round_up;     // nearest: (int)(double(r * l) + 0.5) (align_corners); else (int)(r * l)
};
// method 0 bilinear / 1 nearest; the ratios and the coordinate rule of (align_corners, align_mode) as interp_ops.hip states them
InterpArgs interp_args(const float* x, int ih, int iw, int oh, int ow, int method, int align_corners, int align_mode);
// yf / yq [planes][oh][ow]: either may be null
void launch_interp(const InterpArgs& a, int64_t planes, float* yf, int8_t* yq, float calib_scale, hipStream_t s);
// x [outer][c][inner] -> y [outer][inner]: the largest index among the maxima; i64: int64 labels, else int32
void launch_arg_max(const float* x, int64_t outer, int c, int64_t inner, void* y, int i64, hipStream_t s);
// a.x [n][c][ih][iw] -> y [n][oh][ow]: arg_max over c of the resampled tensor, which is never written
void launch_interp_argmax(const InterpArgs& a, int n, int c, void* y, int i64, hipStream_t s);

// transpose of fp32 tensors of rank <= 4 and the one-launch join of an SSD head: transpose_ops.hip
struct TransposeArgs {
  const float* x;
  float* y;
  int64_t total;
  // rows copied whole: output extents and the source stride of every output axis (leading axes of extent 1 fill the rank)
  int64_t od[4], ss[4];
  // batch of 2-D transposes: D = the destination's innermost axis (source row stride sd), S = the source's innermost axis
  // (destination row stride dd), two batch axes with their strides on both sides
  int64_t D, S, sd, dd, B0, B1, bs[2], bd[2];
};
// y = transpose(x, perm): x of extents dims[rank], y axis k is x axis perm[k]
void launch_transpose(const float* x, const int64_t* dims, const int* perm, int rank, float* y, hipStream_t s);
struct ConcatNhwcArgs {
  const float* part[CONCAT_MAX_PARTS];  // NCHW [n][c[p]][hw[p]]
  int64_t c[CONCAT_MAX_PARTS], hw[CONCAT_MAX_PARTS];
  int64_t off[CONCAT_MAX_PARTS];        // where operand p starts inside an image of y
  float* y;                             // [n][stride]
  int64_t stride, n;
};
// xs[i]: NCHW [n][channels[i]][hw[i]] -> y [n][sum channels * hw], operand i as [hw[i]][channels[i]].  One launch per
// CONCAT_MAX_PARTS operands.
void launch_concat_nhwc(const float* const* xs, const int64_t* channels, const int64_t* hw, int count, int64_t n, float* y, hipStream_t s);

// box_coder (decode_center_size) and multiclass_nms: detection_ops.hip
struct BoxCoderArgs {
  const float* prior;   // [cols][4] (axis 0) | [rows][4] (axis 1)
  const float* pvar;    // like prior, var == 2 only
  const float* target;  // [rows][cols][4]
  float* y;             // [rows][cols][4]
  v4f variance;         // var == 1: the attribute; var == 0: ones
  int64_t rows, cols, boxes;
  int axis, normalized, var, vec;
};
void launch_box_coder_decode(BoxCoderArgs a, hipStream_t s);  // fills boxes and vec
struct NmsArgs {
  const float* boxes;   // [N][P][4]
  const float* scores;  // image i, class c, prior p at scores[i * C * P + c * ssc + p * ssp]
  float* out;           // [N][keep][6]
  int* index;           // [N][keep] or null
  int* count;           // [N]
  uint64_t* ws_list;    // [N][C][cap]: (score bits << 32) | prior of the class's kept boxes, in the order they were kept
  int* ws_len;          // [N][C]
  int C, P;
  int64_t ssc, ssp;
  int bg;
  float sthr, nthr;
  int keep, normalized;
  int kmax, cap, nact;  // nms_sizes
  int box_off, kept_off, wcnt_off, removed_off, wcnt_off_b, vec;  // launch_multiclass_nms fills them
};
void nms_sizes(int C, int P, int bg, int nms_top_k, int keep_top_k, int* kmax, int* cap, int* nact);
void launch_multiclass_nms(NmsArgs a, int N, hipStream_t s);

// yolo_box of one scale and the one-launch head of up to YOLO_MAX_SCALES scales: yolo_ops.hip
constexpr int YOLO_MAX_SCALES = 8;    // as CONCAT_MAX_PARTS: the operands travel in the argument struct
constexpr int YOLO_MAX_ANCHORS = 16;  // anchors of one scale; they travel in the argument struct too
struct YoloScale {
  const float* x;  // [n][an * (5 + classes)][h][w]
  int h, w, an, ratio;
  int anchors[2 * YOLO_MAX_ANCHORS];
  int p_off, chunks, vec;  // the head: launch_yolo_head fills them
};
struct YoloCommon {
  const int* img_size;  // [n][2]: height, width
  int64_t n;
  int classes, clip;
  float thresh, scale, bias;
};
struct YoloBoxArgs {
  YoloScale s;
  YoloCommon c;
  float* boxes;   // [n][an * h * w][4]
  float* scores;  // [n][an * h * w][classes]
  int vec;        // launch_yolo_box fills it
};
void launch_yolo_box(YoloBoxArgs a, hipStream_t s);
struct YoloHeadArgs {
  YoloScale s[YOLO_MAX_SCALES];
  YoloCommon c;
  float* boxes;   // [n][P][4], P = sum of an * h * w, scale i behind the scales in front of it
  float* scores;  // [n][classes][P]
  int count;
  int P, box_vec, first[YOLO_MAX_SCALES];  // launch_yolo_head fills them; first: the scale's first block of grid x
};
void launch_yolo_head(YoloHeadArgs a, hipStream_t s);

}  // namespace plhip
