// dw_plan.h — which depthwise / fused depthwise -> 1x1 kernel instance runs a problem, with which grid: pure host functions.
//
// depthwise_launch_plan (depthwise_i8.hip), dwpw_launch_plan (fusion D: fused_dwpw_i8.hip, fused_dwpw_stream.hip,
// fused_dwpw_small.hip) and dw_conv1x1_launch_plan (fusion G: fused_dwconv_i8.hip) decide family, template parameters, the
// launch-plan fields of the kernel's argument block, grid, block and dynamic LDS.  The launchers only execute a plan, the C
// entries and their *_supported predicates ask the same function (plhip_capi_conv.hip), plhip_debug_dw_plan prints it for the
// tests, and tests/golden/dw_plans/ pins it over a sweep (tools/dump_dw_plans.py).  Plain C++17, no HIP: a stand-alone
// program compiles it with g++ alone.  The knobs: DESIGN.md 3.6; the quirks kept on purpose: DESIGN.md 3.6a.
// The (DWNN, PWNN) split of the fused kernels follows the activations, which no plan reads: it stays with the executor.
#pragma once
#include <stddef.h>
#include <stdio.h>
#include <string.h>

#include "dw_common.h"

namespace plhip {

enum DwFamily { DW_NONE = 0, DW_DIRECT, DW_BAND, DWPW_14, DWPW_STREAM, DWPW_7, DW_CONV1X1 };
enum { DW_OUT_I32 = 0, DW_OUT_F32 = 1, DW_OUT_I8 = 2, DW_OUT_GAP = 3 };  // == OUT_* (plhip_device.h) == plhip_out_kind

// LDS geometry the kernels and their plans share
constexpr int FW_SP = 112;      // 14 x 14 kernel: staging pitch of a channel row (98 bytes used)
constexpr int FW_KSTEP = 4096;  // 14 x 14 kernel: LDS bytes of one K-step of the activation image: [kg 4][k%8 8][chunk slot 8][16 B]
constexpr int fs_pitch(int tp) { return tp == 128 ? 160 : (tp == 224 ? 288 : 544); }  // streaming kernel: bytes per channel row of a TP-pixel tile
constexpr int F7_PITCH = 96;    // 7 x 7 kernel: bytes per channel row of the image: 64 slots + pad
constexpr int DC_APITCH = 48;   // fusion G: LDS bytes per pixel row of the activation tile (32 channels of a K-step + 16)
constexpr int DC_THREADS = 256;

// what the decisions read of a launch
struct DwProblem {
  int n, C, h, w, oh, ow, kh, kw, pt, pl, sh, sw, dh, dw;
  int out;                // DW_OUT_*
  int pw_M = 0;           // the fused kinds: output channels of the 1x1 conv
  bool x_aligned = true;  // fusion G: the input pointer is 4-byte aligned
};

// the A/B knobs at their defaults
struct DwKnobs {
  int stage = 1;         // DW_STAGE: int8 output staged through LDS on narrow planes
  int stage_np2 = 1;     // DW_STAGE_NP2: 1 = rows of a non-power-of-two quad count staged up to 32 columns, 2 = up to 64, 0 = never
  int fastv = 1;         // DW_FASTV: the fast row fetch
  int k5_direct = 1;     // DW5_DIRECT: 0 = 5x5 filters on the LDS-band kernel
  int rs1 = 0, rs2 = 0;  // DW_RS1 / DW_RS2: strip height forced (4, 7, 8) at stride 1 / 2; other values: automatic
  int fused_stream = 1;  // FUSED_STREAM: 1 every shape of the streaming kernel, 2 stride 1 only, 3 not the 14-wide plane, 0 off
  int fused_small = 1;   // FUSED_SMALL: 0 off, 1 one block per image, 2 two blocks per image along M
  int dwconv_fused = 1;  // DWCONV_FUSED: 0 = fusion G refuses every shape
};

// the whole launch.  Template parameters a family does not have are 0.
struct DwPlan {
  int family = DW_NONE;
  const char* why = "";           // DW_NONE: the reason the C ABI reports
  char name[24] = "none";
  unsigned grid_x = 0, grid_y = 1, block = 0;
  size_t lds = 0;                 // dynamic LDS bytes
  // ---- template parameters
  int KS = 0, RS = 0;             // dw_direct: filter size 3 | 5, rows per strip 4 | 7 | 8 (dwpw_stream: RS too)
  int S = 0;                      // stride: dw_direct, dwpw_stream, dwpw_7x7, dw_conv1x1
  bool STAGE = false, FASTV = false;  // dw_direct: output staging through LDS, fast row fetch
  int FAST = 0;                   // dw_band: 31 | 32 | 51 | 52 = (k, stride) of a dot4 path, 0 = dw_generic's scalar path
  int MTW = 0;                    // dwpw_14x14: m tiles per wave (2: M = 512)
  int W = 0, K = 0, M = 0, TP = 0, PD = 0, MP = 0;  // dwpw_stream (K, M, PD: dwpw_7x7 too)
  int MB = 0;                     // dwpw_7x7: blocks per image along M
  int NACC = 0, PL = 0;           // dw_conv1x1: accumulators per wave, left padding
  bool DWORD = false;             // dw_conv1x1: rows staged as dwords (else bytes)
  // ---- launch-plan fields of the argument block
  struct Direct {                 // DwArgs, direct kernels
    long total_lanes;
    int owq_log2, spp_log2, fast_div;
    unsigned div_owq_m, div_spp_m, div_c_m;
    int div_owq_s, div_spp_s, div_c_s;
    int stage_bytes, lw, nblocks;
  } d = {};
  struct Band { int PB, OB, bands, in_rows, pitch; } b = {};  // DwArgs, LDS-band kernel
  int tiles = 0, NT = 0;          // FusedArgs::tiles, FusedArgs::pw.NT (streaming kernel: tiles per image)
  struct G {                      // DwConvArgs (the fields' meaning: plhip_kernels.h)
    int KS, mt32, mtpb, mgroups, TR, CW, NT, tr_tiles, cw_tiles, tpi, IR, WP, wu, rpp;
    unsigned ir_m, owq_m, tr_m, cw_m, tpi_m, ctl_m;
    int ir_s, owq_s, tr_s, cw_s, tpi_s, ctl_s;
  } g = {};
};

namespace dw_plan_detail {

inline DwPlan named(int family, const char* name) {
  DwPlan p;
  p.family = family;
  strncpy(p.name, name, sizeof p.name - 1);
  return p;
}
inline DwPlan refused(const char* why) {
  DwPlan p;
  p.why = why;
  return p;
}
inline unsigned round8(long blocks) { return (unsigned)((blocks + 7) / 8 * 8); }  // 8 XCDs x equal shares (the kernels' vb map)
inline int lg2_exact(long v) {
  int l = 0;
  while ((1L << l) < v) ++l;
  return (1L << l) == v ? l : -1;
}

// Tiling of the LDS-band kernel: a block covers PB planes x OB output rows; aim at ~2K quads (8 per thread) per block and keep
// the LDS tile under 48 KiB so that several blocks share a CU.  false: a single row band does not fit in LDS (60 KiB).
inline bool band_tiling(const DwProblem& a, DwPlan::Band* t) {
  const long planes = (long)a.n * a.C;
  const int owq = (a.ow + 3) / 4;
  const int OFF = (a.pl + 3) / 4 * 4;
  const int maxcol = (4 * owq - 1) * a.sw - a.pl + (a.kw - 1) * a.dw + OFF;
  const int pitch = ((maxcol > OFF + a.w ? maxcol : OFF + a.w) + 1 + 16 + 3) / 4 * 4;
  const int target = 2048;
  int OB, PB;
  if (a.oh * owq >= target) {
    PB = 1;
    OB = target / owq;
    if (OB < 1) OB = 1;
    if (OB > a.oh) OB = a.oh;
  } else {
    OB = a.oh;
    PB = target / (a.oh * owq);
    if (PB < 1) PB = 1;
    if (PB > 64) PB = 64;
    if (PB > planes) PB = (int)planes;
  }
  auto in_rows_of = [&](int ob) { return (ob - 1) * a.sh + (a.kh - 1) * a.dh + 1; };
  // the fit test counts the filter bytes + 16; the launch (band_lds) rounds them up to 16: always less, so a tiling that
  // passes here can never exceed the 64 KiB a launch may ask for without raising the limit
  auto lds_of = [&](int pb, int ob) {
    return (size_t)pb * in_rows_of(ob) * pitch + (size_t)pb * a.kh * 8 + (size_t)pb * 8 + (size_t)pb * a.kh * a.kw + 16;
  };
  while (lds_of(PB, OB) > 48 * 1024 && PB > 1) PB = PB / 2;
  while (lds_of(PB, OB) > 48 * 1024 && OB > 1) OB = (OB + 1) / 2;
  if (lds_of(PB, OB) > 60 * 1024) return false;
  *t = DwPlan::Band{PB, OB, (a.oh + OB - 1) / OB, in_rows_of(OB), pitch};
  return true;
}
inline size_t band_lds(const DwProblem& a, const DwPlan::Band& t) {
  return (size_t)t.PB * t.in_rows * t.pitch + (size_t)t.PB * a.kh * 8 + (size_t)t.PB * 8 + (((size_t)t.PB * a.kh * a.kw + 15) & ~(size_t)15);
}

// The direct strip kernels: 3x3 / 5x5, stride 1 | 2, dilation 1, left padding <= 3, 32-bit element offsets.
inline bool direct_plan(const DwProblem& a, const DwKnobs& kn, DwPlan* out) {
  const long planes = (long)a.n * a.C;
  const bool k3 = a.kh == 3 && a.kw == 3, k5 = a.kh == 5 && a.kw == 5 && kn.k5_direct;
  if (!((k3 || k5) && a.dh == 1 && a.dw == 1 && a.sh == a.sw && (a.sw == 1 || a.sw == 2) && a.pl <= 3)) return false;
  if (planes * a.h * a.w >= (1L << 31) || planes * a.oh * a.ow >= (1L << 31)) return false;
  DwPlan p = named(DW_DIRECT, "dw_direct");
  p.KS = k5 ? 5 : 3;
  p.S = a.sw;
  // rows per strip: amortise the 2-row halo while keeping many lanes (and bytes) in flight
  const int forced = a.sw == 1 ? kn.rs1 : kn.rs2;
  int rs;
  if (forced == 4 || forced == 7 || forced == 8) rs = forced;
  else if (a.sw == 1) rs = (a.oh % 8 == 0) ? 8 : (a.oh % 7 == 0 ? 7 : (a.oh >= 8 ? 8 : (a.oh >= 5 ? 7 : 4)));
  // stride 2 fetches 2 rows per output row: taller strips measured slower (dw3 33.7 -> 37.1 us): not VALU-bound
  else rs = (a.oh % 7 == 0 && a.oh <= 14) ? 7 : 4;
  p.RS = rs;
  const long owq = (a.ow + 3) >> 2;
  const long spp = (a.oh + rs - 1) / rs;
  const long total = planes * spp * owq;
  DwPlan::Direct& d = p.d;
  d.total_lanes = total;
  d.owq_log2 = lg2_exact(owq);
  d.spp_log2 = lg2_exact(spp);
  d.fast_div = d.owq_log2 >= 0 && d.spp_log2 >= 0 && lg2_exact(a.C) >= 0;
  fastdiv_magic(owq, d.div_owq_m, d.div_owq_s);
  fastdiv_magic(spp, d.div_spp_m, d.div_spp_s);
  fastdiv_magic(a.C, d.div_c_m, d.div_c_s);
  // output staging through LDS: int8 output, narrow planes, a wave = whole strips, strips = whole rows of the plane
  // (owq a power of two: a wave = 64 lanes = whole strips; otherwise a wave uses (64 / owq) * owq lanes: 63 of 64 on
  // 28-wide planes, 56 of 64 on 56-wide ones — the 14x14 layers went 19.3 -> 11.0 us with staging, and a 28x28 layer
  // moves the same bytes with the same arithmetic)
  // measured: 28-wide planes gain ~5 % (dw6 19.7 -> 18.7 us), 56-wide ones lose ~5 %: the store-request granularity that
  // staging cures is a narrow-row effect; stage_np2 = 2 forces it for every width <= 64
  p.STAGE = kn.stage && a.out == DW_OUT_I8 && a.ow <= 64 && owq <= 64 && a.oh % rs == 0 &&
            (d.owq_log2 >= 0 || (kn.stage_np2 == 1 && a.ow <= 32) || kn.stage_np2 >= 2);
  d.lw = p.STAGE ? (int)((64 / owq) * owq) : 64;
  d.nblocks = p.STAGE ? (int)(((total + d.lw - 1) / d.lw + 3) / 4) : (int)((total + 255) / 256);
  d.stage_bytes = p.STAGE ? (int)(((64 / owq) * rs * a.ow + 15) & ~15) : 0;
  // fast row fetch: only the first / last row of a strip can leave the image, windows start inside the row
  const int PV = (p.KS - 1) / 2;
  p.FASTV = kn.fastv && a.pt <= PV && (a.oh - 1) * p.S + p.KS - 1 - a.pt <= a.h - 1 + PV && a.oh % rs == 0 &&
            (owq - 1) * 4 * p.S - a.pl < a.w;
  p.grid_x = round8(d.nblocks);
  p.block = 256;
  p.lds = p.STAGE ? (size_t)4 * d.stage_bytes : 0;
  *out = p;
  return true;
}

// the streaming kernel's instances: MobileNetV1's pairs on the large planes
// ROWS: the produce stage takes its input rows as 16-byte pieces through a wave-private LDS stage (stream_rows.h) instead of
// row windows straight from global memory.  The stage is STATIC LDS of the kernel instance: no part of DwPlan::lds, not printed
// by dw_plan_text.  On for the stride-1 pairs at 112 and 56 (46.7 / 43.1 -> 38.2 / 39.0 us and 38.4 / 38.6 -> 36.1 / 36.3 us in
// the serial step).  Off where the stage does not fit (256 -> 256 @28: 80 KiB are half a CU), where the kernel is not
// VALU-bound (14), and for the stride-2 pairs onto 56 and 28: staged they issue 33 / 60 fewer VALU and 20 / 33 fewer vector
// loads per wave and ran 29.5 / 30.6 -> 31.7 / 33.6 us and 21.7 / 21.0 -> 23.7 / 23.3 us (DESIGN 8.2 "Rows staged").
struct StreamShape { int W, S, K, M, TP, RS, PD, MP; bool ROWS; };  // W = output plane width
constexpr StreamShape kStreamShapes[] = {
    {112, 1, 32, 64, 448, 4, 2, 1, true},   // 4-row tiles of 448 pixels (2-row tiles fetched and cut every input row twice: 61 us, the two kernels 56)
    {56, 1, 128, 128, 224, 4, 2, 1, true},
    {28, 1, 256, 256, 224, 4, 2, 1, false},
    {56, 2, 64, 128, 224, 4, 2, 1, false},
    {28, 2, 128, 256, 224, 4, 2, 1, false},
    {14, 2, 256, 512, 128, 7, 2, 2, false},  // half images, M in two passes
};
constexpr bool stream_rows_staged(int W, int S) {
  for (const StreamShape& t : kStreamShapes)
    if (t.W == W && t.S == S) return t.ROWS;
  return false;
}
// the 7 x 7 kernel's: MobileNetV1's last two pairs
struct SmallShape { int S, K, M; };
constexpr SmallShape kSmallShapes[] = {{2, 512, 1024}, {1, 1024, 1024}};

// square planes, pad 1, h = oh * stride, 32-bit element offsets: what the streaming and the 7 x 7 kernel ask alike
inline bool pair_plane_ok(const DwProblem& a) {
  return a.h == a.w && a.oh == a.ow && a.pt == 1 && a.pl == 1 && a.h == a.oh * a.sh && a.n >= 1 &&
         (long)a.n * a.C * a.h * a.w < ((long)1 << 31) - 65536 && (long)a.n * a.pw_M * a.oh * a.ow < ((long)1 << 31);
}

}  // namespace dw_plan_detail

// plhip_depthwise_conv_int8.  The band tiling is asked first, and its refusal stands even where the direct kernel, which needs
// no band, would have run the shape.
inline DwPlan depthwise_launch_plan(const DwProblem& a, const DwKnobs& kn) {
  using namespace dw_plan_detail;
  DwPlan::Band t;
  if (!band_tiling(a, &t)) return refused("a single row band does not fit in LDS");
  DwPlan p;
  if (direct_plan(a, kn, &p)) return p;
  const bool fast = a.kh == a.kw && (a.kw == 3 || a.kw == 5) && a.sh == a.sw && (a.sw == 1 || a.sw == 2) && a.dh == 1 && a.dw == 1;
  p = named(DW_BAND, fast ? "dw_band" : "dw_generic");
  p.FAST = fast ? a.kw * 10 + a.sw : 0;
  p.b = t;
  p.grid_x = (unsigned)(((a.n * a.C + t.PB - 1) / t.PB) * t.bands);
  p.block = 256;
  p.lds = band_lds(a, t);
  return p;
}

// plhip_dwpw_fused_int8 (fusion D): a 3x3 depthwise conv (int8 out) and the 1x1 conv behind it
inline DwPlan dwpw_launch_plan(const DwProblem& a, const DwKnobs& kn) {
  using namespace dw_plan_detail;
  static const char* const outside = "shape outside the fused path";
  if (!(a.kh == 3 && a.kw == 3 && a.sh == a.sw && (a.sh == 1 || a.sh == 2) && a.dh == 1 && a.dw == 1)) return refused(outside);
  const int fs = kn.fused_stream;
  // (the plane average as output, DW_OUT_GAP, exists on the 7 x 7 kernel only: nothing else may accept it)
  if (a.out != DW_OUT_GAP && fs && (a.sh == 1 || fs != 2) && !(fs == 3 && a.ow == 14) && pair_plane_ok(a)) {
    for (const StreamShape& t : kStreamShapes) {
      if (!(a.ow == t.W && a.sh == t.S && a.C == t.K && a.pw_M == t.M)) continue;
      DwPlan p = named(DWPW_STREAM, "dwpw_stream");
      p.W = t.W; p.K = t.K; p.M = t.M; p.TP = t.TP; p.RS = t.RS; p.PD = t.PD; p.S = t.S; p.MP = t.MP;
      const int TR = t.W == 14 ? 7 : t.TP / t.W;
      p.NT = (a.oh + TR - 1) / TR;
      p.tiles = a.n * p.NT;
      p.grid_x = round8(p.tiles);
      p.block = 256;
      // image, depthwise parameters, sink of the idle lanes (256 -> 256 @28 has none: its 80 KiB are exactly half a CU's LDS,
      // and 512 bytes more made it one block per CU: 28.3 -> 34.0 us).
      // The row stage of the ROWS shapes (4 waves x stream_rows::Rows::WB = 6.25 KiB at 112 and at 56 wide) is STATIC LDS of the
      // kernel instance and no part of lds=: this is the dynamic size the launch asks for, the one dw_plan_text prints and
      // tests/golden/dw_plans pins; the kernel asserts static + dynamic bytes x blocks per CU against the CU's 160 KiB.
      p.lds = (size_t)t.K * fs_pitch(t.TP) + (size_t)t.K * 32 + (t.M / t.MP < 256 ? 512 : 0);
      return p;
    }
  }
  if (kn.fused_small && a.oh == 7 && pair_plane_ok(a)) {
    for (const SmallShape& t : kSmallShapes) {
      if (!(a.sh == t.S && a.C == t.K && a.pw_M == t.M)) continue;
      DwPlan p = named(DWPW_7, "dwpw_7x7");
      p.K = t.K; p.M = t.M; p.S = t.S; p.PD = 2;
      // blocks per image along M: 1 (default) = no duplicated work, half the CUs at batch 128: what several predictors in
      // flight prefer (c3: 379 k img/s against 370 k / 370 k with two blocks / the two kernels; one step in flight 300 k /
      // 308 k / 291 k); 2 = every CU gets a block, the depthwise stage computed twice: best alone
      p.MB = kn.fused_small == 2 ? 2 : 1;
      p.tiles = a.n * p.MB;
      p.grid_x = round8(p.tiles);
      p.block = 512;
      p.lds = (size_t)t.K * F7_PITCH + (size_t)t.K * 32;
      return p;
    }
  }
  // the 14 x 14 kernel: stride 1, pad 1, 128 | C <= 512 (whole rounds; the K x 128 activation image + the staging image fit the
  // LDS), M = 256 or 512 (one or two m tiles per wave)
  if (a.out == DW_OUT_GAP || a.sh != 1) return refused(outside);
  if (!(a.h == 14 && a.w == 14 && a.oh == 14 && a.ow == 14 && a.pt == 1 && a.pl == 1)) return refused(outside);
  if (a.C % 128 != 0 || a.C < 128 || a.C > 512) return refused(outside);
  if (a.pw_M != 256 && a.pw_M != 512) return refused(outside);
  if (a.n < 1 || (long)a.n * a.C * 196 >= ((long)1 << 31) - 65536 || (long)a.n * a.pw_M * 196 >= ((long)1 << 31)) return refused(outside);
  DwPlan p = named(DWPW_14, a.pw_M == 512 ? "dwpw_14x14_mtw2" : "dwpw_14x14");
  p.MTW = a.pw_M == 512 ? 2 : 1;
  p.tiles = 2 * a.n;  // (image, half-plane) tiles
  p.grid_x = round8(p.tiles);
  p.block = 512;
  p.lds = (size_t)(a.C / 32) * FW_KSTEP + (a.out == DW_OUT_I8 ? (size_t)8 * 32 * p.MTW * FW_SP : 0);
  return p;
}

// plhip_dw_conv1x1_fused_int8 (fusion G): 3x3, dilation 1, stride 1 | 2, paddings 0 | 1 (the C entry checks those)
inline DwPlan dw_conv1x1_launch_plan(const DwProblem& a, const DwKnobs& kn) {
  using namespace dw_plan_detail;
  static const char* const outside = "shape outside the fused kernel (C % 16, C <= 1024, M % 8, M <= 1024, 32-bit element offsets)";
  if (!kn.dwconv_fused) return refused("fused depthwise -> 1x1 kernel switched off (diagnostics knob DWCONV_FUSED = 0)");
  const int M = a.pw_M, S = a.sh;
  if (a.n < 1 || a.h < 1 || a.w < 1 || a.oh < 1 || a.ow < 1) return refused(outside);
  if (a.C < 16 || a.C % 16 != 0 || a.C > 1024) return refused(outside);
  if (M < 8 || M % 8 != 0 || M > 1024) return refused(outside);
  if (S != 1 && S != 2) return refused(outside);
  if (a.pl != 0 && a.pl != 1) return refused(outside);
  // int32 element offsets: every tensor index (input, output, residual, calib copy) below 2^31
  if ((long long)a.n * a.C * a.h * a.w >= (1ll << 31) || (long long)a.n * M * a.oh * a.ow >= (1ll << 31)) return refused(outside);
  DwPlan p = named(DW_CONV1X1, "dw_conv1x1");
  DwPlan::G& g = p.g;
  g.KS = (a.C + 31) / 32;
  g.mt32 = (M + 31) / 32;
  // tile: whole rows, <= 128 pixels (wider rows: 128-column segments), LDS <= 64 KiB
  g.CW = a.ow <= 128 ? a.ow : 128;
  g.TR = a.ow <= 128 ? (128 / a.ow < a.oh ? 128 / a.ow : a.oh) : 1;
  if (g.TR < 1) g.TR = 1;
  const int nd = (7 + 3 * S) / 4 + 1, owq = (g.CW + 3) / 4;
  for (;;) {
    g.IR = (g.TR - 1) * S + 3;
    g.WP = 4 * (owq - 1) * S + 4 * nd;
    g.NT = (g.TR * g.CW + 31) / 32;
    p.lds = (size_t)2 * 32 * g.IR * g.WP + (size_t)2 * g.NT * 32 * DC_APITCH;
    if (p.lds <= 64 * 1024 || g.TR == 1) break;
    g.TR = (g.TR + 1) / 2;
  }
  if (p.lds > 64 * 1024) return refused(outside);
  g.mtpb = g.mt32 < 32 / g.NT ? g.mt32 : 32 / g.NT;
  g.mgroups = (g.mt32 + g.mtpb - 1) / g.mtpb;
  const int pairs = g.mtpb * g.NT;
  p.NACC = pairs <= 4 ? 1 : (pairs <= 8 ? 2 : (pairs <= 16 ? 4 : 8));
  g.tr_tiles = (a.oh + g.TR - 1) / g.TR;
  g.cw_tiles = (a.ow + g.CW - 1) / g.CW;
  g.tpi = g.tr_tiles * g.cw_tiles;
  if ((long long)a.n * g.tpi >= (1ll << 31)) return refused(outside);
  // rows are staged as dwords when they and the input pointer sit on 4 bytes, else byte by byte; rows per wave pass
  p.DWORD = a.w % 4 == 0 && a.x_aligned;
  g.wu = p.DWORD ? g.WP / 4 : g.WP;
  g.rpp = g.wu <= 64 ? 64 / g.wu : 1;
  fastdiv_magic(g.IR, g.ir_m, g.ir_s);
  fastdiv_magic(owq, g.owq_m, g.owq_s);
  fastdiv_magic(g.TR, g.tr_m, g.tr_s);
  fastdiv_magic(g.CW, g.cw_m, g.cw_s);
  fastdiv_magic(g.tpi, g.tpi_m, g.tpi_s);
  fastdiv_magic(g.cw_tiles, g.ctl_m, g.ctl_s);
  p.S = S;
  p.PL = a.pl;
  p.grid_x = (unsigned)(a.n * g.tpi);
  p.grid_y = (unsigned)g.mgroups;
  p.block = DC_THREADS;
  return p;
}

// the plan as one line of text (plhip_debug_dw_plan, tests/golden/dw_plans/): name, the instance, the launch, the argument fields
inline int dw_plan_text(const DwPlan& p, char* buf, size_t cap) {
  if (p.family == DW_NONE) return snprintf(buf, cap, "none why=%s", p.why);
  int n = snprintf(buf, cap, "%s KS=%d S=%d RS=%d STAGE=%d FASTV=%d FAST=%d MTW=%d W=%d K=%d M=%d TP=%d PD=%d MP=%d MB=%d NACC=%d PL=%d DWORD=%d "
                   "grid=%u,%u block=%u lds=%zu |",
                   p.name, p.KS, p.S, p.RS, (int)p.STAGE, (int)p.FASTV, p.FAST, p.MTW, p.W, p.K, p.M, p.TP, p.PD, p.MP, p.MB, p.NACC, p.PL,
                   (int)p.DWORD, p.grid_x, p.grid_y, p.block, p.lds);
  if (n < 0 || (size_t)n >= cap) return n;
  char* o = buf + n;
  const size_t room = cap - (size_t)n;
  int m = 0;
  if (p.family == DW_DIRECT)
    m = snprintf(o, room, " total=%ld owq_log2=%d spp_log2=%d fast_div=%d div=%u,%d,%u,%d,%u,%d stage_bytes=%d lw=%d nblocks=%d", p.d.total_lanes,
                 p.d.owq_log2, p.d.spp_log2, p.d.fast_div, p.d.div_owq_m, p.d.div_owq_s, p.d.div_spp_m, p.d.div_spp_s, p.d.div_c_m,
                 p.d.div_c_s, p.d.stage_bytes, p.d.lw, p.d.nblocks);
  else if (p.family == DW_BAND)
    m = snprintf(o, room, " PB=%d OB=%d bands=%d in_rows=%d pitch=%d", p.b.PB, p.b.OB, p.b.bands, p.b.in_rows, p.b.pitch);
  else if (p.family == DW_CONV1X1)
    m = snprintf(o, room, " KS=%d mt32=%d mtpb=%d mgroups=%d TR=%d CW=%d NT=%d tr_tiles=%d cw_tiles=%d tpi=%d IR=%d WP=%d wu=%d rpp=%d "
                 "div=%u,%d,%u,%d,%u,%d,%u,%d,%u,%d,%u,%d",
                 p.g.KS, p.g.mt32, p.g.mtpb, p.g.mgroups, p.g.TR, p.g.CW, p.g.NT, p.g.tr_tiles, p.g.cw_tiles, p.g.tpi, p.g.IR, p.g.WP,
                 p.g.wu, p.g.rpp, p.g.ir_m, p.g.ir_s, p.g.owq_m, p.g.owq_s, p.g.tr_m, p.g.tr_s, p.g.cw_m, p.g.cw_s, p.g.tpi_m, p.g.tpi_s,
                 p.g.ctl_m, p.g.ctl_s);
  else
    m = snprintf(o, room, " tiles=%d NT=%d", p.tiles, p.NT);
  return m < 0 ? m : n + m;
}

}  // namespace plhip
