// gemm_plan.h — which GEMM kernel instance runs a problem, with which grid: ONE pure host function.
//
// launch_gemm_i8 (gemm_i8.hip) executes the plan, the implicit-GEMM route asks it whether its kernel takes a descriptor
// (plhip_capi_conv.hip), plhip_debug_gemm_plan prints it for the tests, and tests/golden/gemm_plans/ pins it over a sweep
// (tools/dump_gemm_plans.py).  Plain C++17, no HIP: a stand-alone program compiles it with g++ alone.  Why each threshold is
// where it is: DESIGN.md 3.1; the kernels themselves: gemm_i8.hip (private tiles, LDS, ring), gemm_tr_i8.hip, gemm_wide_i8.hip.
#pragma once
#include <stddef.h>
#include <stdio.h>
#include <string.h>

namespace plhip {

enum GemmFamily { GEMM_NONE = 0, GEMM_PRIVATE, GEMM_LDS, GEMM_RING, GEMM_TR, GEMM_WIDE };
enum { GEMM_OUT_I32 = 0, GEMM_OUT_F32 = 1, GEMM_OUT_I8 = 2 };  // == OUT_* (plhip_device.h) == plhip_out_kind

// what the decision reads of a launch (GemmArgs, plhip_kernels.h) and of its caller
struct GemmProblem {
  int M, K, KS;       // rows, reduction length, K-steps of 32
  int HWX, HWY;       // columns per image as the caller counts them (dense slab: rounded up to 4) / valid output columns
  int XP;             // x row pitch in bytes (0: implicit GEMM)
  int NB;             // images (implicit GEMM: batch * output rows)
  int im_kw, im_s;    // implicit GEMM: filter width (0 = a plain GEMM) and stride
  bool res, y2, y;    // the fused tail's residual / int8 copy, and the output itself, are set
  int out;            // GEMM_OUT_*
  int ma;             // 32-row fragment tiles per wave tile the weights were packed for (1: M <= 32, else 2)
  bool vec_store, aligned_loads;  // outputs on 4 elements / B rows on 4 bytes
};

// the A/B knobs at their defaults
struct GemmKnobs {
  int variant = 0;     // GEMM_VARIANT: 0 automatic, 1 private tiles, 2 LDS, 3 ring
  int areg = 1;        // GEMM_AREG: A fragments of the ring kernel in a register ring
  int ma = 0;          // GEMM_MA: 0 automatic, 1 32-row wave tiles, other: as packed
  int tr = 1;          // GEMM_TR: 0 off, 1 the implicit-GEMM engine, 2 plain GEMMs too
  int tr_cfg = 3;      // TR_CFG: bit 0 / 1 = the 4-wave tile for M > 128 / M > 64
  int wide = 1;        // GEMM_WIDE
  // the wide tile forced (4, 7, 8; 0 = the cost model): plhip_debug_wide_ntt's value when it is >= 0, else the knob WIDE_NTT.
  // wide_any_out: either mechanism is engaged (an override >= 0, 0 included, or a non-zero knob): 32-bit outputs may then
  // take the wide kernel too.
  int wide_force = 0;
  bool wide_any_out = false;
  // LDS bytes of the timeline stamps per family: an EXPERIMENTS=1 build's; 0 in a default build
  int stamp_lds_ring = 0, stamp_lds_tr = 0, stamp_lds_wide = 0;
};

// the one place where the two ways to force the wide tile meet: override = plhip_debug_wide_ntt's value (-1: none), knob = WIDE_NTT
inline void gemm_resolve_wide_force(GemmKnobs* k, int override_value, int knob_value) {
  k->wide_force = override_value >= 0 ? override_value : knob_value;
  k->wide_any_out = override_value >= 0 || knob_value != 0;
}

// the whole launch.  Template parameters a family does not have are 0.
struct GemmPlan {
  int family = GEMM_NONE;  // GEMM_NONE: the operand exists on one kernel only and it declines (launch_gemm_i8's -3)
  int MA = 0;              // private / LDS / ring
  int OUT = 0;             // tr: after the F32 -> I8 substitution
  bool VEC_STORE = false, MFULL = false, ALIGNED = false;  // private / LDS (ring: no ALIGNED)
  int NG = 0;              // ring: KS / 4 of the straight-line AREG form, 0 = A through LDS
  int WN = 0, WM = 0, D = 0;  // tr: waves along N / M, K-steps in flight
  bool IM = false;         // tr: implicit GEMM
  int NTT = 0;             // wide: 32-column n tiles per block
  int HWX = 0, MT = 0, NT = 0;  // GemmArgs fields as the kernel receives them
  unsigned grid = 0, block = 0;
  size_t lds = 0;          // dynamic LDS bytes
  // ring, implicit GEMM: false = the ring kernel runs it because no other first-generation kernel can, not because its
  // thresholds chose it (the route table takes a descriptor for the ring only on merit)
  bool on_merit = true;
  char name[24] = "none";
};

namespace gemm_plan_detail {

inline void set_name(GemmPlan* p, const char* name) { strncpy(p->name, name, sizeof p->name - 1); }
inline long cdiv(long a, long b) { return (a + b - 1) / b; }
inline unsigned grid8(long m_blocks, int nt) { return (unsigned)(m_blocks * (long)((nt + 7) / 8 * 8)); }  // N tiles padded to the 8 XCDs

// The wide kernel's tile: n tiles per block so that the blocks fill the CUs once with as little idle tail as possible;
// 0 = the shape is outside the kernel.  hwx: the TRUE row length.
inline int wide_ntt(const GemmProblem& g, const GemmKnobs& kn, int hwx) {
  // 32-bit outputs: the ring kernels are faster on every MobileNetV1 layer (row-per-lane 16-byte stores write 32 contiguous
  // bytes per row and instruction, the ring kernels' epilogue 64): reachable for them only through a forced tile
  if (g.out != GEMM_OUT_I8 && !kn.wide_any_out) return 0;
  if (!kn.wide || g.im_kw != 0 || g.res || g.y2) return 0;
  if (g.K != g.KS * 32 || (g.KS != 4 && g.KS != 8 && g.KS != 16 && g.KS != 32)) return 0;
  // dense slabs only: the column space IS the output row (an im2col buffer whose rows are padded to a multiple of 4 has
  // HWX > HWY: its pad columns must not be stored, and the whole-chunk stores would spill into the next row)
  if (g.M < 256 || hwx < 16 || hwx != g.HWY) return 0;
  const int CPI = (hwx + 15) >> 4;
  const long chunks = (long)g.NB * CPI;
  if (chunks * 16 >= ((long)1 << 31) - 4096) return 0;
  const int mblocks = (g.M + 255) / 256;
  int best = 0;
  double best_cost = 1e30;
  const int cands[3] = {4, 7, 8};
  for (int i = 0; i < 3; ++i) {
    const int ntt = cands[i];
    if (kn.wide_force && ntt != kn.wide_force) continue;
    if (g.KS == 32 && ntt != 4) continue;  // K = 1024 is instantiated for 4 n tiles only (the others do not fit the LDS)
    {  // the activation tile + the staging images must fit the LDS
      const int c1 = 2 * ntt > 8 ? 2 * ntt - 8 : 0;
      if ((long)g.KS * 4 * (1024 + c1 * 128) + 8 * 32 * 48 + kn.stamp_lds_wide > 160 * 1024) continue;
    }
    const long nblocks = (chunks + 2 * ntt - 1) / (2 * ntt);
    const long blocks = nblocks * mblocks;
    const long rounds = (blocks + 255) / 256;
    // time ~ rounds x (operand ingest of a tile + a fixed prologue / epilogue share)
    const double cost = (double)rounds * ((double)g.KS * 32 * (256 + 32 * ntt) + 40000.0);
    if (cost < best_cost) {
      best_cost = cost;
      best = ntt;
    }
  }
  return best;
}

// 32-row fragment tiles per wave tile.  The packed layout is a sequence of 32-row tiles, so a layer packed for 2 also runs with 1.
inline int wave_tile_ma(const GemmProblem& g, const GemmKnobs& kn) {
  int ma = g.ma;
  // M <= 128: 64-row tiles would leave waves of the 4-wave block without work
  if (ma == 2 && ((kn.ma == 0 && g.M <= 128 && g.M > 64) || (kn.ma == 1 && g.im_kw == 0))) ma = 1;
  // 64-row tiles whose last tile is at most half full (M = 144: 192 rows computed and stored-checked for 144), and the
  // streaming shapes with K <= 64 and M > 64 (MobileNetV2's expand convs: 24 -> 144 ran at 3.0 TB/s with 64-row tiles,
  // 3.9 with 32-row ones; 64 -> 384 @14x14 12.1 -> 9.8 us): 32-row wave tiles
  // (K = 32, M = 64 — MobileNetV1's first pointwise conv — too: 28.7 -> 27.4 us at batch 128)
  if (ma == 2 && kn.ma == 0 && g.im_kw == 0 &&
      (((g.M & 63) != 0 && (g.M & 63) <= 32) || (g.KS <= 2 && g.M > 64) || (g.KS == 1 && g.M == 64)))
    ma = 1;
  return ma;
}

}  // namespace gemm_plan_detail

inline GemmPlan gemm_plan(const GemmProblem& g, const GemmKnobs& kn) {
  using namespace gemm_plan_detail;
  GemmPlan p;
  const bool implicit = g.im_kw > 0;
  // dense NCHW slabs whose rows are not a multiple of 4 bytes (HW = 49: the 7x7 layers) arrive with HWX rounded up to 4 for
  // the dword kernels; the kernels that move END-aligned 16-byte pieces (ring, tr, wide) must know the TRUE row length, or
  // the last piece of a row reaches into the next row -- and past the end of the tensor on its last row
  const int hw_true = (!implicit && g.XP > 0 && g.XP < g.HWX) ? g.XP : g.HWX;
  const int HWP = (hw_true + 15) & ~15;  // their 16-byte padded column space
  p.OUT = g.out;

  // third generation (gemm_wide_i8.hip): plain 1x1 GEMMs with M >= 256 and K in {128, 256, 512, 1024}: one 256 x (128..256)
  // tile per CU, the weight panel read once per CU, every operand byte in flight before the first MFMA
  if (!implicit && kn.variant == 0) {
    if (const int ntt = wide_ntt(g, kn, hw_true)) {
      const int c1 = 2 * ntt > 8 ? 2 * ntt - 8 : 0;
      p.family = GEMM_WIDE;
      p.NTT = ntt;
      p.HWX = hw_true;
      p.NT = (int)cdiv((long)g.NB * ((hw_true + 15) >> 4), 2 * ntt);
      p.MT = (g.M + 255) / 256;
      p.grid = grid8(p.MT, p.NT);
      p.block = 512;
      p.lds = (size_t)(g.KS * 4 * (1024 + c1 * 128) + 8 * 32 * 48) + kn.stamp_lds_wide;
      set_name(&p, ntt == 4 ? "gemm_wide_n4" : ntt == 7 ? "gemm_wide_n7" : "gemm_wide_n8");
      return p;
    }
  }

  // The transposed-read ring kernel (gemm_tr_i8.hip) is the implicit-GEMM engine (any M > 32, rows down to 7 columns, stride 2
  // on a phase-split copy).  For plain 1x1 / im2col GEMMs it is opt-in (GEMM_TR = 2): on MobileNetV1's pointwise layers it
  // ties the first-generation ring kernel at batch 128 and loses at batch 256.
  if (g.M > 32 && (implicit || (kn.variant == 0 && kn.tr >= 2))) {
    // rows shorter than 16 bytes: only on the padded copy of the implicit route (a 16-byte piece may run past the row)
    if (kn.tr && g.KS >= 4 && (hw_true >= 16 || implicit) && (long)g.NB * HWP < ((long)1 << 31) - 1024) {
      p.family = GEMM_TR;
      // fp32-output conv whose fp32 value nobody reads and whose only tail is the calib: the staged int8 epilogue (16-byte
      // row stores) instead of the row-per-lane 32-bit one (ResNet50's stem behind the int8 max pool)
      if (g.out == GEMM_OUT_F32 && !g.y && g.y2 && !g.res) p.OUT = GEMM_OUT_I8;
      // TR_CFG 3: 4-wave blocks (128 x 256 / 256 x 128 tiles), two per CU, for every M (ResNet50's 3x3 layers: 5-8 % faster
      // than one 8-wave block per CU, whose waves read LDS together and multiply together); 0 = the 8-wave tiles
      if (g.M > 128) { p.WN = (kn.tr_cfg & 1) ? 1 : 2; p.WM = 4; }
      else if (g.M > 64) { p.WN = (kn.tr_cfg & 2) ? 2 : 4; p.WM = 2; }
      else { p.WN = 4; p.WM = 1; }
      // 4-wave blocks: 3 K-steps in flight = 4 ring slots = 72 KiB, so that TWO blocks share a CU
      p.D = p.WN * p.WM == 4 ? 3 : 4;
      p.IM = implicit;
      const int BN = p.WN * 128, BM = p.WM * 64;
      p.HWX = hw_true;
      p.NT = (int)cdiv((long)g.NB * HWP, BN);  // blocks along N
      p.MT = (g.M + BM - 1) / BM;              // blocks along M
      p.grid = grid8(p.MT, p.NT);
      p.block = 64u * p.WN * p.WM;
      p.lds = (size_t)(p.D + 1) * (BN * 32 + BM * 32) + kn.stamp_lds_tr;
      set_name(&p, p.WM == 4 ? (p.WN == 1 ? "gemm_tr_1x4" : "gemm_tr_2x4") : p.WM == 2 ? (p.WN == 2 ? "gemm_tr_2x2" : "gemm_tr_4x2") : "gemm_tr_4x1");
      return p;
    }
    // stride-2 / short-row implicit GEMMs exist on that kernel ONLY: the first-generation kernels would read outside their
    // operands for these shapes
    if (implicit && (g.im_s == 2 || g.HWX < 16)) return p;
  }

  // first generation (gemm_i8.hip)
  const int MA = wave_tile_ma(g, kn);
  const bool mfull = g.M % (32 * MA) == 0;
  const bool vec_store = g.vec_store && g.aligned_loads;
  p.MA = MA;
  p.MT = (g.M + 32 * MA - 1) / (32 * MA);
  p.block = 256;
  // (32-row wave tiles with a short K -- e.g. 128->128 at 56x56 -- run faster on the register-staged kernel: 24.8 vs 26.6 us)
  const bool ring_merit = g.HWX >= 16 && g.KS >= 4 && (kn.variant == 3 || (kn.variant == 0 && p.MT >= 4 && (MA == 2 || g.KS >= 8)));
  if (implicit || ring_merit) {  // the implicit-GEMM operand exists only in the ring kernel
    if (implicit && (long)g.NB * HWP >= ((long)1 << 31) - 1024) return p;  // its column space is a 32-bit index too
    p.family = GEMM_RING;
    p.on_merit = ring_merit;
    p.VEC_STORE = vec_store;
    p.MFULL = mfull;
    p.HWX = hw_true;
    p.NT = (int)cdiv((long)g.NB * HWP, 128);
    p.grid = grid8((p.MT + 3) / 4, p.NT);
    // straight-line K loop with the A fragments in registers: K = 128 / 256 / 512 / 1024, whole 64-row tiles
    const int ng = (kn.areg && (g.KS & 3) == 0 && mfull && MA == 2) ? g.KS >> 2 : 0;
    p.NG = (ng == 1 || ng == 2 || ng == 4 || ng == 8) ? ng : 0;
    p.lds = (size_t)(4 + 1) * (p.NG ? 4096 : 4096 + 4 * MA * 1024) + 4 * 2 * MA * 32 * 4 + kn.stamp_lds_ring;
    set_name(&p, p.NG ? "gemm_areg" : MA == 2 ? "gemm_ring" : "gemm_ring_ma1");
    return p;
  }
  // the dword kernels: unaligned rows are loaded bytewise-safe and stored element by element; whole tiles skip the row checks
  // only in the vector-store form
  p.ALIGNED = g.aligned_loads;
  p.VEC_STORE = vec_store;
  p.MFULL = vec_store && mfull;
  p.HWX = g.HWX;
  p.NT = (int)cdiv((long)g.NB * g.HWX, 128);
  if (kn.variant == 2 || (kn.variant == 0 && p.MT >= 2 && g.KS >= 2)) {
    p.family = GEMM_LDS;
    p.grid = grid8((p.MT + 3) / 4, p.NT);
    set_name(&p, "gemm_vperm_lds");
  } else {
    p.family = GEMM_PRIVATE;
    p.grid = (unsigned)(((long)p.MT * p.NT + 3) / 4);
    set_name(&p, "gemm_nchw");
  }
  return p;
}

// the plan as one line of text (plhip_debug_gemm_plan, tests/golden/gemm_plans/)
inline int gemm_plan_text(const GemmPlan& p, char* buf, size_t cap) {
  static const char* const fam[] = {"none", "private", "lds", "ring", "tr", "wide"};
  return snprintf(buf, cap, "%s family=%s MA=%d OUT=%d VS=%d MF=%d AL=%d NG=%d WN=%d WM=%d D=%d IM=%d NTT=%d HWX=%d MT=%d NT=%d grid=%u block=%u lds=%zu",
                  p.name, fam[p.family], p.MA, p.OUT, (int)p.VEC_STORE, (int)p.MFULL, (int)p.ALIGNED, p.NG, p.WN, p.WM, p.D, (int)p.IM,
                  p.NTT, p.HWX, p.MT, p.NT, p.grid, p.block, p.lds);
}

}  // namespace plhip
