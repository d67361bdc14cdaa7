// gemm_i8.hip — int8 x int8 -> int32 GEMM on v_mfma_i32_32x32x32_i8 with NCHW-native operands and a fused
// per-channel dequant/requant + bias + activation epilogue.  (The weight pre-pack, im2col and the padded copies: conv_glue_i8.hip;
// which kernel runs a problem: gemm_plan.h.)
//
// Replaces (reference, ARM): gemm_prepack_int8 (lite/backends/arm/math/gemm_prepacked_int8.cc:5263-5457,
// hot loop :2582-2744, epilogue :643-796), packb_int8 (:3285) and the batch/group driver loops of
// conv1x1s1_gemm_int8 / conv_im2col_gemm_int8 (lite/backends/arm/math/conv_impl.cc:260-331, 490-598).
//
// Shape mapping (conv_impl.cc:275-299): per group  Y[b] (M x N) = W (M x K) * X[b] (K x N),
// M = cout/g, K = cin/g*kh*kw, N = oh*ow.  Unlike the reference, the batch is folded into N
// (n = b*HWX + hw) so that late layers (N = 49) still fill whole MFMA tiles.
//
// MI355X design
//   * one wave owns a (32*MA) x 128 output tile: MA A-fragments x 4 B-fragments of the 32x32x32 MFMA,
//     accumulators live in 64*MA VGPRs (VGPR form: the epilogue reads every value);
//   * A (weights) is pre-packed once into MFMA fragment order, so a wave's A fragment is one fully
//     coalesced 1 KiB dwordx4 load served by L2;
//   * B (activations, K x N with N contiguous = NCHW slab) is transposed IN REGISTERS with v_perm_b32 into the
//     K-contiguous 16-byte-per-lane operand the MFMA wants: lane (c = lane&31, h = lane>>5) ends up
//     with, for i = 0..3, column n = 4c+i, k = 16h..16h+15.  MFMA i therefore computes columns
//     {4c+i}, so each lane finishes with 4 CONSECUTIVE n for every output row and the int8 result is
//     stored as one dword per row (32 lanes x 4 B = 128 contiguous bytes of an NCHW row);
//   * three kernels share this scheme and differ in how B reaches the registers:
//       gemm_i8_nchw_kernel  private tiles, no LDS, no barrier (M <= 64 or one K-step: purely streaming layers);
//       gemm_i8_lds_kernel   4 waves split M and share B through LDS in fragment order (register-staged loads);
//       gemm_i8_dma_kernel   LDS-DMA ring (16-byte pieces, counted vmcnt, one barrier per K-step), A through LDS or
//                            (NG > 0) straight into a register ring; also the implicit-GEMM route of dense k x k convs.
//     All of them map block b to the (b % 8)-th eighth of the N tiles (XCD-contiguous work, xcd_tile_map).
// The MFMA's k-slot <-> (lane>>5, byte) map never matters: A and B use the same one.
#include <stdlib.h>

#include "plhip_device.h"
#include "plhip_kernels.h"
#include <type_traits>

#include "gemm_epilogue.h"
#include "dw_common.h"

namespace plhip {

// ALIGNED: every row dword is 4-byte aligned and inside the tensor.  Otherwise (dense slabs with HW % 4 != 0, e.g. the
// 7x7 layers, or a misaligned base) the dwords are read unaligned — legal for global memory on gfx950 — and the one
// dword that would cross the end of the tensor is assembled bytewise.  Columns >= HW of a 4-column group then hold
// bytes of the next row: harmless, a GEMM column only ever feeds its own (discarded) output column.
// XCD-aware tile map of the shared-B kernels.  Workgroups are dealt round-robin over the 8 XCDs (private L2 each), so
// block b runs on XCD b % 8.  (1) The mtb_n blocks that share one B tile get ids equal mod 8 and adjacent in dispatch
// order: the tile crosses the fabric once instead of mtb_n times (FETCH_SIZE was 3.4x the algorithmic bytes on the M = 512
// layers).  (2) Each XCD owns a CONTIGUOUS range of N tiles: a tile's 128-byte row segments are not cache-line aligned
// (row pitch HW = 196, 784, 3136 ...), so neighbouring tiles share most of their cache lines; with neighbours on
// different XCDs every such line was fetched twice (FETCH x2 was still 2.2-2.4x the input bytes after (1)).
__device__ __forceinline__ void xcd_tile_map(int b, int mtb_n, int NT, int& mtb, int& nt) {
  const int ntx = (NT + 7) >> 3;  // N tiles per XCD
  const int x = b & 7, q = b >> 3;
  const int j = q / mtb_n;
  mtb = q - j * mtb_n;
  nt = x * ntx + j;  // >= NT for the padding blocks of the last XCDs: callers return
}

template <bool ALIGNED>
__device__ __forceinline__ void load_b(const int8_t* __restrict__ xb, int ks, int h, int K, int XP, long room, uint32_t (&raw)[16]) {
#pragma unroll
  for (int j = 0; j < 16; ++j) {
    int k = ks * 32 + 16 * h + j;
    k = k < K ? k : K - 1;  // rows >= K meet zero-padded weights; only the address must stay legal
    const long off = (long)k * XP;
    if (ALIGNED) {
      raw[j] = *reinterpret_cast<const uint32_t*>(xb + off);
    } else if (off + 4 <= room) {
      uint32_t v;
      __builtin_memcpy(&v, xb + off, 4);
      raw[j] = v;
    } else {
      uint32_t v = 0;
      for (int i = 0; i < 4; ++i)
        if (off + i < room) v |= (uint32_t)(uint8_t)xb[off + i] << (8 * i);
      raw[j] = v;
    }
  }
}

// the 16 raw row dwords of a lane (K rows 16h .. 16h+15, columns 4c .. 4c+3) -> its four B fragments (fragment i = column 4c+i,
// 16 K-contiguous bytes)
__device__ __forceinline__ void transpose_b16(const uint32_t (&raw)[16], v4i (&bf)[4]) {
#pragma unroll
  for (int jg = 0; jg < 4; ++jg) {
    uint32_t o0, o1, o2, o3;
    transpose4x4_b8(raw[4 * jg], raw[4 * jg + 1], raw[4 * jg + 2], raw[4 * jg + 3], o0, o1, o2, o3);
    bf[0][jg] = (int)o0;
    bf[1][jg] = (int)o1;
    bf[2][jg] = (int)o2;
    bf[3][jg] = (int)o3;
  }
}

// the fields every kernel of this file reads, live in the entry block (PLHIP_PRELOAD, plhip_device.h)
#define PLHIP_PRELOAD_GEMM(g)                                                                                                  \
  PLHIP_PRELOAD(g.wp); PLHIP_PRELOAD(g.x); PLHIP_PRELOAD(g.y); PLHIP_PRELOAD(g.scale); PLHIP_PRELOAD(g.bias);                  \
  PLHIP_PRELOAD(g.M); PLHIP_PRELOAD(g.K); PLHIP_PRELOAD(g.KS); PLHIP_PRELOAD(g.HWX); PLHIP_PRELOAD(g.HWY); PLHIP_PRELOAD(g.XP); \
  PLHIP_PRELOAD(g.NB); PLHIP_PRELOAD(g.x_bstride); PLHIP_PRELOAD(g.y_bstride); PLHIP_PRELOAD(g.MT); PLHIP_PRELOAD(g.NT);       \
  PLHIP_PRELOAD(g.act); PLHIP_PRELOAD(g.alpha)

template <int MA, int OUT, bool VEC_STORE, bool MFULL, bool ALIGNED>
__global__ __launch_bounds__(256, 2) void gemm_i8_nchw_kernel(GemmArgs g) {
  PLHIP_PRELOAD_GEMM(g);
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);  // wave-uniform for the compiler too
  const uint32_t wid = blockIdx.x * 4u + (uint32_t)wave;  // MT * NT < 2^31 (launcher)
  if (wid >= (uint32_t)g.MT * (uint32_t)g.NT) return;  // wave-uniform; the kernel uses no barrier
  const int nt = (int)(wid / (uint32_t)g.MT);
  const int mt = (int)(wid - (uint32_t)nt * (uint32_t)g.MT);
  __shared__ __attribute__((aligned(16))) float lsb_all[4][2 * MA * 32];
  float* lsb = lsb_all[wave];
  const int c = lane & 31, h = lane >> 5;
  const int ntot = g.NB * g.HWX;  // multiple of 4 by construction

  int n4 = nt * 128 + 4 * c;
  const bool nvalid = n4 < ntot;
  if (!nvalid) n4 = 0;
  const int b = n4 / g.HWX;
  const int hw = n4 - b * g.HWX;
  const int8_t* xb = g.x + (size_t)b * g.x_bstride + hw;
  const long room = g.x_bytes - ((long)b * (long)g.x_bstride + hw);  // bytes from xb to the end of the tensor

  v16i acc[MA][4];  // first written by K-step 0 (zero addend): no separate zeroing of the 64*MA registers
  uint32_t raw[16];
  v4i af[MA];
  load_b<ALIGNED>(xb, 0, h, g.K, g.XP, room, raw);
  load_a<MA>(g.wp, mt, g.KS, 0, lane, af);
  float my_s = 1.f, my_b = 0.f;  // this lane's share of the tile's scale / bias, issued behind the first operand loads
  if (OUT != OUT_I32) load_scale_bias<MA>(g, mt, lane, my_s, my_b);

  auto kbody = [&](int ks, auto first_c) {
    constexpr bool FIRST = decltype(first_c)::value;
    v4i bf[4];
    transpose_b16(raw, bf);
    v4i ac[MA];
#pragma unroll
    for (int a = 0; a < MA; ++a) ac[a] = af[a];
    if (ks + 1 < g.KS) {  // prefetch the next K-step under this step's MFMAs
      load_b<ALIGNED>(xb, ks + 1, h, g.K, g.XP, room, raw);
      load_a<MA>(g.wp, mt, g.KS, ks + 1, lane, af);
    }
    const v16i zero = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
    for (int a = 0; a < MA; ++a)
#pragma unroll
      for (int i = 0; i < 4; ++i)
        acc[a][i] = __builtin_amdgcn_mfma_i32_32x32x32_i8(ac[a], bf[i], FIRST ? zero : acc[a][i], 0, 0, 0);
  };
  kbody(0, std::integral_constant<bool, true>{});
  for (int ks = 1; ks < g.KS; ++ks) kbody(ks, std::integral_constant<bool, false>{});

  if (OUT != OUT_I32) store_scale_bias<MA, OUT>(lsb, lane, my_s, my_b);
  if (!nvalid) return;
  gemm_epilogue_act<MA, OUT, VEC_STORE, MFULL>(g, acc, mt, h, b, hw, lsb, g.HWY - hw);
}

// =====================================================================================================================
// LDS-shared variant for M >= 128: a 256-thread block owns a (4 * 32*MA) x 128 tile; its 4 waves split M and SHARE the
// B tile.  Per stage (4 K-steps = 128 k) wave w fetches + transposes K-step w of the stage (16 coalesced dword loads,
// 32 v_perm) and writes its four 1-KiB MFMA fragments to LDS in fragment order (ds_write_b128, conflict free); after
// ONE barrier per stage every wave reads all 16 fragments back (ds_read_b128, lane-linear) for its own 4*MA MFMAs per
// K-step.  B therefore crosses L2 -> CU once per block instead of once per wave (4x less), LDS is double buffered
// (2 x 16 KiB) and the next stage's global loads are in flight under the current stage's MFMAs.  A fragments stay
// private (fragment-ordered, one coalesced 1-KiB load each) and are prefetched two K-steps ahead in a 4-deep
// register ring with static indices.
template <int MA, int OUT, bool VEC_STORE, bool MFULL, bool ALIGNED>
__global__ __launch_bounds__(256, 2) void gemm_i8_lds_kernel(GemmArgs g) {
  PLHIP_PRELOAD_GEMM(g);
  __shared__ __attribute__((aligned(16))) v4i bs[2][4][4][64];  // [buf][kstep][i][lane] : 32 KiB
  __shared__ __attribute__((aligned(16))) float lsb_all[4][2 * MA * 32];
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int mtb_n = (g.MT + 3) >> 2;  // blocks along M
  int mtb, nt;
  xcd_tile_map(blockIdx.x, mtb_n, g.NT, mtb, nt);
  if (nt >= g.NT) return;  // block-uniform (grid is padded to 8 N-tiles)
  const int mt = mtb * 4 + wave;
  const bool mactive = mt < g.MT;  // wave-uniform; inactive waves still load their share of B and hit the barriers
  const int mtc = mactive ? mt : g.MT - 1;
  float* lsb = lsb_all[wave];
  const int c = lane & 31, h = lane >> 5;
  const int ntot = g.NB * g.HWX;

  int n4 = nt * 128 + 4 * c;
  const bool nvalid = n4 < ntot;
  if (!nvalid) n4 = 0;
  const int b = n4 / g.HWX;
  const int hw = n4 - b * g.HWX;
  const int8_t* xb = g.x + (size_t)b * g.x_bstride + hw;
  const long room = g.x_bytes - ((long)b * (long)g.x_bstride + hw);

  v16i acc[MA][4];  // first written by K-step 0 (zero addend)

  const int KS = g.KS;
  const int S = (KS + 3) >> 2;
  uint32_t raw[16];
  v4i a0[MA], a1[MA], a2[MA], a3[MA];

  auto stage_write = [&](int buf) {  // transpose raw (this wave's K-step) into 4 fragments of bs[buf][wave]
    v4i bf[4];
    transpose_b16(raw, bf);
#pragma unroll
    for (int i = 0; i < 4; ++i) bs[buf][wave][i][lane] = bf[i];
  };
  auto kstep_t = [&](int buf, int kk, const v4i (&af)[MA], auto first_c) {
    constexpr bool FIRST = decltype(first_c)::value;
    const v16i zero = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    v4i bf[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) bf[i] = bs[buf][kk][i][lane];
#pragma unroll
    for (int a = 0; a < MA; ++a)
#pragma unroll
      for (int i = 0; i < 4; ++i)
        acc[a][i] = __builtin_amdgcn_mfma_i32_32x32x32_i8(af[a], bf[i], FIRST ? zero : acc[a][i], 0, 0, 0);
  };
  auto kstep = [&](int buf, int kk, const v4i (&af)[MA]) { kstep_t(buf, kk, af, std::integral_constant<bool, false>{}); };
  auto load_a_c = [&](int ks, v4i (&af)[MA]) {  // clamped: K-steps past the end reload the last one (never used)
    load_a<MA>(g.wp, mtc, KS, ks < KS ? ks : KS - 1, lane, af);
  };

  // prologue: stage 0 into LDS, A ring primed with K-steps 0 and 1
  if (wave < KS) load_b<ALIGNED>(xb, wave, h, g.K, g.XP, room, raw);
  load_a_c(0, a0);
  load_a_c(1, a1);
  float my_s = 1.f, my_b = 0.f;
  if (OUT != OUT_I32) load_scale_bias<MA>(g, mtc, lane, my_s, my_b);
  if (wave < KS) stage_write(0);
  __syncthreads();

  for (int s = 0; s < S; ++s) {
    const int buf = s & 1;
    const int ks0 = 4 * s;
    const bool more = s + 1 < S;
    const int myks = ks0 + 4 + wave;  // the K-step this wave stages for the next round
    if (more && myks < KS) load_b<ALIGNED>(xb, myks, h, g.K, g.XP, room, raw);
    // 4 K-steps, A ring: slot kk holds K-step ks0+kk; refill two steps ahead
    load_a_c(ks0 + 2, a2);
    if (mactive) {
      if (s == 0) kstep_t(buf, 0, a0, std::integral_constant<bool, true>{});  // uniform
      else kstep(buf, 0, a0);
    }
    load_a_c(ks0 + 3, a3);
    if (mactive && ks0 + 1 < KS) kstep(buf, 1, a1);
    load_a_c(ks0 + 4, a0);
    if (mactive && ks0 + 2 < KS) kstep(buf, 2, a2);
    load_a_c(ks0 + 5, a1);
    if (mactive && ks0 + 3 < KS) kstep(buf, 3, a3);
    if (more && myks < KS) stage_write(buf ^ 1);
    __syncthreads();
  }

  if (OUT != OUT_I32) store_scale_bias<MA, OUT>(lsb, lane, my_s, my_b);
  if (!nvalid || !mactive) return;
  gemm_epilogue_act<MA, OUT, VEC_STORE, MFULL>(g, acc, mt, h, b, hw, lsb, g.HWY - hw);
}

// =====================================================================================================================
// timeline stamps of the LDS-DMA kernel (EXPERIMENTS=1 builds, plhip_device.h): per wave, kept in LDS during the run and
// flushed to the "gemm" stamp buffer [block < 1024][wave 4][STAMP_SLOTS] at the end (tools/gemm_timeline.py)
constexpr int STAMP_SLOTS = 32;
constexpr size_t STAMP_LDS = kStamps ? 4 * STAMP_SLOTS * 8 : 0;

// LDS-DMA ring variant (the fast path for MFMA-heavy layers: M >= 256-ish, K >= 128, 4-byte aligned rows).
// PMC on the register-staged kernel showed MFMA busy ~13 % per wave and one full memory latency per stage: register
// staging cannot keep enough K-steps in flight (VGPR-bound), and the in-order vmcnt couples the short A loads to the
// long B loads.  Here NOTHING in the K loop loads into VGPRs from global memory:
//   * per K-step the block needs a raw B slab (32 k-rows x 128 columns = 4 KiB, NCHW rows as they lie in memory) and
//     each wave its own MA fragment-ordered A tiles (1 KiB each).  Both are fetched by LDS-DMA
//     (global_load_lds dword / dwordx4): asynchronous, no VGPRs, D-1 K-steps in flight per wave in an NS-slot ring;
//   * a wave waits with a COUNTED s_waitcnt vmcnt for its own share of K-step ks, one raw s_barrier makes the whole
//     slot visible, then every wave reads the raw rows (16 ds_read_b32), transposes them in registers (32 v_perm) and
//     reads its A tiles (ds_read_b128) for 4*MA MFMAs.  The transposes are redundant across the 4 waves but run on the
//     VALU beside the MFMA pipe (128 of 256 MFMA cycles per K-step at MA = 2).
// One barrier per K-step; slot reuse distance NS - (D-1) = 2 iterations, so a slot is rewritten only after every wave
// has passed the barrier that follows its last read.

template <int N>
__device__ __forceinline__ void wait_vmcnt() {
  asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory");
}

// GD_D = K-steps in flight (including the one being consumed); ring slots GD_NS = GD_D + 1.
// AREG: the A fragments go straight from L2 into a 4-deep REGISTER ring (they are already in fragment order in memory) and
// never touch LDS: per block and K-step the LDS sees 20 KB (4 KB of B written once, read by 4 waves) instead of 36 KB --
// with two blocks per CU the old traffic alone (72 KB / 128 B per clock = 562 cycles) exceeded the MFMA time of a K-step
// pair (512).  Needs KS % 4 == 0 (static register names: the loop is unrolled by the ring size).
// NG = KS / 4 as a template constant: the K loop is then straight-line code.  With a loop back-edge the compiler cannot
// count the vector-memory operations in flight and protects the loop-carried fragment registers with s_waitcnt vmcnt(0)
// at the top of every group, which drains the whole pipeline.  NG == 0: A through LDS (any KS).
template <int MA, int OUT, bool VEC_STORE, bool MFULL, int GD_D, int NG>
__global__ __launch_bounds__(256, GD_D <= 4 ? 2 : 1) void gemm_i8_dma_kernel(GemmArgs g) {
  constexpr bool AREG = NG > 0;
  PLHIP_PRELOAD_GEMM(g);
  PLHIP_PRELOAD(g.im_kw); PLHIP_PRELOAD(g.im_khkw); PLHIP_PRELOAD(g.im_c); PLHIP_PRELOAD(g.im_ph); PLHIP_PRELOAD(g.im_pw); PLHIP_PRELOAD(g.im_oh);
  constexpr int GD_NS = GD_D + 1;
  constexpr int SLOT = AREG ? 4096 : 4096 + 4 * MA * 1024;
  constexpr int PER = 1 + MA;  // vector-memory instructions per wave per K-step (1 B piece + MA A fragments)
  extern __shared__ __attribute__((aligned(16))) uint8_t ring[];  // GD_NS * SLOT ring + 4 waves x scale/bias (ONE LDS object)
  typedef __attribute__((address_space(3))) void* lds_ptr;
  typedef const __attribute__((address_space(1))) void* glb_ptr;
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int mtb_n = (g.MT + 3) >> 2;
  int mtb, nt;
  xcd_tile_map(blockIdx.x, mtb_n, g.NT, mtb, nt);
  if (nt >= g.NT) return;  // block-uniform (grid is padded to 8 N-tiles)
  const int mt = mtb * 4 + wave;
  const bool mactive = mt < g.MT;
  const int mtc = mactive ? mt : g.MT - 1;
  const int c = lane & 31, h = lane >> 5;
  // Column space: every image's HWX columns are padded to HWP = roundup(HWX, 16) so that the B tile moves as 16-byte
  // pieces (ONE 1-KiB LDS-DMA instruction per wave and K-step instead of four 256-byte ones: the loop was bound by the
  // number of vector-memory instructions, not by bytes).  The last piece of an image is END-aligned (source columns
  // HWX-16 .. HWX-1), so nothing is read outside the plane; its first 16-r columns duplicate earlier ones and are
  // never stored (r = HWX % 16; with HWX % 4 != 0 one lane per image holds both kinds: `skip`).  Neither the rows nor
  // the pieces need any alignment: LDS-DMA takes byte-aligned global addresses (tools/probe_dma_unaligned.hip).
  const int HWP = (g.HWX + 15) & ~15, full16 = g.HWX & ~15, rem16 = g.HWX & 15;
  int n4 = nt * 128 + 4 * c;
  int b = n4 / HWP;
  int j = n4 - b * HWP;
  // lane's columns j .. j+3: real if below full16, or (last piece) from column HWP - rem16 on; `skip` leading duplicates
  int skip = j < full16 ? 0 : HWP - rem16 - j;
  skip = skip < 0 ? 0 : skip;
  const bool nvalid = b < g.NB && skip < 4;
  if (!nvalid) { b = 0; j = 0; skip = 0; }
  int hw = j < full16 ? j : j + rem16 - 16;
  const bool implicit = g.im_kw > 0;  // wave-uniform
  if (implicit) {  // "image" = output row (batch image, oh): the epilogue wants the batch image and hw = oh*OW + column
    const int bi = b / g.im_oh;
    hw += (b - bi * g.im_oh) * g.HWX;
    b = bi;
  }
  // my 16-byte piece of the B tile: row 8*wave + lane/8 of the K-step, columns 16*(lane&7) ...
  const int prow = 8 * wave + (lane >> 3);
  const int8_t* xb;
  {
    const int np = nt * 128 + 16 * (lane & 7);
    int pb = np / HWP;
    int pj = np - pb * HWP;
    if (pb >= g.NB) { pb = 0; pj = 0; }
    const int pcol = pj < full16 ? pj : g.HWX - 16;
    if (implicit) {
      const int bi = pb / g.im_oh, oh = pb - bi * g.im_oh;
      xb = g.x + ((size_t)bi * g.im_c * g.im_ph + oh) * g.im_pw + pcol;
    } else {
      xb = g.x + (size_t)pb * g.x_bstride + pcol;
    }
  }
  // implicit GEMM: (channel, tap) of this lane's K-row, advanced by 32 rows per issued K-step (issue() is called with
  // consecutive K-steps), so that no division sits in the loop
  int kc = 0, krs = 0;
  if (implicit) {
    kc = prow / g.im_khkw;
    krs = prow - kc * g.im_khkw;
  }
  const int kc_step = implicit ? 32 / g.im_khkw : 0, krs_step = implicit ? 32 - kc_step * g.im_khkw : 0;
  const int8_t* ab = g.wp + (size_t)mtc * MA * g.KS * 1024 + lane * 16;
  const int KS = g.KS;
  float* lsb = reinterpret_cast<float*>(ring + GD_NS * SLOT) + wave * 2 * MA * 32;
  unsigned long long* const gstamp = PLHIP_STAMPS_OF(g);
  const bool diag = kStamps && gstamp;
  unsigned long long* lstamp = reinterpret_cast<unsigned long long*>(ring + GD_NS * SLOT + 4 * 2 * MA * 32 * 4) + wave * STAMP_SLOTS;
  PLHIP_STAMP_REAL(0);
  PLHIP_STAMP(1);
  PLHIP_STAMP_CLOCK(2, (unsigned long long)__builtin_amdgcn_s_getreg(63492) | ((unsigned long long)__builtin_amdgcn_s_getreg(63508) << 32));

  auto issue = [&](int ks, int slot) {
    uint8_t* sb = ring + slot * SLOT;
    size_t koff;
    if (implicit) {
      // rows past K meet zero-padded weights: any in-bounds address will do (the last real tap)
      const int c = kc < g.im_c ? kc : g.im_c - 1, rs = kc < g.im_c ? krs : g.im_khkw - 1;
      const int r = (rs * ((65536 + g.im_kw - 1) / g.im_kw)) >> 16;  // rs / kw, exact for rs < 128, kw <= 11
      koff = ((size_t)c * g.im_ph + r) * g.im_pw + (rs - r * g.im_kw);
      kc += kc_step;
      krs += krs_step;
      if (krs >= g.im_khkw) {
        krs -= g.im_khkw;
        ++kc;
      }
    } else {
      int k = ks * 32 + prow;
      k = k < g.K ? k : g.K - 1;  // rows past K meet zero-padded weights
      koff = (size_t)k * g.XP;
    }
    __builtin_amdgcn_global_load_lds((glb_ptr)(xb + koff), (lds_ptr)(sb + wave * 1024), 16, 0, 0);
    if (!AREG) {
#pragma unroll
      for (int a = 0; a < MA; ++a)
        __builtin_amdgcn_global_load_lds((glb_ptr)(ab + ((size_t)a * KS + ks) * 1024), (lds_ptr)(sb + 4096 + (wave * MA + a) * 1024), 16, 0, 0);
    }
  };
  // AREG: fragment order in memory == register layout.  The load is issued through inline asm ON PURPOSE: next to LDS-DMA
  // operations the compiler's wait-count pass protects every register written by an ordinary load with
  // s_waitcnt vmcnt(0) (seen in the ISA even in straight-line code), which would drain the whole DMA pipeline at each
  // first use.  The asm load is invisible to that pass; the counted waits of the pipeline (wait_vmcnt, in-order vmcnt)
  // already guarantee that K-step ks's fragments have arrived one iteration before they are multiplied.  The price is a
  // build-time obligation: no register copy of an in-flight fragment may be inserted between the load and its MFMAs --
  // the parity suite (random operands) fails on any such copy, and tools/check_areg_isa.py checks the ISA.
  auto load_a_regs = [&](int ks, v4i (&dst)[MA]) {
#pragma unroll
    for (int a = 0; a < MA; ++a) {
      const int8_t* p = ab + ((size_t)a * KS + ks) * 1024;
      asm volatile("global_load_dwordx4 %0, %1, off" : "=v"(dst[a]) : "v"(p) : "memory");
    }
  };

  // ---- pipeline ----
  // Ring of GD_NS = GD_D + 1 slots, AHEAD = GD_D K-steps in flight.  Iteration ks:
  //   wait(my pieces of K-step ks+1 landed) ; barrier ; issue the LDS reads of K-step ks+1 (raw B rows + my A fragments) ;
  //   MFMAs of K-step ks from registers, and IN THEIR SHADOW: the DMA of K-step ks+AHEAD (its slot held K-step ks-1,
  //   which every wave finished reading before this barrier), then the 32 v_perm that turn the raw rows of ks+1 into B
  //   fragments.  An in-order wave stalls at the first consumer of an LDS read, so the first MFMAs carry the DMA issue
  //   and the transposes start only after them (timeline stamps: the former order -- waitcnt lgkmcnt(0) in front of the
  //   first MFMA, DMA issue and a run-time vmcnt switch in front of the barrier -- cost ~1190 cycles per K-step for
  //   256 cycles of MFMA).
  constexpr int AHEAD = GD_D;
  // prologue: K-steps 0 .. AHEAD-1 in flight (the launcher guarantees KS >= AHEAD); the accumulators are zeroed
  // behind the issue, while the first bytes travel
  v4i aring[AREG ? 4 : 1][MA];
  static_assert(!AREG || GD_D == 4, "the register ring is as deep as the DMA look-ahead");
#pragma unroll
  for (int p = 0; p < AHEAD; ++p) {
    issue(p, p);
    if (AREG) load_a_regs(p, aring[AREG ? p : 0]);
  }
  float my_s = 1.f, my_b = 0.f;
  if (OUT != OUT_I32) load_scale_bias<MA>(g, mtc, lane, my_s, my_b);  // 2 more vmcnt entries, younger than the prologue DMA
  __builtin_amdgcn_sched_barrier(0);
  v16i acc[MA][4];
  if (!AREG) {  // AREG: straight-line K loop, K-step 0 multiplies into a zero addend instead (no 64*MA v_mov)
#pragma unroll
    for (int a = 0; a < MA; ++a)
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[a][i][r] = 0;
  }

  auto read_slot = [&](int slot, uint32_t (&raw)[16], v4i (&af)[MA]) {
    const uint8_t* sb = ring + slot * SLOT;
#pragma unroll
    for (int j = 0; j < 16; ++j) raw[j] = *reinterpret_cast<const uint32_t*>(sb + (16 * h + j) * 128 + 4 * c);
    if (!AREG) {
#pragma unroll
      for (int a = 0; a < MA; ++a) af[a] = *reinterpret_cast<const v4i*>(sb + 4096 + (wave * MA + a) * 1024 + lane * 16);
    }
  };

  PLHIP_STAMP(3);
  uint32_t raw[16];
  v4i af_cur[MA], af_nxt[MA], bf_cur[4], bf_nxt[4];
  // K-step 0 into registers: AHEAD-1 younger K-steps of PER pieces each.  The scale / bias loads behind them are NOT
  // counted: there are 0, 1 or 2 of them (no bias pointer, int32 output), and a count that is too high by one lets the
  // wave run ahead of its own last piece (seen as an intermittent wrong 32-row tile); too low only waits a little longer.
  wait_vmcnt<(AHEAD - 1) * PER>();
  __builtin_amdgcn_s_barrier();
  read_slot(0, raw, af_cur);
  transpose_b16(raw, bf_cur);

  // one iteration; YOUNGER = my K-steps issued after ks+1 that may still be in flight at the wait, ISSUE / NEXT: whether
  // K-step ks+AHEAD / ks+1 exists (compile-time in the steady state and in the peeled tail)
  int rslot = 1, islot = AHEAD % GD_NS;
  const v16i zero16 = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
  auto step = [&](int ks, auto younger_c, auto issue_c, auto next_c, auto ring_c, auto first_c) {
    constexpr bool FIRST = decltype(first_c)::value;  // K-step 0 of the straight-line (AREG) loop
    constexpr int RI = AREG ? decltype(ring_c)::value : 0;  // AREG: K-step ks lives in aring[ks % 4]
    constexpr int YOUNGER = decltype(younger_c)::value;
    constexpr bool ISSUE = decltype(issue_c)::value;
    constexpr bool NEXT = decltype(next_c)::value;
    if (ks < STAMP_SLOTS - 8) PLHIP_STAMP(4 + ks);
    if (NEXT) {
      wait_vmcnt<YOUNGER * PER>();
      __builtin_amdgcn_s_barrier();  // K-step ks+1 complete for everyone; nobody reads K-step ks-1's slot any more
      read_slot(rslot, raw, af_nxt);
      rslot = rslot + 1 == GD_NS ? 0 : rslot + 1;
    }
    if (ISSUE) {
      issue(ks + AHEAD, islot);
      islot = islot + 1 == GD_NS ? 0 : islot + 1;
    }
#pragma unroll
    for (int a = 0; a < MA; ++a)
#pragma unroll
      for (int i = 0; i < 4; ++i)
        acc[a][i] = __builtin_amdgcn_mfma_i32_32x32x32_i8(AREG ? aring[RI][a] : af_cur[a], bf_cur[i],
                                                          (AREG && FIRST) ? zero16 : acc[a][i], 0, 0, 0);
    if (NEXT) transpose_b16(raw, bf_nxt);
    // schedule: [MFMA + one DMA piece] x (pieces issued here), bare MFMAs, then the remaining MFMAs share the transposes
    constexpr int NM = 4 * MA;
    constexpr int NDMA = AREG ? 1 : PER;  // LDS-DMA pieces issued among the first MFMAs
    constexpr int LEAD = PER;             // MFMAs in front of the first transpose (LDS read latency)
#pragma unroll
    for (int q = 0; q < LEAD; ++q) {
      __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
      if (ISSUE && q < NDMA) __builtin_amdgcn_sched_group_barrier(0x002, 2, 0);  // address arithmetic of the piece
      if (ISSUE && q < NDMA) __builtin_amdgcn_sched_group_barrier(0x010, 1, 0);
    }
#pragma unroll
    for (int q = LEAD; q < NM; ++q) {
      __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
      __builtin_amdgcn_sched_group_barrier(0x002, (32 + NM - LEAD - 1) / (NM - LEAD), 0);
    }
    // AREG: the fragments of K-step ks+AHEAD replace the ones just consumed.  At the END of the step: an asm statement
    // closes the scheduling region, and the MFMA / v_perm interleave above must stay in one region.
    if (AREG && ISSUE) load_a_regs(ks + AHEAD, aring[RI]);
    if (NEXT) {
#pragma unroll
      for (int i = 0; i < 4; ++i) bf_cur[i] = bf_nxt[i];
      if (!AREG) {
#pragma unroll
        for (int a = 0; a < MA; ++a) af_cur[a] = af_nxt[a];
      }
    }
  };
  using std::integral_constant;
  typedef integral_constant<bool, true> T_;
  typedef integral_constant<bool, false> F_;
  if (AREG) {
    // unrolled by the ring size: K-step ks uses aring[ks % 4]; KS == 4 * NG, so the last group is the peeled tail
    int ks = 0;
    // (the very first step multiplies into a zero addend: FIRST)
    if (NG > 1) {
      step(0, integral_constant<int, 2>{}, T_{}, T_{}, integral_constant<int, 0>{}, T_{});
      step(1, integral_constant<int, 2>{}, T_{}, T_{}, integral_constant<int, 1>{}, F_{});
      step(2, integral_constant<int, 2>{}, T_{}, T_{}, integral_constant<int, 2>{}, F_{});
      step(3, integral_constant<int, 2>{}, T_{}, T_{}, integral_constant<int, 3>{}, F_{});
      ks = 4;
    }
#pragma unroll
    for (int gi = 1; gi + 1 < NG; ++gi, ks += 4) {
      step(ks, integral_constant<int, 2>{}, T_{}, T_{}, integral_constant<int, 0>{}, F_{});
      step(ks + 1, integral_constant<int, 2>{}, T_{}, T_{}, integral_constant<int, 1>{}, F_{});
      step(ks + 2, integral_constant<int, 2>{}, T_{}, T_{}, integral_constant<int, 2>{}, F_{});
      step(ks + 3, integral_constant<int, 2>{}, T_{}, T_{}, integral_constant<int, 3>{}, F_{});
    }
    if (NG > 1) step(ks, integral_constant<int, 2>{}, F_{}, T_{}, integral_constant<int, 0>{}, F_{});
    else step(ks, integral_constant<int, 2>{}, F_{}, T_{}, integral_constant<int, 0>{}, T_{});
    step(ks + 1, integral_constant<int, 1>{}, F_{}, T_{}, integral_constant<int, 1>{}, F_{});
    step(ks + 2, integral_constant<int, 0>{}, F_{}, T_{}, integral_constant<int, 2>{}, F_{});
    step(ks + 3, integral_constant<int, 0>{}, F_{}, F_{}, integral_constant<int, 3>{}, F_{});
  } else {
    const int kmain = KS - AHEAD;
    for (int ks = 0; ks < kmain; ++ks) step(ks, integral_constant<int, AHEAD - 2>{}, T_{}, T_{}, integral_constant<int, 0>{}, F_{});
    // peeled tail: K-steps KS-AHEAD .. KS-1, nothing left to issue, the in-flight count shrinks
    static_assert(AHEAD >= 2 && AHEAD <= 8, "tail is written for 2..8 K-steps ahead");
    int ks = KS - AHEAD;
#define PLHIP_TAIL(T)                                                                                                    \
  if (AHEAD - 1 > T) {                                                                                                   \
    step(ks, integral_constant<int, (AHEAD - 2 - T > 0 ? AHEAD - 2 - T : 0)>{}, F_{}, T_{}, integral_constant<int, 0>{}, F_{}); \
    ++ks;                                                                                                                \
  }
    PLHIP_TAIL(0) PLHIP_TAIL(1) PLHIP_TAIL(2) PLHIP_TAIL(3) PLHIP_TAIL(4) PLHIP_TAIL(5) PLHIP_TAIL(6)
#undef PLHIP_TAIL
    step(ks, integral_constant<int, 0>{}, F_{}, F_{}, integral_constant<int, 0>{}, F_{});
  }

  if (OUT != OUT_I32) store_scale_bias<MA, OUT>(lsb, lane, my_s, my_b);
  PLHIP_STAMP(STAMP_SLOTS - 4);
  if (nvalid && mactive) gemm_epilogue_act<MA, OUT, VEC_STORE, MFULL>(g, acc, mt, h, b, hw, lsb, g.HWY - hw, skip);
  if (diag) {  // wave-uniform
    PLHIP_STAMP(STAMP_SLOTS - 3);  // epilogue instructions issued
    wait_vmcnt<0>();
    PLHIP_STAMP(STAMP_SLOTS - 2);  // stores acknowledged
    PLHIP_STAMP_REAL(STAMP_SLOTS - 1);
    if (blockIdx.x < 1024 && lane < STAMP_SLOTS) gstamp[((size_t)blockIdx.x * 4 + wave) * STAMP_SLOTS + lane] = lstamp[lane];
  }
}

// ---- host side: launch_gemm_i8 plans (gemm_plan.h) and executes; called from plhip_capi_conv.hip ----
static int g_wide_ntt_override = -1;  // tests / A-B runs: plhip_debug_wide_ntt (-1 = the knob WIDE_NTT or automatic)
void debug_set_wide_ntt(int v) { g_wide_ntt_override = v; }

GemmKnobs gemm_knobs() {
  GemmKnobs k;
  k.variant = knob("GEMM_VARIANT", k.variant);
  k.areg = knob("GEMM_AREG", k.areg);
  k.ma = knob("GEMM_MA", k.ma);
  k.tr = knob("GEMM_TR", k.tr);
  k.tr_cfg = knob("TR_CFG", k.tr_cfg);
  k.wide = knob("GEMM_WIDE", k.wide);
  gemm_resolve_wide_force(&k, g_wide_ntt_override, knob("WIDE_NTT", 0));
  k.stamp_lds_ring = (int)STAMP_LDS;
  k.stamp_lds_tr = gemm_tr_stamp_lds();
  k.stamp_lds_wide = gemm_wide_stamp_lds();
  return k;
}

// the first-generation kernels of this file: private tiles, LDS, ring
template <int MA, int OUT>
static void run_gemm_t(const GemmPlan& p, GemmArgs g, hipStream_t s) {
  typedef std::integral_constant<int, 0> F_;
  typedef std::integral_constant<int, 1> T_;
  const dim3 grid(p.grid), block(p.block);
  if (p.family == GEMM_RING) {
    PLHIP_SET_STAMPS(g, "gemm", sizeof(unsigned long long) * 1024 * 4 * STAMP_SLOTS);
    with_const<0, 1>(p.VEC_STORE, [&](auto vs) {
      with_const<0, 1>(p.MFULL, [&](auto mf) {
        constexpr bool VS = decltype(vs)::value != 0, MF = decltype(mf)::value != 0;
        auto launch = [&](auto ng) {
          auto kfn = gemm_i8_dma_kernel<MA, OUT, VS, MF, 4, decltype(ng)::value>;
          if (p.lds > 64 * 1024) (void)hipFuncSetAttribute((const void*)kfn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)p.lds);
          hipLaunchKernelGGL(kfn, grid, block, p.lds, s, g);
        };
        if constexpr (MA == 2 && MF) with_const<0, 1, 2, 4, 8>(p.NG, launch);  // the AREG forms exist for whole 64-row tiles only
        else launch(F_{});
      });
    });
    return;
  }
  auto launch = [&](auto vs, auto mf, auto al) {  // the four store / load forms the dword kernels are built in
    constexpr bool VS = decltype(vs)::value != 0, MF = decltype(mf)::value != 0, AL = decltype(al)::value != 0;
    if (p.family == GEMM_LDS) hipLaunchKernelGGL((gemm_i8_lds_kernel<MA, OUT, VS, MF, AL>), grid, block, 0, s, g);
    else hipLaunchKernelGGL((gemm_i8_nchw_kernel<MA, OUT, VS, MF, AL>), grid, block, 0, s, g);
  };
  if (!p.ALIGNED) launch(F_{}, F_{}, F_{});
  else if (p.MFULL) launch(T_{}, T_{}, T_{});
  else if (p.VEC_STORE) launch(T_{}, F_{}, T_{});
  else launch(F_{}, F_{}, T_{});
}

int launch_gemm_i8(const GemmArgs& g_in, int ma, int out, bool vec_store, bool aligned_loads, hipStream_t s) {
  const GemmPlan p = gemm_plan(gemm_problem(g_in, ma, out, vec_store, aligned_loads), gemm_knobs());
  GemmArgs g = g_in;
  g.HWX = p.HWX;
  g.MT = p.MT;
  g.NT = p.NT;
  switch (p.family) {
    case GEMM_NONE: return -3;
    case GEMM_WIDE: run_gemm_wide(p, g, s); break;
    case GEMM_TR: run_gemm_tr(p, g, s); break;
    default:
      with_const<1, 2>(p.MA, [&](auto ma_c) {
        with_const<OUT_I32, OUT_F32, OUT_I8>(p.OUT, [&](auto out_c) { run_gemm_t<decltype(ma_c)::value, decltype(out_c)::value>(p, g, s); });
      });
  }
  return 0;
}

}  // namespace plhip
