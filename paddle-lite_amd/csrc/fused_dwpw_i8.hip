// fused_dwpw_i8.hip — depthwise 3x3 [int8_out] fused with the pointwise 1x1 convolution that consumes it, ONE launch.
//
// SURVEY.md §8(f) rank 1.  Replaces the instruction pair
//   DepthwiseConv<kInt8,kInt8>::Run (lite/kernels/arm/conv_depthwise.cc:407-446 -> lite/backends/arm/math/conv3x3s1_depthwise_int8.cc:33-447)
//   GemmLikeConv<kInt8,*>::Run      (lite/kernels/arm/conv_gemmlike.cc:399-462 -> lite/backends/arm/math/gemm_prepacked_int8.cc:2582-2744)
// of the MobileNet programs.  Run as two kernels the int8 tensor between them makes a full HBM round trip; here it never
// leaves the CU.  Results are bit-identical to plhip_depthwise_conv_int8 (int8 out) followed by plhip_conv2d_int8.
//
// Round 4: third form.  The two earlier kernels (git history) were K-step synchronous — one barrier per 32
// channels, every wave walking stage -> produce -> consume in lock step — and lost to the two kernels (1.4x).  This one is
// built on the wide-tile GEMM's structure (gemm_wide_kernel.h): the whole K x 128-pixel activation tile is LDS-resident in
// the image ds_read_b64_tr_b8 transposes from, and the DEPTHWISE STAGE IS ITS PRODUCER instead of the LDS-DMA:
//   * tile = (image, half): 7 output rows of a 14-wide plane = 7 chunks of 16 pixels (14 real) = 4 MFMA n tiles, all M
//     output channels: one 8-wave block per CU, 256 tiles at batch 128 = one wave of blocks;
//   * produce task = 16 channels x 4 column quads x the 7-row strip on one wave: the rows-in-registers dot4 body of
//     depthwise3x3_direct_kernel (9 unaligned 8-byte row windows per lane straight from global memory, v_alignbyte +
//     v_dot4_i32_i8, the reference's requantisation), each requantised dword written straight into the activation image;
//     with an int8 output the rows come as two 16-byte-per-lane loads of whole rows through a wave-private LDS stage (FW_RP
//     below), and a lane reads its windows from there: 2 scattered loads per task instead of 9, no v_perm per row;
//   * a ROUND = 8 tasks = 128 channels = 4 K-steps.  While round r is produced (VALU), the 4 K-steps of round r - 1 are
//     multiplied (MFMA, weights global -> registers one round ahead, a wave owns 32 MTW output channels for all 4 n tiles):
//     the two pipes of a SIMD work side by side, one barrier per ROUND (4 for K = 512), the next round's input rows and
//     weights are fetched under the current round's arithmetic;
//   * epilogue: requantise, two v_permlane32_swap give a lane one 14-pixel output row of one channel, the wave's 64 x 98
//     bytes are assembled in LDS and leave as 16-byte pieces of whole channel rows.
// No inline-asm memory operation: every wait count is the compiler's.
#include <stdlib.h>

#include <type_traits>

#include "plhip_device.h"
#include "plhip_kernels.h"
#include "dw_common.h"
#include "gemm_tr_common.h"

namespace plhip {

constexpr int FW_TR = 7;       // output rows per tile
constexpr int FW_NT = 4;       // 32-pixel n tiles per tile (2 rows of pitch 16 each; the second half of the last one is empty)
// (FW_SP, FW_KSTEP: dw_plan.h, which sizes the launch with them)
// The row stage of the int8-output form: a wave's slice of the output staging region (idle until the epilogue) holds the input
// rows of the task being produced, [channel 16][row slot 9][20 B]: a row is stored from column -1 on (bytes 0 and 15 .. 19 are
// zero: the pad columns), so quad q's window is dwords q and q + 1 of its row.  Slot t is strip row t; the slot of the row outside
// the image (0 in the upper half, 8 in the lower one) is never written and stays zero.  52 dwords per channel = 20 (mod 32): the 8
// channels x 4 quads of a half wave read 32 different banks.
constexpr int FW_RP = 20;      // stage: bytes per row slot
constexpr int FW_CP = 208;     // stage: bytes per channel
constexpr int FW_STAGE_AT = 5; // stage: the row chunk of a producing round at which the next task's two pieces are requested
static_assert(16 * FW_CP <= 32 * FW_SP && 16 * FW_CP % 16 == 0, "the row stage lives in one wave's staging slice of the M = 256 form");

// timeline stamps (EXPERIMENTS=1 builds, plhip_device.h): per wave of the first 1024 tiles at the phase boundaries, straight
// into the "fw" stamp buffer [tile][wave 8][FW_STAMP_SLOTS] (tools/fused_timeline.py).  Slots: 0 realtime start, 1 entry,
// 2 operands of round 0 requested, 3 round 0 produced, 4 + 2 (r - 1) round r done, 5 + 2 (r - 1) behind its barrier (r < 5),
// 12 last K-steps multiplied, 13 requantised + staged, 14 stores issued, 15 stores acknowledged
constexpr int FW_STAMP_SLOTS = 16;

// 8 bytes of an input row: scalar base + the lane's 32-bit offset (>= 0) + a compile-time row distance (the immediate of
// the load: no address arithmetic per row)
template <int DELTA>
__device__ __forceinline__ void fw_load_row(const int8_t* __restrict__ xs, uint32_t off, uint32_t (&d)[2]) {
  __builtin_memcpy(d, xs + off + DELTA, 8);
}

// MTW: 32-row m tiles per wave (M = 256 MTW).  OUT: output kind.  DWNN / PWNN: the depthwise / pointwise activation is
// relu or relu6 (the packed non-negative requantisation); else none / leaky (leaky with slope 1 for none: exact).
// R: rounds of 128 input channels, a compile-time constant of the body (the kernel below dispatches on it): which round is the
// first to multiply and which the last to produce is then known where the round is compiled, and every path is straight-line code.
template <int MTW, int OUT, bool DWNN, bool PWNN, int R>
__device__ __forceinline__ void fused_dwpw14_body(const FusedArgs& a) {
  const GemmArgs& g = a.pw;
  PLHIP_PRELOAD(a.x); PLHIP_PRELOAD(a.dw_w); PLHIP_PRELOAD(a.dw_scale); PLHIP_PRELOAD(a.dw_bias); PLHIP_PRELOAD(a.dw_act);
  PLHIP_PRELOAD(a.dw_alpha); PLHIP_PRELOAD(a.n); PLHIP_PRELOAD(a.C); PLHIP_PRELOAD(a.tiles); PLHIP_PRELOAD(a.ones); PLHIP_PRELOAD(g.wp); PLHIP_PRELOAD(g.y);
  PLHIP_PRELOAD(g.scale); PLHIP_PRELOAD(g.bias); PLHIP_PRELOAD(g.M); PLHIP_PRELOAD(g.KS); PLHIP_PRELOAD(g.act); PLHIP_PRELOAD(g.alpha);
  extern __shared__ __attribute__((aligned(16))) uint8_t fw_lds[];  // [activation image KS x 4096][8 waves x 32 MTW rows x FW_SP]
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  // XCD-contiguous tiles: both halves of an image (they share two halo rows) and neighbouring images on one L2
  const unsigned nb = (unsigned)a.tiles, per = (nb + 7) >> 3;
  const unsigned vb = (blockIdx.x & 7) * per + (blockIdx.x >> 3);
  if (vb >= nb) return;  // block-uniform
  const int b = (int)(vb >> 1), hf = (int)(vb & 1);
  unsigned long long* const gstamp = PLHIP_STAMPS_OF(g);
  const bool diag = kStamps && gstamp && vb < 1024;
  unsigned long long* const lstamp = diag ? gstamp + ((size_t)vb * 8 + wave) * FW_STAMP_SLOTS : nullptr;
  PLHIP_STAMP_REAL(0);
  PLHIP_STAMP(1);
  constexpr int KS = 4 * R;  // == g.KS (K % 128 == 0: dwpw_launch_plan)
  const int C = a.C;
  const int c = lane & 31, h = lane >> 5;

  // ------------------------------------------------------------------ producer state
  const int chl = lane >> 2, q = lane & 3;
  // A lane's 8-byte row window never leaves its row (so no load ever leaves the tensor): quad q fetches from column
  // {0, 3, 6, 6}[q] and two v_perm_b32 with per-lane selectors move the bytes to window positions (byte i = input column
  // 4 q - 1 + i), writing zeros (selector 0x0c) for the pad columns -1 and 14 ..: the same 2 VALU per row the masks cost.
  // Rows outside the image (row -1 of the upper half, row 14 of the lower one) are fetched from the neighbouring row
  // and meet a zeroed filter row.
  const uint32_t sel_lo = q == 0 ? 0x0201000cu : (q == 1 ? 0x03020100u : (q == 2 ? 0x04030201u : 0x0c070605u));
  const uint32_t sel_hi = q == 0 ? 0x06050403u : (q == 1 ? 0x07060504u : (q == 2 ? 0x0c070605u : 0x0c0c0c0cu));
  // byte offset of (image b, channel 16 wave + chl, input row 7 hf, the window's fetch column); a round advances it by 128
  // planes.  Strip row t is input row 7 hf - 1 + t: distance 14 (t - 1), an immediate; the two rows that can lie outside
  // the image get their own scalar base (the neighbouring row's address).
  //
  // STAGED (int8 output: the plan has a staging region): the rows come through the wave's row stage instead.  A task's strip is 8
  // rows of the image (0 .. 7 / 6 .. 13) x 16 channels = 128 rows = two wave loads of one 16-byte piece per lane: lane l of
  // load i fetches row 6 hf + (l & 7) of the task's channel 8 i + (l >> 3) from ONE BYTE IN FRONT OF THE ROW, so that what it gets
  // is the stage's row as it stands (column -1 .. 14) and only bytes 0 and 15, which belong to the neighbouring rows, are cleared.
  // Kept inside the tensor: the piece of the tensor's first row would start one byte in front of it: that lane (image 0, channel 0,
  // round 0: the prologue only) fetches from the row's first byte and shifts up; the piece of the tensor's last row would end
  // one byte behind it: that lane (nb1 = 1) fetches from two bytes in front of the row and shifts down, in every round.  Every other
  // row has a whole row on either side.  The row outside the image is not fetched at all: its slot of the stage stays zero.
  constexpr bool STAGED = OUT == OUT_I8;
  const uint32_t stage0 = (uint32_t)(KS * FW_KSTEP + wave * (32 * MTW * FW_SP));  // == stg of the epilogue
  const uint32_t rdb = stage0 + (uint32_t)(chl * FW_CP + 4 * q);                                       // window reads
  const uint32_t wst = stage0 + (uint32_t)((lane >> 3) * FW_CP + ((lane & 7) + 1 - hf) * FW_RP);      // row writes
  const uint32_t xrow = (uint32_t)(((b * C + 16 * wave + (lane >> 3)) * 14 + 6 * hf + (lane & 7)) * 14);  // the loader lane's row, load 0
  // the last byte any of this lane's pieces reaches (load 1 of round R - 1) against the tensor's size: at most one byte over
  const uint32_t nb1 = STAGED && xrow + (uint32_t)(8 * 196 + (R - 1) * (128 * 196) + 15) > (uint32_t)(a.n * C * 196) ? 1u : 0u;
  uint32_t xoff = STAGED ? xrow - 1u - nb1 : (uint32_t)(((b * C + 16 * wave + chl) * 14 + 7 * hf) * 14 + (q == 0 ? 0 : (q == 1 ? 3 : 6)));
  const uint32_t top = hf == 0 ? 0u : 0xffffffffu, bot = hf == 1 ? 0u : 0xffffffffu;  // scalar (block-uniform)
  const int8_t* const xs0 = a.x + (hf == 0 ? 0 : -14);   // strip row 0: input row 7 hf - 1, or row 0 again for the upper half
  const int8_t* const xs8 = a.x + (hf == 1 ? 84 : 98);   // strip row 8: input row 7 hf + 7, or row 13 again for the lower half
  // activation image address of (channel, output row o, quad): k = channel: K-step k / 32, kg = (k % 32) / 8, row k % 8,
  // chunk o in slot o ^ (2 ((k % 8) >> 1)) (the swizzle of gemm_wide_kernel.h), byte 4 q:  address = wbase ^ (o << 4)
  const int ch0 = 16 * wave + chl;
  uint32_t wbase = (uint32_t)((ch0 >> 5) * FW_KSTEP + ((ch0 >> 3) & 3) * 1024 + (ch0 & 7) * 128 + ((ch0 & 6) << 4) + 4 * q);
  // (requant_hi2 / requant_leak, plhip_device.h, written out: through the functions this unit's ISA moves)
  const float dw_hi2 = a.dw_act == ACT_RELU6 ? fminf(a.dw_alpha + a.dw_alpha, 254.f) : 254.f;
  const float dw_leak = a.dw_act == ACT_LEAKY ? a.dw_alpha : 1.f;

  uint32_t in[9][2];   // the 9 input row windows of the task being produced / fetched
  uint32_t wr[3];      // its packed filter rows (w0, w1, w2, 0)
  float dsc, dbi;      // its doubled scale / bias
  auto load_row = [&](auto t_c, uint32_t off, uint32_t (&d)[2]) __attribute__((always_inline)) {
    constexpr int t = decltype(t_c)::value;
    if constexpr (t == 0) fw_load_row<0>(xs0, off, d);
    else if constexpr (t == 8) fw_load_row<0>(xs8, off, d);
    else fw_load_row<14 * (t - 1)>(a.x, off, d);
  };
  auto fetch_task = [&](int ch, uint32_t off) __attribute__((always_inline)) {
    // ch / off: this lane's channel and window offset of the task
    dw_filter_rows3(a.dw_w + (size_t)ch * 9, wr);
    const float s = a.dw_scale[ch], bb = a.dw_bias ? a.dw_bias[ch] : 0.f;
    dsc = s + s;
    dbi = bb + bb;
    load_row(std::integral_constant<int, 0>{}, off, in[0]);
    load_row(std::integral_constant<int, 1>{}, off, in[1]);
    load_row(std::integral_constant<int, 2>{}, off, in[2]);
    load_row(std::integral_constant<int, 3>{}, off, in[3]);
    load_row(std::integral_constant<int, 4>{}, off, in[4]);
    load_row(std::integral_constant<int, 5>{}, off, in[5]);
    load_row(std::integral_constant<int, 6>{}, off, in[6]);
    load_row(std::integral_constant<int, 7>{}, off, in[7]);
    load_row(std::integral_constant<int, 8>{}, off, in[8]);
  };
  // STAGED: the two pieces of the task being fetched (the registers are the stage's second buffer), its parameters
  v4i nx[2];
  auto load_rows = [&](uint32_t off) __attribute__((always_inline)) {
    __builtin_memcpy(&nx[0], a.x + off, 16);
    __builtin_memcpy(&nx[1], a.x + off + 8 * 196, 16);
  };
  auto fetch_params = [&](int ch, uint32_t (&w)[3], float& s, float& bb) __attribute__((always_inline)) {
    dw_filter_rows3(a.dw_w + (size_t)ch * 9, w);
    s = a.dw_scale[ch];
    bb = (a.dw_bias ? a.dw_bias : a.dw_scale)[ch];  // no branch inside a round
    if (!a.dw_bias) bb = 0.f;
  };
  // the pieces into the stage: behind the last window read of the task it holds (the wave's own LDS order: no barrier)
  auto stage_rows = [&]() __attribute__((always_inline)) {
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const uint32_t d0 = (uint32_t)nx[i][0], d1 = (uint32_t)nx[i][1], d2 = (uint32_t)nx[i][2], d3 = (uint32_t)nx[i][3];
      uint32_t* p = reinterpret_cast<uint32_t*>(fw_lds + wst + i * (8 * FW_CP));
      p[0] = __builtin_amdgcn_alignbyte(d1, d0, nb1) & 0xffffff00u;
      p[1] = __builtin_amdgcn_alignbyte(d2, d1, nb1);
      p[2] = __builtin_amdgcn_alignbyte(d3, d2, nb1);
      p[3] = __builtin_amdgcn_alignbyte(0u, d3, nb1) & 0x00ffffffu;
    }
  };

  // ------------------------------------------------------------------ consumer state
  // transposed-read addresses (gemm_wide_kernel.h): tile t <-> chunk pair (2t, 2t+1); lane 2q'+p of a 16-lane group -> row
  // q', sub-chunk p; 16-lane group parity -> chunk parity; k half h -> kg {2h, 2h+1}
  // n tile tt: slot pair 2 (tt ^ (q' >> 1)) + parity: address of tile tt = tr00 ^ (tt << 5) (bits 5-6 hold nothing else)
  uint32_t tr00;
  {
    const int qr = (lane & 15) >> 1, par = (lane >> 4) & 1;
    tr00 = (uint32_t)((h * 2) * 1024 + qr * 128 + ((2 * (qr >> 1) + par) * 16) + (lane & 1) * 8);
  }
  const int mt0 = wave * MTW;  // my first 32-row m tile
  const uint8_t* const wpk = reinterpret_cast<const uint8_t*>(g.wp) + (size_t)mt0 * KS * 1024;  // [mt][ks][64 lanes][16 B]: wave-uniform
  const uint32_t wlane = (uint32_t)lane * 16;
  v4i W[4][MTW];       // weight fragments of the 4 K-steps being multiplied / fetched
  auto fetch_w = [&](int j, int ks) __attribute__((always_inline)) {
#pragma unroll
    for (int m = 0; m < MTW; ++m) W[j][m] = *reinterpret_cast<const v4i*>(wpk + ((size_t)m * KS + ks) * 1024 + wlane);  // scalar base + lane offset
  };
  v16i acc[FW_NT][MTW];  // never zeroed: K-step 0 multiplies into the constant
  const v16i zero16 = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};

  // ------------------------------------------------------------------ one round
  // PRODUCE: the task in (in, wr, dsc, dbi) -> K-steps 4 rp .. 4 rp + 3 of the image, and the next task's operands fetched
  // into the same registers behind their last use.  CONSUME: K-steps 4 rc .. 4 rc + 3 (W) multiplied, the next four fetched.
  // The MFMAs are dealt over the 9 row chunks of the task so that every chunk carries VALU and matrix work side by side.
  using std::integral_constant;
  // A producing round is TAPS FIRST: the 9 row chunks' window cuts and v_dot4 taps with no MFMA between them, then the 7
  // requantisation slices with the round's MFMAs dealt over them.  v_dot4_i32_i8 runs on the matrix pipe: beside an MFMA it
  // waits for it (tools/probe_coexec.hip: one wave's MFMA + 8 fma take 51 cycles, MFMA + 8 dot4 90; a dot4-only wave beside an
  // MFMA-only wave runs at 9.5 cycles per dot4), while cvt / fma / min / perm overlap with it.  (Dealing everything over the
  // row chunks instead made rounds take MFMA time + VALU time, profiles/r04_fused_timeline_order0.txt.)  The consume-only
  // last round deals its MFMAs over the 9 row chunks' proportions.
  // FIRST: the round multiplies K-steps 0 .. 3 (K-step 0 into the constant 0: the accumulators are never zeroed).  LAST: the
  // last producing round requests no next task; the consume-only round behind it requests no weights.  Both are compile-time:
  // there is no branch inside a round.
  auto round = [&](auto produce_c, auto consume_c, auto first_c, auto last_c, int rp, int rc) __attribute__((always_inline)) {
    constexpr bool PRODUCE = decltype(produce_c)::value, CONSUME = decltype(consume_c)::value;
    constexpr bool FIRST = decltype(first_c)::value, LAST = decltype(last_c)::value;
    constexpr bool NEXT_TASK = PRODUCE && !LAST;  // round rp + 1 produces
    constexpr bool NEXT_W = PRODUCE;              // K-steps 4 (rc + 1) .. exist: only the consume-only round multiplies the last four
    const int nch = 128 * (rp + 1) + 16 * wave + chl;
    const uint32_t noff = xoff + (uint32_t)(128 * 196);
    const uint32_t wb = wbase + (uint32_t)rp * (4 * FW_KSTEP);
    const uint32_t rb = (uint32_t)rc * (4 * FW_KSTEP);
    int dacc[FW_TR][4];
    // input row 0 / 8 of the strip lies outside the image in the upper / lower half (STAGED: its slot of the stage is zero)
    const uint32_t wr0t = STAGED ? wr[0] : wr[0] & top, wr2b = STAGED ? wr[2] : wr[2] & bot;
    uint32_t nwr[3];
    float ndsc = 0.f, ndbi = 0.f;
    v2i lo[FW_NT], hi[FW_NT];
    auto read_frag = [&](int j, int n) __attribute__((always_inline)) {
      const uint32_t ta = (tr00 + rb) ^ (uint32_t)(n << 5);
      lo[n] = __builtin_amdgcn_ds_read_tr8_b64_v2i32((lds_v2i_ptr_t)(fw_lds + ta + j * FW_KSTEP));
      hi[n] = __builtin_amdgcn_ds_read_tr8_b64_v2i32((lds_v2i_ptr_t)(fw_lds + ta + j * FW_KSTEP + 1024));
    };
    // MFMA i of the round: K-step j = i / (4 MTW), n tile (i / MTW) % 4, m tile i % MTW
    auto mfma = [&](auto i_c) __attribute__((always_inline)) {
      constexpr int i = decltype(i_c)::value;
      constexpr int j = i / (FW_NT * MTW), n = (i / MTW) % FW_NT, m = i % MTW;
      if constexpr (m == 0) {
        if constexpr (n == 0 && j == 0) {
          read_frag(0, 0);
          read_frag(0, 1);
        }
        // fragments two n tiles ahead
        constexpr int nn = (n + 2) % FW_NT, jn = j + (n + 2) / FW_NT;
        if constexpr (jn < 4) read_frag(jn, nn);
      }
      const v4i av = {lo[n][0], lo[n][1], hi[n][0], hi[n][1]};
      acc[n][m] = __builtin_amdgcn_mfma_i32_32x32x32_i8(av, W[j][m], FIRST && j == 0 ? zero16 : acc[n][m], 0, 0, 0);
      if constexpr (NEXT_W && n == FW_NT - 1 && m == MTW - 1) fetch_w(j, 4 * (rc + 1) + j);  // K-step j done: its registers take K-step j of the next round
    };
    auto mfmas = [&](auto self, auto i_c, auto end_c) __attribute__((always_inline)) -> void {
      constexpr int i = decltype(i_c)::value, end = decltype(end_c)::value;
      if constexpr (i < end) {
        mfma(integral_constant<int, i>{});
        self(self, integral_constant<int, i + 1>{}, integral_constant<int, end>{});
      }
    };
    constexpr int NM = 4 * FW_NT * MTW;  // MFMAs per round and wave: 32 / 16
    // first MFMA of row chunk t (t = 9: end): proportional to the chunk's VALU work (rows 0 / 1 carry no requantisation)
    constexpr auto mstart = [](int t) {
      constexpr int cum[10] = {0, 1, 3, 7, 11, 15, 19, 23, 28, 32};
      return cum[t] * NM / 32;
    };
    auto taps = [&](auto t_c) __attribute__((always_inline)) {
      constexpr int t = decltype(t_c)::value;
      uint32_t e0, e1;
      if constexpr (STAGED) {  // dwords q, q + 1 of the row's slot: one 4-byte aligned two-dword read
        const uint32_t* rp2 = reinterpret_cast<const uint32_t*>(fw_lds + rdb + t * FW_RP);
        e0 = rp2[0];
        e1 = rp2[1];
      } else {
        e0 = __builtin_amdgcn_perm(in[t][1], in[t][0], sel_lo);
        e1 = __builtin_amdgcn_perm(in[t][1], in[t][0], sel_hi);
      }
      uint32_t win[4];
      win[0] = e0;
      win[1] = __builtin_amdgcn_alignbyte(e1, e0, 1);
      win[2] = __builtin_amdgcn_alignbyte(e1, e0, 2);
      win[3] = __builtin_amdgcn_alignbyte(e1, e0, 3);
#pragma unroll
      for (int r = 0; r < 3; ++r) {
        const int o = t - r;
        if (o < 0 || o >= FW_TR) continue;
#pragma unroll
        for (int jj = 0; jj < 4; ++jj)
          dacc[o][jj] = r == 0 ? sdot4_first(win[jj], t == 0 ? wr0t : wr[0])
                               : __builtin_amdgcn_sdot4((int)win[jj], (int)(t == 8 ? wr2b : wr[r]), dacc[o][jj], false);
      }
      if constexpr (NEXT_TASK) {
        // the next task's row t into the registers just consumed; STAGED: its two pieces, once
        if constexpr (!STAGED) load_row(integral_constant<int, t>{}, noff, in[t]);
        else if constexpr (t == FW_STAGE_AT) load_rows(noff);
        if constexpr (t == 2) fetch_params(nch, nwr, ndsc, ndbi);
      }
    };
    auto finish = [&](auto o_c) __attribute__((always_inline)) {  // output row o is complete: requantise, into the image
      constexpr int o = decltype(o_c)::value;
      const uint32_t pk = DWNN ? requant4_nn_rtz(dacc[o], dsc, dbi, dw_hi2, a.ones) : requant4<ACT_LEAKY>(dacc[o], dsc, dbi, dw_leak, -254.f, 254.f);
      *reinterpret_cast<uint32_t*>(fw_lds + (wb ^ (uint32_t)(o << 4))) = pk;
    };
    auto chunk = [&](auto t_c) __attribute__((always_inline)) {  // consume-only round: row chunk t's share of the MFMAs
      constexpr int t = decltype(t_c)::value;
      mfmas(mfmas, integral_constant<int, mstart(t)>{}, integral_constant<int, mstart(t + 1)>{});
      __builtin_amdgcn_sched_barrier(0);
    };
    // first MFMA of requantisation slice o (o = 7: end)
    constexpr auto m1start = [](int o) {
      constexpr int cum[8] = {0, 5, 10, 14, 19, 23, 28, 32};
      return cum[o] * NM / 32;
    };
    auto slice = [&](auto o_c) __attribute__((always_inline)) {  // requantisation slice o with its share of the MFMAs
      constexpr int o = decltype(o_c)::value;
      if constexpr (CONSUME) mfmas(mfmas, integral_constant<int, m1start(o)>{}, integral_constant<int, m1start(o + 1)>{});
      finish(o_c);
      __builtin_amdgcn_sched_barrier(0);
    };
    if constexpr (!PRODUCE) {
      chunk(integral_constant<int, 0>{});
      chunk(integral_constant<int, 1>{});
      chunk(integral_constant<int, 2>{});
      chunk(integral_constant<int, 3>{});
      chunk(integral_constant<int, 4>{});
      chunk(integral_constant<int, 5>{});
      chunk(integral_constant<int, 6>{});
      chunk(integral_constant<int, 7>{});
      chunk(integral_constant<int, 8>{});
    } else {
      taps(integral_constant<int, 0>{});
      taps(integral_constant<int, 1>{});
      taps(integral_constant<int, 2>{});
      taps(integral_constant<int, 3>{});
      taps(integral_constant<int, 4>{});
      taps(integral_constant<int, 5>{});
      taps(integral_constant<int, 6>{});
      taps(integral_constant<int, 7>{});
      taps(integral_constant<int, 8>{});
      __builtin_amdgcn_sched_barrier(0);
      slice(integral_constant<int, 0>{});
      slice(integral_constant<int, 1>{});
      slice(integral_constant<int, 2>{});
      slice(integral_constant<int, 3>{});
      slice(integral_constant<int, 4>{});
      slice(integral_constant<int, 5>{});
      if constexpr (STAGED && NEXT_TASK) {  // every window of this task has been read: the stage takes the next one
        stage_rows();
        __builtin_amdgcn_sched_barrier(0);
      }
      slice(integral_constant<int, 6>{});
    }
    if constexpr (NEXT_TASK) {
      wr[0] = nwr[0];
      wr[1] = nwr[1];
      wr[2] = nwr[2];
      dsc = ndsc + ndsc;
      dbi = ndbi + ndbi;
    }
  };

  if constexpr (STAGED) {
    // the stage zeroed once: the fifth dword of every row and the slot of the row outside the image stay zero
    const v4i z4 = {0, 0, 0, 0};
#pragma unroll
    for (int i = 0; i < 4; ++i)
      if (64 * i + lane < 16 * FW_CP / 16) *reinterpret_cast<v4i*>(fw_lds + stage0 + (64 * i + lane) * 16) = z4;
    const bool first = xoff == 0xffffffffu;  // the tensor's first row: fetched from its first byte, shifted up one
    load_rows(first ? 0u : xoff);
    float s, bb;
    fetch_params(ch0, wr, s, bb);
    dsc = s + s;
    dbi = bb + bb;
    if (first) {  // (both pieces: the lane's second one shares the offset register)
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        const uint32_t d0 = (uint32_t)nx[i][0], d1 = (uint32_t)nx[i][1], d2 = (uint32_t)nx[i][2], d3 = (uint32_t)nx[i][3];
        nx[i][0] = (int)(d0 << 8);
        nx[i][1] = (int)__builtin_amdgcn_alignbyte(d1, d0, 3);
        nx[i][2] = (int)__builtin_amdgcn_alignbyte(d2, d1, 3);
        nx[i][3] = (int)__builtin_amdgcn_alignbyte(d3, d2, 3);
      }
    }
  } else {
    fetch_task(ch0, xoff);
  }
  fetch_w(0, 0);
  fetch_w(1, 1);  // (KS >= 4: whole rounds)
  fetch_w(2, 2);
  fetch_w(3, 3);
  PLHIP_STAMP(2);
  if constexpr (STAGED) stage_rows();
  // the rounds: 0 produces only, 1 is the first to multiply, R - 1 the last to produce
  using T = std::true_type;
  using F = std::false_type;
  auto behind = [&](int r) __attribute__((always_inline)) {  // round r is done: the stamps of the timeline, the barrier
    // The rounds of a path are one basic block.  An MFMA has no side effect, and nothing but the epilogue reads an accumulator:
    // without this empty statement the compiler moved whole accumulation chains behind the last round and kept every operand of
    // theirs in scratch until then.  It costs no instruction: the accumulators of round r exist here, in their registers.
    if (r >= 1) {
#pragma unroll
      for (int n = 0; n < FW_NT; ++n)
#pragma unroll
        for (int m = 0; m < MTW; ++m) asm volatile("" : "+v"(acc[n][m]));
    }
    xoff += 128 * 196;
    if (r == 0) PLHIP_STAMP(3);
    else if (r < 5) PLHIP_STAMP(4 + 2 * (r - 1));
    __syncthreads();
    if (r >= 1 && r < 5) PLHIP_STAMP(5 + 2 * (r - 1));
  };
  round(T{}, F{}, F{}, std::bool_constant<R == 1>{}, 0, 0);
  behind(0);
  if constexpr (R >= 2) {
    round(T{}, T{}, T{}, std::bool_constant<R == 2>{}, 1, 0);
    behind(1);
  }
  if constexpr (R >= 3) {
    round(T{}, T{}, F{}, std::bool_constant<R == 3>{}, 2, 1);
    behind(2);
  }
  if constexpr (R >= 4) {
    static_assert(R <= 4, "C <= 512: dwpw_launch_plan");
    round(T{}, T{}, F{}, T{}, 3, 2);
    behind(3);
  }
  float psc[MTW], pbi[MTW];  // pointwise scale / bias of this lane's channels: fetched under the last round's MFMAs
#pragma unroll
  for (int m = 0; m < MTW; ++m) {
    psc[m] = 1.f;
    pbi[m] = 0.f;
    if (OUT != OUT_I32) {
      psc[m] = g.scale[(mt0 + m) * 32 + c];
      if (g.bias) pbi[m] = g.bias[(mt0 + m) * 32 + c];
    }
  }
  // ------------------------------------------------------------------ last K-steps + epilogue
  // accumulator register r of n tile n: pixel 32 n + 8 (r >> 2) + 4 h + (r & 3) = output row 2 n + (r >> 3), column
  // 8 ((r >> 2) & 1) + 4 h + (r & 3) of the 16-wide chunk; lane (c, h) owns output channel 32 (mt0 + m) + c.
  const int orow0 = FW_TR * hf;
  if (OUT == OUT_I8) {
    // int8: the last round's 4 K-steps n-tile-major, so that tile n - 1 is requantised (fma / min / cvt: they overlap with the
    // matrix pipe) in the shadow of tile n's MFMAs; only the last tile's epilogue is exposed
    // (requant_hi2 / requant_leak, plhip_device.h, written out: through the functions this unit's ISA moves)
    const float hi2 = g.act == ACT_RELU6 ? fminf(g.alpha + g.alpha, 254.f) : 254.f;
    const float leak = g.act == ACT_LEAKY ? g.alpha : 1.f;
    uint8_t* stg = fw_lds + (size_t)KS * FW_KSTEP + wave * (32 * MTW * FW_SP);
    const uint32_t rbf = (uint32_t)(R - 1) * (4 * FW_KSTEP);
    v2i flo[2][4], fhi[2][4];  // fragments of the 4 K-steps of one n tile, two sets
    auto read_tile = [&](auto n_c) __attribute__((always_inline)) {
      constexpr int n = decltype(n_c)::value;
      const uint32_t ta = (tr00 + rbf) ^ (uint32_t)(n << 5);
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        flo[n & 1][j] = __builtin_amdgcn_ds_read_tr8_b64_v2i32((lds_v2i_ptr_t)(fw_lds + ta + j * FW_KSTEP));
        fhi[n & 1][j] = __builtin_amdgcn_ds_read_tr8_b64_v2i32((lds_v2i_ptr_t)(fw_lds + ta + j * FW_KSTEP + 1024));
      }
    };
    auto mfma_tile = [&](auto n_c, auto first_c) __attribute__((always_inline)) {  // first_c: these are K-steps 0 .. 3 (R = 1)
      constexpr int n = decltype(n_c)::value;
      constexpr bool FIRST = decltype(first_c)::value;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const v4i av = {flo[n & 1][j][0], flo[n & 1][j][1], fhi[n & 1][j][0], fhi[n & 1][j][1]};
#pragma unroll
        for (int m = 0; m < MTW; ++m) acc[n][m] = __builtin_amdgcn_mfma_i32_32x32x32_i8(av, W[j][m], FIRST && j == 0 ? zero16 : acc[n][m], 0, 0, 0);
      }
    };
    auto epi_tile = [&](auto n_c) __attribute__((always_inline)) {
      constexpr int n = decltype(n_c)::value;
#pragma unroll
      for (int m = 0; m < MTW; ++m) {
        const float s2 = psc[m] + psc[m], b2 = pbi[m] + pbi[m];
        uint32_t edw[4] = {0, 0, 0, 0};  // (tr_requant_chunk, gemm_tr_common.h, written out: the last tile skips its two dead groups)
#pragma unroll
        for (int gq = 0; gq < 4; ++gq) {
          if (n == FW_NT - 1 && gq >= 2) continue;  // row 7 of the tile does not exist
          int v[4] = {acc[n][m][4 * gq], acc[n][m][4 * gq + 1], acc[n][m][4 * gq + 2], acc[n][m][4 * gq + 3]};
          edw[gq] = PWNN ? requant4_nn_rtz(v, s2, b2, hi2, a.ones) : requant4<ACT_LEAKY>(v, s2, b2, leak, -254.f, 254.f);
        }
        // half exchange: every lane gets the 16 pixels of ONE output row of its channel (h = 0: row 2 n, h = 1: row 2 n + 1)
        auto s02 = __builtin_amdgcn_permlane32_swap(edw[0], edw[2], false, false);
        auto s13 = __builtin_amdgcn_permlane32_swap(edw[1], edw[3], false, false);
        const uint32_t d0 = s02[0], d1 = s02[1], d2 = s13[0], d3 = s13[1];
        if (n < FW_NT - 1 || h == 0) {
          // 14 bytes at a 2-byte aligned position: halfword writes
          uint16_t* p = reinterpret_cast<uint16_t*>(stg + (32 * m + c) * FW_SP + (2 * n + h) * 14);
          p[0] = (uint16_t)d0; p[1] = (uint16_t)(d0 >> 16);
          p[2] = (uint16_t)d1; p[3] = (uint16_t)(d1 >> 16);
          p[4] = (uint16_t)d2; p[5] = (uint16_t)(d2 >> 16);
          p[6] = (uint16_t)d3;
        }
      }
    };
    using I0 = integral_constant<int, 0>;
    using I1 = integral_constant<int, 1>;
    using I2 = integral_constant<int, 2>;
    using I3 = integral_constant<int, 3>;
    auto last_k_steps = [&](auto first_c) __attribute__((always_inline)) {
      read_tile(I0{});
      read_tile(I1{});
      mfma_tile(I0{}, first_c);
      __builtin_amdgcn_sched_barrier(0);
      read_tile(I2{});
      mfma_tile(I1{}, first_c);
      epi_tile(I0{});
      __builtin_amdgcn_sched_barrier(0);
      read_tile(I3{});
      mfma_tile(I2{}, first_c);
      epi_tile(I1{});
      __builtin_amdgcn_sched_barrier(0);
      mfma_tile(I3{}, first_c);
      epi_tile(I2{});
      __builtin_amdgcn_sched_barrier(0);
    };
    last_k_steps(std::bool_constant<R == 1>{});  // R = 1: the first consuming round is the last one
    PLHIP_STAMP(12);
    epi_tile(I3{});
    PLHIP_STAMP(13);
    // copy-out: lane -> (row lane >> 3 of a group of 8, 16-byte piece lane & 7); a channel row is 98 contiguous bytes
    const int piece = lane & 7, rsub = lane >> 3;
    int8_t* ybase = reinterpret_cast<int8_t*>(g.y) + ((size_t)b * g.M + mt0 * 32) * 196 + 98 * hf + piece * 16;
#pragma unroll
    for (int i = 0; i < 4 * MTW; ++i) {
      const int row = 8 * i + rsub;
      const v4i v = *reinterpret_cast<const v4i*>(stg + row * FW_SP + (piece < 7 ? piece : 6) * 16);
      int8_t* yp = ybase + (size_t)row * 196;
      if (piece < 6) __builtin_memcpy(yp, &v, 16);  // possibly unaligned: fine for global memory
      else if (piece == 6) {
        const uint16_t t2 = (uint16_t)v[0];
        __builtin_memcpy(yp, &t2, 2);
      }
    }
  } else {
    round(F{}, T{}, std::bool_constant<R == 1>{}, T{}, R, R - 1);  // R = 1: the first consuming round is the last one
    PLHIP_STAMP(12);
    // the lane's k half again from the thread index, which is in a register anyway (through an empty statement, or the compiler
    // recognises `h`): `h` kept from the top of the kernel to here was the one register too many of the M = 512 forms
    uint32_t tid = threadIdx.x;
    asm volatile("" : "+v"(tid));
    const int h = (int)(tid >> 5) & 1;
    const float fcap = f32_cap(g.act, g.alpha);
    const float flo = f32_lo(g.act);
#pragma unroll
    for (int m = 0; m < MTW; ++m) {
      const size_t chan = ((size_t)b * g.M + (mt0 + m) * 32 + c) * 196;
#pragma unroll
      for (int n = 0; n < FW_NT; ++n) {
#pragma unroll
        for (int gq = 0; gq < 4; ++gq) {
          const int o = 2 * n + (gq >> 1);
          if (o >= FW_TR) continue;
          const int col = 8 * (gq & 1) + 4 * h;
          const size_t off = chan + (size_t)(orow0 + o) * 14 + col;
          if (OUT == OUT_F32) {
            float f[4];
#pragma unroll
            for (int e = 0; e < 4; ++e) f[e] = f32_clamped(acc[n][m][4 * gq + e], psc[m], pbi[m], g.act, g.alpha, flo, fcap);
            float* yp = reinterpret_cast<float*>(g.y) + off;
            if (col + 3 < 14) {
              const v4f v = {f[0], f[1], f[2], f[3]};
              __builtin_memcpy(yp, &v, 16);
            } else if (col < 14) {
              yp[0] = f[0];
              yp[1] = f[1];
            }
          } else {
            int* yp = reinterpret_cast<int*>(g.y) + off;
            if (col + 3 < 14) {
              const v4i v = {acc[n][m][4 * gq], acc[n][m][4 * gq + 1], acc[n][m][4 * gq + 2], acc[n][m][4 * gq + 3]};
              __builtin_memcpy(yp, &v, 16);
            } else if (col < 14) {
              yp[0] = acc[n][m][4 * gq];
              yp[1] = acc[n][m][4 * gq + 1];
            }
          }
        }
      }
    }
  }
  PLHIP_STAMP(14);
  if (diag) {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    PLHIP_STAMP(15);
  }
}

template <int MTW, int OUT, bool DWNN, bool PWNN>
__global__ __launch_bounds__(512, 2) void fused_dwpw14_kernel(FusedArgs a) {
  switch (a.pw.KS >> 2) {  // block-uniform (128 | C <= 512: dwpw_launch_plan)
    case 1: return fused_dwpw14_body<MTW, OUT, DWNN, PWNN, 1>(a);
    case 2: return fused_dwpw14_body<MTW, OUT, DWNN, PWNN, 2>(a);
    case 3: return fused_dwpw14_body<MTW, OUT, DWNN, PWNN, 3>(a);
    default: return fused_dwpw14_body<MTW, OUT, DWNN, PWNN, 4>(a);
  }
}

// executes a plan of dwpw_launch_plan (dw_plan.h): the 14 x 14 kernel of this file, or the streaming / 7 x 7 kernel
void launch_fused_dwpw(const FusedArgs& a_in, const DwPlan& p, int out, hipStream_t s) {
  FusedArgs a = a_in;
  a.tiles = p.tiles;
  a.pw.NT = p.NT;
  a.ones = 0x01010101u;
  if (p.family == DWPW_7) return run_fused_small(p, a, out, s);
  if (p.family == DWPW_STREAM) return run_fused_stream(p, a, out, s);
  PLHIP_SET_STAMPS(a.pw, "fw", sizeof(unsigned long long) * 1024 * 8 * FW_STAMP_SLOTS);
  with_const<1, 2>(p.MTW, [&](auto mtw) {
    with_out_nonneg<OUT_I32, OUT_F32, OUT_I8>(out, a.dw_act, a.pw.act, [&](auto out_c, auto dn, auto pn) {
      constexpr int OUT = decltype(out_c)::value;
      constexpr bool DN = decltype(dn)::value != 0, PN = decltype(pn)::value != 0;
      // (PWNN exists for int8 output only)
      if constexpr (OUT == OUT_I8 || !PN) launch_max_lds(fused_dwpw14_kernel<decltype(mtw)::value, OUT, DN, PN>, p, s, a);
    });
  });
}

}  // namespace plhip
