// conv_stem_common.h — what the MFMA stem kernels share: conv_direct_i8.hip (3x3 stride 2, int8 input), conv_stem_f32in.hip and
// conv_stem_u8in.hip (the same conv behind a fused quantiser) and conv_stem7_i8.hip (7x7 stride 2).  All four run one block per
// (image, 4 output rows, 32 column quads = 128 output pixels), a wave per output row, a lane per quad and k half, and end in
// gemm_epilogue.  The three 3x3 kernels differ only in how a lane gets its five row windows; everything behind the windows is
// here ONCE, because the packed A fragments (pack_conv3x3s2_mfma_kernel) are a contract with this k order.
#pragma once
#include <type_traits>

#include "gemm_epilogue.h"
#include "gemm_tr_common.h"  // v2i
#include "plhip_kernels.h"

namespace plhip {

// LDS row pitch of the staged int8 tile of the f32in / u8in kernels ([Cin * 9 rows][STEM_LDS_PITCH]): 4 bytes in front of the
// tile's first column, 256 columns, 12 behind
constexpr int STEM_LDS_PITCH = 272;

// ---- host: grid and instantiation ------------------------------------------------------------------------------------
// 1-D grid, a multiple of 8 blocks (stem_block below); the callers' envelopes keep the count below 2^31 - 8
inline dim3 stem_grid(const DirectS2Args& a) {
  const long nblk = (long)(((a.ow >> 2) + 31) / 32) * ((a.oh + 3) / 4) * a.n;
  return dim3((unsigned)((nblk + 7) / 8 * 8));
}

// calls launch(integral_constant<int, OUT>, integral_constant<bool, MFULL>) for the output kind and cout % 32 == 0
template <class F>
inline void stem_dispatch(const DirectS2Args& a, int out, F&& launch) {
  using std::integral_constant;
  const bool mfull = a.cout % 32 == 0;
#define PLHIP_STEM(O)                                                                \
  do {                                                                               \
    if (mfull) launch(integral_constant<int, O>{}, integral_constant<bool, true>{}); \
    else launch(integral_constant<int, O>{}, integral_constant<bool, false>{});      \
  } while (0)
  if (out == OUT_I32) PLHIP_STEM(OUT_I32);
  else if (out == OUT_F32) PLHIP_STEM(OUT_F32);
  else PLHIP_STEM(OUT_I8);
#undef PLHIP_STEM
}

// ---- device ----------------------------------------------------------------------------------------------------------
// block = (quad tile of a row, group of 4 output rows, image), decoded from a 1-D grid of 8 * per blocks: XCD x (= blockIdx % 8,
// round-robin dispatch) gets the x-th eighth of the (image, row group, column tile) space, so that row groups sharing an input
// row sit on one L2.  All of it is block-uniform; false = a block of the grid's round-up, nothing to do.
// (decoded before the range test, without an early return: with one, conv3x3s2_mfma_kernel<OUT_I8, true> was allocated 134 VGPRs
// instead of 128, one wave per SIMD less; nx, ny >= 1, so the divisions are safe for the round-up blocks too)
__device__ __forceinline__ bool stem_block(const DirectS2Args& a, int& bx, int& by, int& b) {
  const int nx = ((a.ow >> 2) + 31) >> 5, ny = (a.oh + 3) >> 2;
  const unsigned nb = (unsigned)(nx * ny * a.n), per = (nb + 7) >> 3;
  const unsigned vb = (blockIdx.x & 7) * per + (blockIdx.x >> 3);
  bx = (int)(vb % (unsigned)nx);
  const unsigned t = vb / (unsigned)nx;
  by = (int)(t % (unsigned)ny);
  b = (int)(t / (unsigned)ny);
  return vb < nb;
}

// the epilogue's view of a stem launch; TAIL: the fused graph tail of the fp32 output (the 7x7 stem only)
template <bool TAIL>
__device__ __forceinline__ void stem_gemm_args(const DirectS2Args& a, GemmArgs& g) {
  g.y = a.y;
  g.scale = a.scale;
  g.bias = a.bias;
  g.M = a.cout;
  g.HWY = a.oh * a.ow;
  g.y_bstride = (size_t)a.cout * a.oh * a.ow;
  g.act = a.act;
  g.alpha = a.alpha;
  g.res = TAIL ? a.res : nullptr;
  g.res_relu = TAIL ? a.res_relu : 0;
  g.y2 = TAIL ? a.y2 : nullptr;
  g.inv_scale2 = TAIL ? a.inv_scale2 : 0.f;
}

// 3x3 stems, first thing in the kernel: g, the first m tile's scales / biases and its A fragment (returned) are requested before
// the caller fetches its windows, so that they arrive under that fetch
template <int OUT>
__device__ __forceinline__ v4i stem3x3_begin(const DirectS2Args& a, const int8_t* __restrict__ afrag, int lane, float* lsb,
                                             GemmArgs& g) {
  stem_gemm_args<false>(a, g);
  const v4i af0 = *reinterpret_cast<const v4i*>(afrag + (size_t)lane * 16);
  if (OUT != OUT_I32) stage_scale_bias<1, OUT>(g, 0, lane, lsb);
  return af0;
}

// the row windows of lane (c, h) of wave `wave` from the staged tile: window cr = 5 h + L -> (channel cr / 3, filter row cr % 3)
// = staged row 9 ci + 2 wave + r3; the lane reads it as 16 aligned LDS bytes and cuts the four 3-byte windows of its quad with
// v_alignbyte (the window of quad c starts at LDS byte 8 c + 3 for the left padding 1)
__device__ __forceinline__ void stem3x3_lds_windows(const uint8_t* img, int cin, int lane, int wave, uint32_t (&win)[4][5]) {
  const int c = lane & 31, h = lane >> 5;
#pragma unroll
  for (int L = 0; L < 5; ++L) {
    const int cr = 5 * h + L;
    const int ci = cr / 3, r3 = cr - ci * 3;
    const bool live = cr < 3 * cin;  // (3 Cin windows exist)
    const int lrow = live ? ci * 9 + 2 * wave + r3 : 0;
    const uint8_t* p = img + lrow * STEM_LDS_PITCH + 8 * c;
    const v2i lo = *reinterpret_cast<const v2i*>(p), hi = *reinterpret_cast<const v2i*>(p + 8);
    const uint32_t m = live ? 0xffffffffu : 0u;
    const uint32_t d0 = (uint32_t)lo[0] & m, d1 = (uint32_t)lo[1] & m, d2 = (uint32_t)hi[0] & m, d3 = (uint32_t)hi[1] & m;
    win[0][L] = __builtin_amdgcn_alignbyte(d1, d0, 3);  // columns 8 xq - 1 ..
    win[1][L] = __builtin_amdgcn_alignbyte(d2, d1, 1);  // 8 xq + 1 ..
    win[2][L] = __builtin_amdgcn_alignbyte(d2, d1, 3);  // 8 xq + 3 ..
    win[3][L] = __builtin_amdgcn_alignbyte(d3, d2, 1);  // 8 xq + 5 ..
  }
}

// 3x3 stems, from the windows on: win[j][L] = the 3 taps of output j of the quad in the lane's row window L (zero where the
// window does not exist or lies in the padding).  The B operand of output j is
//     (L0.0 L0.1 L0.2 L1.0 | L1.1 L1.2 L2.0 L2.1 | L2.2 L3.0 L3.1 L3.2 | L4.0 L4.1 L4.2 0),
// the 27 taps are ONE K-step of the 32x32x32 MFMA per output and m tile.
// hw = the quad's first output inside its image; qvalid = false: a clamped duplicate, computed and not stored.
// (g by value on purpose: the copy dissolves when the helper is inlined, and taken by reference one instantiation of
// conv3x3s2_mfma_kernel was allocated 98 VGPRs instead of 94, one wave per SIMD less)
template <int OUT, bool MFULL>
__device__ __forceinline__ void stem3x3_mfma(const GemmArgs g, const int8_t* __restrict__ afrag, v4i af0, const uint32_t (&win)[4][5],
                                             float* lsb, int lane, int b, int hw, bool qvalid) {
  const int h = lane >> 5;
  v4i bf[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    bf[j][0] = (int)__builtin_amdgcn_perm(win[j][1], win[j][0], 0x04020100u);
    bf[j][1] = (int)__builtin_amdgcn_perm(win[j][2], win[j][1], 0x05040201u);
    bf[j][2] = (int)__builtin_amdgcn_perm(win[j][3], win[j][2], 0x06050402u);
    bf[j][3] = (int)(win[j][4] & 0x00ffffffu);
  }
  const int MT = (g.M + 31) >> 5;
  for (int mt = 0; mt < MT; ++mt) {  // uniform
    v4i af = af0;
    if (mt > 0) {
      af = *reinterpret_cast<const v4i*>(afrag + ((size_t)mt * 64 + lane) * 16);
      if (OUT != OUT_I32) stage_scale_bias<1, OUT>(g, mt, lane, lsb);
    }
    v16i acc[1][4];
    const v16i zero16 = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};  // (an inline operand of the MFMA: no accumulator zeroing)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[0][j] = __builtin_amdgcn_mfma_i32_32x32x32_i8(af, bf[j], zero16, 0, 0, 0);
    if (qvalid) gemm_epilogue_act<1, OUT, true, MFULL>(g, acc, mt, h, b, hw, lsb, g.HWY - hw);
  }
}

// f32in / u8in, behind the staging loop (the block's barrier is here: the first A fragment and the scales / biases are requested
// in front of it).  A wave owns output row 4 by + wave, lane (c, h) quad 32 bx + c of it.
template <int OUT, bool MFULL>
__device__ __forceinline__ void stem3x3_staged(const DirectS2Args& a, const int8_t* __restrict__ afrag, const uint8_t* img, float* lsb,
                                               int lane, int wave, int bx, int by, int b) {
  const int owq = a.ow >> 2;
  const int oy = by * 4 + wave;
  int xq = bx * 32 + (lane & 31);
  const bool qvalid = xq < owq && oy < a.oh;
  if (xq >= owq) xq = owq - 1;

  GemmArgs g;
  const v4i af0 = stem3x3_begin<OUT>(a, afrag, lane, lsb, g);
  __syncthreads();

  uint32_t win[4][5];
  stem3x3_lds_windows(img, a.cin, lane, wave, win);
  stem3x3_mfma<OUT, MFULL>(g, afrag, af0, win, lsb, lane, b, oy * a.ow + 4 * xq, qvalid);
}

}  // namespace plhip
