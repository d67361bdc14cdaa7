// conv_stem_f32in.hip — calib[fp32_to_int8] + conv 3x3 stride 2 (Cin <= 3) in ONE launch: the first two instructions of the
// MobileNet programs (the fp32 image is quantised with the conv's input scale, then convolved).  As two kernels the int8 image is
// written and read back (19 + 19 MB of the 147 MB the pair moves at batch 128) and the calib launch is a pure stream at the HBM
// roof (16 us) in front of a stem that cannot start before it ends.
// Replaces the instruction pair CalibComputeFp32ToInt8 (lite/kernels/arm/calib_compute.cc:25-40 -> type_trans.cc:34-187) ;
// DirectConv<kInt8,*> (lite/kernels/arm/conv_direct.cc -> conv3x3s2_direct_int8.cc); results bit-identical to the two kernels:
// every input value is quantised exactly as calib_f32_to_i8_kernel does (round_sat_i8(inv_scale * x)), the conv is the MFMA
// form of conv_direct_i8.hip (same A fragments, same MFMA half and epilogue: conv_stem_common.h).
//
// block = (image, 4 output rows, 32 column quads = 128 output pixels): the 9 input rows x Cin channels x 264 columns it reads are
// fetched ONCE as aligned 16-byte pieces of fp32, quantised and written to LDS ([Cin * 9 rows][272 B], zeros where the padding
// is: no masks later); a wave then owns one output row and reads its row windows from there (stem3x3_staged, conv_stem_common.h).
#include "conv_stem_common.h"

namespace plhip {

bool conv3x3s2_f32in_supported(const DirectS2Args& a) {
  return a.cin >= 1 && a.cin <= 3 && (a.ow & 3) == 0 && (a.w & 3) == 0 && a.pl == 1 && (a.pt == 0 || a.pt == 1) && a.cout <= 128 &&
         (long)a.n * a.cin * a.h * a.w < (1L << 31) && (long)(((a.ow >> 2) + 31) / 32) * ((a.oh + 3) / 4) * a.n < (1L << 31) - 8;
}

template <int OUT, bool MFULL>
__global__ __launch_bounds__(256) void conv3x3s2_mfma_f32in_kernel(DirectS2Args a, const int8_t* __restrict__ afrag) {
  PLHIP_PRELOAD(a.xf); PLHIP_PRELOAD(a.y); PLHIP_PRELOAD(a.scale); PLHIP_PRELOAD(a.bias); PLHIP_PRELOAD(afrag);
  PLHIP_PRELOAD(a.n); PLHIP_PRELOAD(a.cin); PLHIP_PRELOAD(a.h); PLHIP_PRELOAD(a.w); PLHIP_PRELOAD(a.cout); PLHIP_PRELOAD(a.oh);
  PLHIP_PRELOAD(a.ow); PLHIP_PRELOAD(a.pt); PLHIP_PRELOAD(a.act); PLHIP_PRELOAD(a.alpha); PLHIP_PRELOAD(a.x_inv_scale);
  __shared__ __attribute__((aligned(16))) float lsb_all[4][64];
  __shared__ __attribute__((aligned(16))) uint8_t img[27 * STEM_LDS_PITCH];
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  float* lsb = lsb_all[wave];
  int bx, by, b;
  if (!stem_block(a, bx, by, b)) return;  // block-uniform

  // ---- stage: input rows 8 by - pt + j (j = 0..8) of every channel, columns 256 bx - 4 .. 256 bx + 259, as int8
  const int c0 = 256 * bx - 4, ih0 = 8 * by - a.pt;
  const int nrows = a.cin * 9;
  const float inv = a.x_inv_scale;
  const size_t img_base = (size_t)b * a.cin * a.h * a.w;
  // (all of a thread's pieces are requested before the first one is converted: fetched and converted one by one the block paid
  // one memory round trip per piece, 7 in a row: 33.8 us for the launch)
  constexpr int NPIECE = (27 * 66 + 255) / 256;
  v4f pv[NPIECE];
  int pdst[NPIECE];
#pragma unroll
  for (int it = 0; it < NPIECE; ++it) {
    const int k = it * 256 + (int)threadIdx.x;
    const int row = k / 66, piece = k - row * 66;
    const int ci = row / 9, j = row - ci * 9;
    const int ih = ih0 + j, col = c0 + 4 * piece;
    pdst[it] = k < nrows * 66 ? row * STEM_LDS_PITCH + 4 * piece : -1;
    pv[it] = v4f{0.f, 0.f, 0.f, 0.f};
    if (k < nrows * 66 && ih >= 0 && ih < a.h && col >= 0 && col < a.w)  // (w % 4 == 0: a piece is inside or outside as a whole)
      pv[it] = *reinterpret_cast<const v4f*>(a.xf + img_base + ((size_t)ci * a.h + ih) * a.w + col);
  }
#pragma unroll
  for (int it = 0; it < NPIECE; ++it) {
    const v4f v = pv[it];
    const uint32_t pk = calib4_i8(v, inv);
    if (pdst[it] >= 0) *reinterpret_cast<uint32_t*>(img + pdst[it]) = pk;  // (a piece outside the image: +0.0 -> 0, the padding)
  }
  // (bytes 264 .. 271 of a row are read by the last quads' 16-byte windows and never used: no need to clear them)

  stem3x3_staged<OUT, MFULL>(a, afrag, img, lsb, lane, wave, bx, by, b);
}

// a.xf = the fp32 image, a.x_inv_scale = 1 / calib scale; a.wp = the packed block of launch_pack_conv3x3s2_direct
void launch_conv3x3s2_f32in(const DirectS2Args& a, const int8_t* afrag, int out, hipStream_t s) {
  stem_dispatch(a, out, [&](auto O, auto MF) {
    hipLaunchKernelGGL((conv3x3s2_mfma_f32in_kernel<decltype(O)::value, decltype(MF)::value>), stem_grid(a), dim3(256), 0, s, a, afrag);
  });
}

}  // namespace plhip
