// conv_stem_u8in.hip — image_to_tensor + calib[fp32_to_int8] + conv 3x3 stride 2 (Cin 1 or 3) in ONE launch: fusion F
// (conv_stem_f32in.hip) with the caller's uint8 interleaved image [n, h, w, cs] as its source instead of the normalised fp32 NCHW
// tensor.  Replaces ImagePreprocess::image_to_tensor (lite/utils/cv/paddle_image_preprocess.cc:143-172 -> image2tensor.cc) on the
// host followed by the instruction pair CalibComputeFp32ToInt8 ; DirectConv<kInt8,*> at the head of the MobileNet programs.
// Bit-identical to the three steps: every staged value is round_sat_i8(inv * ((float(byte) - means[c]) * scales[c])) — the two
// roundings of image2tensor.cc:549-563, then the quantiser of calib_f32_to_i8_kernel — and everything behind the staging loop is
// the code conv_stem_f32in.hip runs (stem3x3_staged, conv_stem_common.h).
//
// block = (image, 4 output rows, 128 output pixels) as there: the block's 9 input rows x 264 columns are fetched ONCE, a lane taking
// 4 pixels of one row (cs aligned dwords: 12 bytes of BGR, a 224-wide row is 56 such pieces), de-interleaved, normalised and
// quantised per channel into the same [Cin * 9 rows][STEM_LDS_PITCH] int8 LDS layout, with zeros where the padding is (the conv pads the
// int8 tensor, not the image).  Needs w % 4 == 0 (a piece is inside or outside the image as a whole, and every row starts on a
// dword: w * cs % 4 == 0), which the f32in envelope asks already.
#include "conv_stem_common.h"

namespace plhip {

bool conv3x3s2_u8in_supported(const DirectS2Args& a, const ImageArgs& im) {
  return conv3x3s2_f32in_supported(a) && (im.cs == 1 || im.cs == 3 || im.cs == 4) && im.c == (im.cs == 1 ? 1 : 3) && a.cin == im.c &&
         im.n == a.n && im.h == a.h && im.w == a.w && (long)a.n * a.h * a.w * im.cs < (1L << 31);
}

template <int OUT, bool MFULL, int CS>
__global__ __launch_bounds__(256) void conv3x3s2_mfma_u8in_kernel(DirectS2Args a, ImageArgs im, const int8_t* __restrict__ afrag) {
  PLHIP_PRELOAD(im.src); PLHIP_PRELOAD(a.y); PLHIP_PRELOAD(a.scale); PLHIP_PRELOAD(a.bias); PLHIP_PRELOAD(afrag);
  PLHIP_PRELOAD(a.n); PLHIP_PRELOAD(a.cin); PLHIP_PRELOAD(a.h); PLHIP_PRELOAD(a.w); PLHIP_PRELOAD(a.cout); PLHIP_PRELOAD(a.oh);
  PLHIP_PRELOAD(a.ow); PLHIP_PRELOAD(a.pt); PLHIP_PRELOAD(a.act); PLHIP_PRELOAD(a.alpha); PLHIP_PRELOAD(a.x_inv_scale);
  constexpr int C = CS == 1 ? 1 : 3;
  __shared__ __attribute__((aligned(16))) float lsb_all[4][64];
  __shared__ __attribute__((aligned(16))) uint8_t img[27 * STEM_LDS_PITCH];
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  float* lsb = lsb_all[wave];
  int bx, by, b;
  if (!stem_block(a, bx, by, b)) return;  // block-uniform

  // ---- stage: input rows 8 by - pt + j (j = 0..8), columns 256 bx - 4 .. 256 bx + 259, every channel, as int8
  const int c0 = 256 * bx - 4, ih0 = 8 * by - a.pt;
  const float inv = a.x_inv_scale;
  // (all of a thread's pieces are requested before the first one is converted, as in the f32in kernel)
  constexpr int NPIECE = (9 * 66 + 255) / 256;
  uint32_t pw[NPIECE][CS];
  int pdst[NPIECE];
  bool pin[NPIECE];
#pragma unroll
  for (int it = 0; it < NPIECE; ++it) {
    const int k = it * 256 + (int)threadIdx.x;
    const int j = k / 66, piece = k - j * 66;
    const int ih = ih0 + j, col = c0 + 4 * piece;
    pdst[it] = k < 9 * 66 ? j * STEM_LDS_PITCH + 4 * piece : -1;
    pin[it] = k < 9 * 66 && ih >= 0 && ih < a.h && col >= 0 && col < a.w;  // (w % 4 == 0: a piece is inside or outside as a whole)
#pragma unroll
    for (int d = 0; d < CS; ++d) pw[it][d] = 0u;
    if (pin[it]) {
      const uint32_t* p = reinterpret_cast<const uint32_t*>(im.src + (((size_t)b * a.h + ih) * a.w + col) * CS);
#pragma unroll
      for (int d = 0; d < CS; ++d) pw[it][d] = p[d];
    }
  }
#pragma unroll
  for (int it = 0; it < NPIECE; ++it) {
#pragma unroll
    for (int ci = 0; ci < C; ++ci) {
      int q[4];
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int bi = e * CS + ci;  // byte ci of pixel e of the piece
        const float u = (float)((pw[it][bi >> 2] >> (8 * (bi & 3))) & 0xffu);
        q[e] = round_sat_i8(inv * ((u - im.mean[ci]) * im.scale[ci]));
      }
      const uint32_t pk = pin[it] ? pack4_i8(q[0], q[1], q[2], q[3]) : 0u;  // (a piece outside the image: the int8 padding, 0)
      if (pdst[it] >= 0) *reinterpret_cast<uint32_t*>(img + ci * 9 * STEM_LDS_PITCH + pdst[it]) = pk;
    }
  }
  // (bytes 264 .. 271 of a row are read by the last quads' 16-byte windows and never used: no need to clear them)

  stem3x3_staged<OUT, MFULL>(a, afrag, img, lsb, lane, wave, bx, by, b);
}

// a.x_inv_scale = 1 / calib scale; afrag = the MFMA A fragments of launch_pack_conv3x3s2_direct's block; im: the image (cs bytes a pixel)
template <int CS>
static void launch_u8in_cs(const DirectS2Args& a, const ImageArgs& im, const int8_t* afrag, int out, hipStream_t s) {
  stem_dispatch(a, out, [&](auto O, auto MF) {
    hipLaunchKernelGGL((conv3x3s2_mfma_u8in_kernel<decltype(O)::value, decltype(MF)::value, CS>), stem_grid(a), dim3(256), 0, s, a, im, afrag);
  });
}

void launch_conv3x3s2_u8in(const DirectS2Args& a, const ImageArgs& im, const int8_t* afrag, int out, hipStream_t s) {
  if (im.cs == 1) launch_u8in_cs<1>(a, im, afrag, out, s);
  else if (im.cs == 3) launch_u8in_cs<3>(a, im, afrag, out, s);
  else launch_u8in_cs<4>(a, im, afrag, out, s);
}

}  // namespace plhip
