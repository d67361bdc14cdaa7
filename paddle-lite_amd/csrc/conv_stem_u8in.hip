// conv_stem_u8in.hip — image_to_tensor + calib[fp32_to_int8] + conv 3x3 stride 2 (Cin 1 or 3) in ONE launch: fusion F
// (conv_stem_f32in.hip) with the caller's uint8 interleaved image [n, h, w, cs] as its source instead of the normalised fp32 NCHW
// tensor.  Replaces ImagePreprocess::image_to_tensor (lite/utils/cv/paddle_image_preprocess.cc:143-172 -> image2tensor.cc) on the
// host followed by the instruction pair CalibComputeFp32ToInt8 ; DirectConv<kInt8,*> at the head of the MobileNet programs.
// Bit-identical to the three steps: every staged value is round_sat_i8(inv * ((float(byte) - means[c]) * scales[c])) — the two
// roundings of image2tensor.cc:549-563, then the quantiser of calib_f32_to_i8_kernel — and the MFMA half and the epilogue below are
// conv_stem_f32in.hip's, line for line.
//
// block = (image, 4 output rows, 128 output pixels) as there: the block's 9 input rows x 264 columns are fetched ONCE, a lane taking
// 4 pixels of one row (cs aligned dwords: 12 bytes of BGR, a 224-wide row is 56 such pieces), de-interleaved, normalised and
// quantised per channel into the same [Cin * 9 rows][SF_PITCH] int8 LDS layout, with zeros where the padding is (the conv pads the
// int8 tensor, not the image).  Needs w % 4 == 0 (a piece is inside or outside the image as a whole, and every row starts on a
// dword: w * cs % 4 == 0), which the f32in envelope asks already.
#include "gemm_epilogue.h"
#include "plhip_kernels.h"
#include "gemm_tr_common.h"

namespace plhip {

constexpr int SU_PITCH = 272;  // as SF_PITCH of conv_stem_f32in.hip: 4 bytes in front of the tile's first column, 256 columns, 12 behind

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
  __shared__ __attribute__((aligned(16))) uint8_t img[27 * SU_PITCH];
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  float* lsb = lsb_all[wave];
  const int nx = ((a.ow >> 2) + 31) >> 5, ny = (a.oh + 3) >> 2;
  const unsigned nb = (unsigned)(nx * ny * a.n), per = (nb + 7) >> 3;
  const unsigned vb = (blockIdx.x & 7) * per + (blockIdx.x >> 3);
  if (vb >= nb) return;  // block-uniform
  const int bx = (int)(vb % (unsigned)nx);
  const unsigned tq = vb / (unsigned)nx;
  const int by = (int)(tq % (unsigned)ny), b = (int)(tq / (unsigned)ny);

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
    pdst[it] = k < 9 * 66 ? j * SU_PITCH + 4 * piece : -1;
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
      if (pdst[it] >= 0) *reinterpret_cast<uint32_t*>(img + ci * 9 * SU_PITCH + pdst[it]) = pk;
    }
  }
  // (bytes 264 .. 271 of a row are read by the last quads' 16-byte windows and never used: no need to clear them)

  // ---- from here on conv_stem_f32in.hip's kernel unchanged
  const int nrows = a.cin * 9;
  const int c = lane & 31, h = lane >> 5;
  const int owq = a.ow >> 2;
  const int oy = by * 4 + wave;
  int xq = bx * 32 + c;
  const bool qvalid = xq < owq && oy < a.oh;
  if (xq >= owq) xq = owq - 1;

  GemmArgs g;
  g.y = a.y;
  g.scale = a.scale;
  g.bias = a.bias;
  g.M = a.cout;
  g.HWY = a.oh * a.ow;
  g.y_bstride = (size_t)a.cout * a.oh * a.ow;
  g.act = a.act;
  g.alpha = a.alpha;
  g.res = nullptr; g.res_relu = 0; g.y2 = nullptr; g.inv_scale2 = 0.f;
  const v4i af0 = *reinterpret_cast<const v4i*>(afrag + (size_t)lane * 16);
  if (OUT != OUT_I32) stage_scale_bias<1, OUT>(g, 0, lane, lsb);
  __syncthreads();

  // ---- operands: window cr = 5 h + L -> (channel cr / 3, filter row cr % 3) = staged row 9 ci + 2 wave + r3
  uint32_t win[4][5];
#pragma unroll
  for (int L = 0; L < 5; ++L) {
    const int cr = 5 * h + L;
    const int ci = cr / 3, r3 = cr - ci * 3;
    const bool live = cr < nrows / 3;  // (nrows / 3 = 3 Cin windows exist)
    const int lrow = live ? ci * 9 + 2 * wave + r3 : 0;
    const uint8_t* p = img + lrow * SU_PITCH + 8 * c;
    const v2i lo = *reinterpret_cast<const v2i*>(p), hi = *reinterpret_cast<const v2i*>(p + 8);
    const uint32_t m = live ? 0xffffffffu : 0u;
    const uint32_t d0 = (uint32_t)lo[0] & m, d1 = (uint32_t)lo[1] & m, d2 = (uint32_t)hi[0] & m, d3 = (uint32_t)hi[1] & m;
    win[0][L] = __builtin_amdgcn_alignbyte(d1, d0, 3);  // columns 8 xq - 1 ..
    win[1][L] = __builtin_amdgcn_alignbyte(d2, d1, 1);  // 8 xq + 1 ..
    win[2][L] = __builtin_amdgcn_alignbyte(d2, d1, 3);  // 8 xq + 3 ..
    win[3][L] = __builtin_amdgcn_alignbyte(d3, d2, 1);  // 8 xq + 5 ..
  }
  v4i bf[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    bf[j][0] = (int)__builtin_amdgcn_perm(win[j][1], win[j][0], 0x04020100u);
    bf[j][1] = (int)__builtin_amdgcn_perm(win[j][2], win[j][1], 0x05040201u);
    bf[j][2] = (int)__builtin_amdgcn_perm(win[j][3], win[j][2], 0x06050402u);
    bf[j][3] = (int)(win[j][4] & 0x00ffffffu);
  }

  const int hw = oy * a.ow + 4 * xq;
  const int MT = (a.cout + 31) >> 5;
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
    if (qvalid) {
      if (OUT == OUT_I32) {
        gemm_epilogue<1, OUT, true, MFULL, ACT_NONE>(g, acc, mt, h, b, hw, lsb, g.HWY - hw);
      } else {
        switch (a.act) {
          case ACT_RELU: gemm_epilogue<1, OUT, true, MFULL, ACT_RELU>(g, acc, mt, h, b, hw, lsb, g.HWY - hw); break;
          case ACT_RELU6: gemm_epilogue<1, OUT, true, MFULL, ACT_RELU6>(g, acc, mt, h, b, hw, lsb, g.HWY - hw); break;
          case ACT_LEAKY: gemm_epilogue<1, OUT, true, MFULL, ACT_LEAKY>(g, acc, mt, h, b, hw, lsb, g.HWY - hw); break;
          default: gemm_epilogue<1, OUT, true, MFULL, ACT_NONE>(g, acc, mt, h, b, hw, lsb, g.HWY - hw); break;
        }
      }
    }
  }
}

// a.x_inv_scale = 1 / calib scale; afrag = the MFMA A fragments of launch_pack_conv3x3s2_direct's block; im: the image (cs bytes a pixel)
template <int CS>
static void launch_u8in_cs(const DirectS2Args& a, const ImageArgs& im, const int8_t* afrag, int out, hipStream_t s) {
  const int owq = a.ow >> 2;
  const long nblk = (long)((owq + 31) / 32) * ((a.oh + 3) / 4) * a.n;
  const dim3 blocks((unsigned)((nblk + 7) / 8 * 8));
  const bool mfull = a.cout % 32 == 0;
#define PLHIP_STEMU(O)                                                                                                \
  do {                                                                                                                \
    if (mfull) hipLaunchKernelGGL((conv3x3s2_mfma_u8in_kernel<O, true, CS>), blocks, dim3(256), 0, s, a, im, afrag);  \
    else hipLaunchKernelGGL((conv3x3s2_mfma_u8in_kernel<O, false, CS>), blocks, dim3(256), 0, s, a, im, afrag);       \
  } while (0)
  if (out == OUT_I32) PLHIP_STEMU(OUT_I32);
  else if (out == OUT_F32) PLHIP_STEMU(OUT_F32);
  else PLHIP_STEMU(OUT_I8);
#undef PLHIP_STEMU
}

void launch_conv3x3s2_u8in(const DirectS2Args& a, const ImageArgs& im, const int8_t* afrag, int out, hipStream_t s) {
  if (im.cs == 1) launch_u8in_cs<1>(a, im, afrag, out, s);
  else if (im.cs == 3) launch_u8in_cs<3>(a, im, afrag, out, s);
  else launch_u8in_cs<4>(a, im, afrag, out, s);
}

}  // namespace plhip
