// image_resize.hip — bilinear resize of a uint8 frame on the device: what ImagePreprocess::imageResize runs on the host
// (lite/utils/cv/paddle_image_preprocess.cc:69-98 -> image_resize.cc:184-369 one channel, :564-726 three, :728-895 four).  Per axis
// a host-made table (plhip_image_resize_tables: the reference's double -> float -> int16 sequence, which is the contract and is
// NOT recomputed here) gives a source index and two 11-bit weights; then, per byte k of a pixel, S0 / S1 the source rows sy, sy + 1:
//   rows0 = (S0[sx cs + k] a0 + S0[(sx + 1) cs + k] a1) >> 4      rows1 likewise on S1            (<= 32655, fits int16)
//   dst   = (((b0 rows0) >> 16) + ((b1 rows1) >> 16) + 2) >> 2                                     (int32 products, 0..255)
// One kernel template, three outputs:
//   RESIZE_OUT_U8   the resized interleaved image [n, h_out, w_out, cs]                        (imageResize alone)
//   RESIZE_OUT_F32 / _I8   the normalised NCHW tensor image_to_tensor makes of that image (image_to_tensor.hip: (float(byte) -
//                   mean[c]) * scale[c], two roundings; int8: round_sat_i8(inv * y)); the resized image is never written
// and two sources: an interleaved frame, or (NV != 0) an NV12 / NV21 frame whose four taps are converted to b, g, r while they are
// fetched (nv_pixel_bgr, the arithmetic of image_convert.hip), so the result equals convert -> resize -> image_to_tensor bit for bit.
//
// Streaming kernels.  Vector form (w_out % 16 == 0, y 16-byte aligned): a lane owns 16 consecutive output pixels of one row and
// stores them as 16-byte pieces (uint8: cs pieces; fp32: four per channel plane; int8: one per plane).  A block is one image x a
// band of output rows: 2^l lanes per row (the smallest power of two >= w_out / 16, at most 64), 256 >> l rows per block, so the row
// and the column group of a lane are a shift and a mask of its thread index; the one division of the kernel, block -> (image, band),
// is wave-uniform.  Blocks are mapped XCD-contiguously (block b works on the (b % 8)-th eighth of the bands), so the source rows a
// band shares with its neighbours stay in one L2.  The taps are byte loads: neighbouring lanes read neighbouring source pixels, so
// the loads of a wave fall into few cache lines.  Anything else runs the scalar form: one output pixel per lane and step.
#include "plhip_device.h"
#include "plhip_kernels.h"

namespace plhip {

namespace {

// the cs bytes (C of them used) of output pixel (dy, dx) of image `img`; K = how many bytes of the pixel are wanted
template <int CS, int NV, int K>
__device__ __forceinline__ void resize_pixel(const ResizeArgs& a, const uint8_t* img, int sy, int sx, int a0, int a1, int b0, int b1,
                                             int (&out)[K]) {
  int t00[K], t01[K], t10[K], t11[K];
  if constexpr (NV != 0) {
    static_assert(K == 3, "an NV frame is resized as b, g, r");
    const uint8_t* y0 = img + (int64_t)sy * a.w_in + sx;
    const uint8_t* y1 = y0 + a.w_in;
    const uint8_t* c0 = img + (int64_t)(a.h_in + (sy >> 1)) * a.w_in;
    const uint8_t* c1 = img + (int64_t)(a.h_in + ((sy + 1) >> 1)) * a.w_in;
    const int xa = sx & ~1, xb = (sx + 1) & ~1;
    const int p0a = c0[xa], p0b = c0[xa + 1], p0c = c0[xb], p0d = c0[xb + 1];
    const int p1a = c1[xa], p1b = c1[xa + 1], p1c = c1[xb], p1d = c1[xb + 1];
    nv_pixel_bgr(y0[0], NV == 2 ? p0b : p0a, NV == 2 ? p0a : p0b, t00);
    nv_pixel_bgr(y0[1], NV == 2 ? p0d : p0c, NV == 2 ? p0c : p0d, t01);
    nv_pixel_bgr(y1[0], NV == 2 ? p1b : p1a, NV == 2 ? p1a : p1b, t10);
    nv_pixel_bgr(y1[1], NV == 2 ? p1d : p1c, NV == 2 ? p1c : p1d, t11);
  } else {
    const uint8_t* s0 = img + ((int64_t)sy * a.w_in + sx) * CS;
    const uint8_t* s1 = s0 + (int64_t)a.w_in * CS;
#pragma unroll
    for (int k = 0; k < K; ++k) {
      t00[k] = s0[k];
      t01[k] = s0[CS + k];
      t10[k] = s1[k];
      t11[k] = s1[CS + k];
    }
  }
#pragma unroll
  for (int k = 0; k < K; ++k) {
    const int rows0 = (t00[k] * a0 + t01[k] * a1) >> 4;
    const int rows1 = (t10[k] * a0 + t11[k] * a1) >> 4;
    out[k] = (((b0 * rows0) >> 16) + ((b1 * rows1) >> 16) + 2) >> 2;
  }
}

__device__ __forceinline__ float sel3(const float (&v)[3], int c) { return c == 0 ? v[0] : (c == 1 ? v[1] : v[2]); }

}  // namespace

// lpr_log2: log2 of the lanes per output row; bands: row bands per image; total = n * bands blocks of work, per8 = ceil(total / 8)
template <int CS, int NV, int OUT>
__global__ __launch_bounds__(256) void image_resize_kernel(ResizeArgs a, void* __restrict__ yv, float inv, int vec, int lpr_log2,
                                                           int bands, int total, int per8) {
  constexpr int C = CS == 1 ? 1 : 3;                // channels of the tensor forms
  constexpr int K = OUT == RESIZE_OUT_U8 ? CS : C;  // bytes of a pixel that are computed (the tensor forms drop the 4th)
  const int64_t frame = NV ? (int64_t)(a.h_in / 2 * 3) * a.w_in : (int64_t)a.h_in * a.w_in * CS;
  const int64_t P = (int64_t)a.h_out * a.w_out;
  if (vec) {
    const int lb = (int)(blockIdx.x & 7u) * per8 + (int)(blockIdx.x >> 3);  // XCD-contiguous
    if (lb >= total) return;
    const int b = lb / bands, band = lb - b * bands;
    const int dy = band * (256 >> lpr_log2) + ((int)threadIdx.x >> lpr_log2);
    if (dy >= a.h_out) return;
    const uint8_t* img = a.src + (int64_t)b * frame;
    const int sy = a.yofs[dy], b0 = a.ycoef[2 * dy], b1 = a.ycoef[2 * dy + 1];
    const int groups = a.w_out >> 4;
    for (int g = (int)threadIdx.x & ((1 << lpr_log2) - 1); g < groups; g += 1 << lpr_log2) {
      const v4i* xo = reinterpret_cast<const v4i*>(a.xofs + 16 * g);   // 64-byte aligned: the table is, g * 16 ints
      const v4i* xc = reinterpret_cast<const v4i*>(a.xcoef + 32 * g);  // 16 (a0, a1) int16 pairs = 64 bytes
      int px[16][K];
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const v4i so = xo[q], co = xc[q];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const int a0 = (int)(int16_t)((uint32_t)co[e] & 0xffffu), a1 = co[e] >> 16;
          resize_pixel<CS, NV, K>(a, img, sy, so[e], a0, a1, b0, b1, px[4 * q + e]);
        }
      }
      if (OUT == RESIZE_OUT_U8) {
        uint8_t* o = static_cast<uint8_t*>(yv) + (((int64_t)b * a.h_out + dy) * a.w_out + 16 * g) * CS;
        uint32_t wd[4 * CS];
#pragma unroll
        for (int i = 0; i < 4 * CS; ++i) wd[i] = 0u;
#pragma unroll
        for (int p = 0; p < 16; ++p)
#pragma unroll
          for (int k = 0; k < K; ++k) {
            const int i = p * CS + k;
            wd[i >> 2] |= (uint32_t)px[p][k] << (8 * (i & 3));
          }
#pragma unroll
        for (int j = 0; j < CS; ++j) {
          v4i r;
#pragma unroll
          for (int e = 0; e < 4; ++e) r[e] = (int)wd[4 * j + e];
          reinterpret_cast<v4i*>(o)[j] = r;
        }
      } else {
#pragma unroll
        for (int c = 0; c < C; ++c) {
          const int64_t off = ((int64_t)b * C + c) * P + (int64_t)dy * a.w_out + 16 * g;
          if (OUT == RESIZE_OUT_F32) {
            v4f* o = reinterpret_cast<v4f*>(static_cast<float*>(yv) + off);
#pragma unroll
            for (int k4 = 0; k4 < 4; ++k4) {
              v4f r;
#pragma unroll
              for (int e = 0; e < 4; ++e) r[e] = ((float)px[4 * k4 + e][c] - a.mean[c]) * a.scale[c];
              o[k4] = r;
            }
          } else {
            v4i r;
#pragma unroll
            for (int k4 = 0; k4 < 4; ++k4) {
              int qv[4];
#pragma unroll
              for (int e = 0; e < 4; ++e) qv[e] = round_sat_i8(inv * (((float)px[4 * k4 + e][c] - a.mean[c]) * a.scale[c]));
              r[k4] = (int)pack4_i8(qv[0], qv[1], qv[2], qv[3]);
            }
            *reinterpret_cast<v4i*>(static_cast<int8_t*>(yv) + off) = r;
          }
        }
      }
    }
    return;
  }
  const int64_t pixels = (int64_t)a.n * P;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < pixels; i += stride) {
    const int64_t b = i / P, q = i - b * P;
    const int dy = (int)(q / a.w_out), dx = (int)(q - (int64_t)dy * a.w_out);
    int px[K];
    resize_pixel<CS, NV, K>(a, a.src + b * frame, a.yofs[dy], a.xofs[dx], a.xcoef[2 * dx], a.xcoef[2 * dx + 1], a.ycoef[2 * dy],
                            a.ycoef[2 * dy + 1], px);
#pragma unroll
    for (int k = 0; k < K; ++k) {
      if (OUT == RESIZE_OUT_U8) {
        static_cast<uint8_t*>(yv)[i * CS + k] = (uint8_t)px[k];
      } else {
        const float v = ((float)px[k] - sel3(a.mean, k)) * sel3(a.scale, k);
        if (OUT == RESIZE_OUT_F32) static_cast<float*>(yv)[(b * C + k) * P + q] = v;
        else static_cast<int8_t*>(yv)[(b * C + k) * P + q] = (int8_t)round_sat_i8(inv * v);
      }
    }
  }
}

template <int CS, int NV, int OUT>
static void launch_resize_t(const ResizeArgs& a, void* y, float inv, hipStream_t s) {
  const bool vec = a.w_out % 16 == 0 && ((uintptr_t)y & 15) == 0 && ((uintptr_t)a.xofs & 63) == 0 && ((uintptr_t)a.xcoef & 63) == 0;
  if (vec) {
    const int groups = a.w_out / 16;
    int l = 0;
    while ((1 << l) < groups && l < 6) ++l;
    const int rows = 256 >> l, bands = (a.h_out + rows - 1) / rows;
    const int total = a.n * bands, per8 = (total + 7) / 8;
    hipLaunchKernelGGL((image_resize_kernel<CS, NV, OUT>), dim3(per8 * 8), dim3(256), 0, s, a, y, inv, 1, l, bands, total, per8);
  } else {
    int64_t blocks = ((int64_t)a.n * a.h_out * a.w_out + 255) / 256;
    if (blocks > 16384) blocks = 16384;
    hipLaunchKernelGGL((image_resize_kernel<CS, NV, OUT>), dim3((unsigned)blocks), dim3(256), 0, s, a, y, inv, 0, 0, 1, 0, 0);
  }
}

template <int CS, int NV>
static void launch_resize_o(const ResizeArgs& a, void* y, int out, float inv, hipStream_t s) {
  if (out == RESIZE_OUT_U8) launch_resize_t<CS, NV, RESIZE_OUT_U8>(a, y, inv, s);
  else if (out == RESIZE_OUT_F32) launch_resize_t<CS, NV, RESIZE_OUT_F32>(a, y, inv, s);
  else launch_resize_t<CS, NV, RESIZE_OUT_I8>(a, y, inv, s);
}

void launch_image_resize(const ResizeArgs& a, void* y, int out, float calib_scale, hipStream_t s) {
  const float inv = out == RESIZE_OUT_I8 ? 1.f / calib_scale : 0.f;  // type_trans.cc:45, as launch_calib_f32_to_i8
  if (a.nv == 1) launch_resize_o<3, 1>(a, y, out, inv, s);
  else if (a.nv == 2) launch_resize_o<3, 2>(a, y, out, inv, s);
  else if (a.cs == 1) launch_resize_o<1, 0>(a, y, out, inv, s);
  else if (a.cs == 3) launch_resize_o<3, 0>(a, y, out, inv, s);
  else launch_resize_o<4, 0>(a, y, out, inv, s);
}

}  // namespace plhip
