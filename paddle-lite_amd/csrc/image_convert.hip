// image_convert.hip — NV12 / NV21 camera frame -> interleaved BGR (or BGRA, 4th byte 255) on the device: what
// ImagePreprocess::imageConvert runs on the host (lite/utils/cv/paddle_image_preprocess.cc:44-67 -> image_convert.cc:175-518, the
// scalar tail :451-514 states the arithmetic).  A frame is [n][h * 3 / 2][w] bytes: h rows of Y, then h / 2 rows of interleaved
// chroma, one pair per 2 x 2 luma block, (u, v) for NV12 and (v, u) for NV21.  Integer arithmetic, >> arithmetic on negatives:
//   ra = (179 (v - 128)) >> 7   ga = (44 (u - 128) + 91 (v - 128)) >> 7   ba = (227 (u - 128)) >> 7
//   r = clamp(y + ra)   g = clamp(y - ga)   b = clamp(y + ba)   to 0..255, bytes written in the order b, g, r
// (nv_pixel_bgr in plhip_kernels.h, shared with the fused frame kernel of image_resize.hip).
//
// A plain stream.  A lane takes a 2 x 16 luma block so that each chroma pair is loaded once: two 16-byte luma loads, one 16-byte
// chroma load, and per luma row 3 (BGR) or 4 (BGRA) 16-byte stores, wherever w % 16 == 0 and both pointers are 16-byte aligned.
// Anything else runs the scalar form: a 2 x 2 block per lane, byte stores.  The grid carries the index: x = column groups,
// y = row pairs, z = image; no division in the kernel.
#include "plhip_device.h"
#include "plhip_kernels.h"

namespace plhip {

namespace {

__device__ __forceinline__ uint32_t byte_of(const v4i& v, int i) {  // i constant
  return ((uint32_t)v[i >> 2] >> (8 * (i & 3))) & 0xffu;
}

}  // namespace

// DCS: bytes per destination pixel (3 BGR, 4 BGRA); VEC: the 2 x 16 block form
template <int NV21, int DCS, int VEC>
__global__ __launch_bounds__(256) void nv_to_bgr_u8_kernel(NvArgs a, uint8_t* __restrict__ y) {
  const int g = blockIdx.x * blockDim.x + threadIdx.x;  // column group
  const int rp = blockIdx.y * blockDim.y + threadIdx.y;  // row pair
  const int b = blockIdx.z;
  constexpr int K = VEC ? 16 : 2;
  if (g * K >= a.w || 2 * rp >= a.h) return;
  const uint8_t* frame = a.src + (int64_t)b * (a.h / 2 * 3) * a.w;
  const uint8_t* y0 = frame + (int64_t)(2 * rp) * a.w + g * K;
  const uint8_t* uv = frame + (int64_t)(a.h + rp) * a.w + g * K;
  uint8_t* o0 = y + ((int64_t)b * a.h + 2 * rp) * a.w * DCS + (int64_t)g * K * DCS;
  uint8_t* o1 = o0 + (int64_t)a.w * DCS;
  if (VEC) {
    const v4i l0 = *reinterpret_cast<const v4i*>(y0);
    const v4i l1 = *reinterpret_cast<const v4i*>(y0 + a.w);
    const v4i c = *reinterpret_cast<const v4i*>(uv);
    uint32_t w0[4 * DCS], w1[4 * DCS];
#pragma unroll
    for (int i = 0; i < 4 * DCS; ++i) w0[i] = w1[i] = 0u;
#pragma unroll
    for (int k = 0; k < 16; ++k) {
      const int c0 = (int)byte_of(c, k & ~1), c1 = (int)byte_of(c, k | 1);
      const int u = NV21 ? c1 : c0, v = NV21 ? c0 : c1;
      int p0[3], p1[3];
      nv_pixel_bgr((int)byte_of(l0, k), u, v, p0);
      nv_pixel_bgr((int)byte_of(l1, k), u, v, p1);
#pragma unroll
      for (int e = 0; e < DCS; ++e) {
        const int i = k * DCS + e;
        w0[i >> 2] |= (uint32_t)(e < 3 ? p0[e] : 255) << (8 * (i & 3));
        w1[i >> 2] |= (uint32_t)(e < 3 ? p1[e] : 255) << (8 * (i & 3));
      }
    }
#pragma unroll
    for (int j = 0; j < DCS; ++j) {
      v4i r0, r1;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        r0[e] = (int)w0[4 * j + e];
        r1[e] = (int)w1[4 * j + e];
      }
      reinterpret_cast<v4i*>(o0)[j] = r0;
      reinterpret_cast<v4i*>(o1)[j] = r1;
    }
    return;
  }
  const int c0 = uv[0], c1 = uv[1];
  const int u = NV21 ? c1 : c0, v = NV21 ? c0 : c1;
#pragma unroll
  for (int k = 0; k < 2; ++k) {
    int p0[3], p1[3];
    nv_pixel_bgr(y0[k], u, v, p0);
    nv_pixel_bgr(y0[a.w + k], u, v, p1);
#pragma unroll
    for (int e = 0; e < DCS; ++e) {
      o0[k * DCS + e] = (uint8_t)(e < 3 ? p0[e] : 255);
      o1[k * DCS + e] = (uint8_t)(e < 3 ? p1[e] : 255);
    }
  }
}

template <int NV21, int DCS>
static void launch_nv(const NvArgs& a, uint8_t* y, hipStream_t s) {
  const bool vec = a.w % 16 == 0 && ((uintptr_t)a.src & 15) == 0 && ((uintptr_t)y & 15) == 0;
  const int groups = a.w / (vec ? 16 : 2), pairs = a.h / 2;
  const dim3 block(64, 4), grid((groups + 63) / 64, (pairs + 3) / 4, a.n);
  if (vec) hipLaunchKernelGGL((nv_to_bgr_u8_kernel<NV21, DCS, 1>), grid, block, 0, s, a, y);
  else hipLaunchKernelGGL((nv_to_bgr_u8_kernel<NV21, DCS, 0>), grid, block, 0, s, a, y);
}

void launch_nv_to_bgr(const NvArgs& a, uint8_t* y, int dst_cs, hipStream_t s) {
  if (a.nv21) {
    if (dst_cs == 3) launch_nv<1, 3>(a, y, s);
    else launch_nv<1, 4>(a, y, s);
  } else {
    if (dst_cs == 3) launch_nv<0, 3>(a, y, s);
    else launch_nv<0, 4>(a, y, s);
  }
}

}  // namespace plhip
