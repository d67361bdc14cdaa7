// image_to_tensor.hip — uint8 interleaved image [n, h, w, cs] -> normalised NCHW tensor on the device: what
// ImagePreprocess::image_to_tensor runs on the host (lite/utils/cv/paddle_image_preprocess.cc:143-172 -> image2tensor.cc).
//   y[b][c][h][w] = (float(src[((b h + h) w + w) cs + c]) - means[c]) * scales[c]            (image2tensor.cc:481-488, 549-563)
// two fp32 roundings, a subtract then a multiply, as the NEON vsubq_f32 / vmulq_f32 pair; channel c of the output is source byte c of
// the pixel, in the image's own order (BGR and RGB alike, Image2Tensor::choose), the 4th byte of BGRA / RGBA is dropped, GRAY gives one
// channel.  The int8 form adds calib[fp32_to_int8] exactly as calib_f32_to_i8_kernel does: round_sat_i8(inv * y), inv = 1 / scale.
//
// Both kernels are plain streams.  Because an NCHW channel plane of one image is contiguous over its h * w pixels, a lane takes 16
// consecutive pixels of one image (16 cs bytes in cs 16-byte loads) and writes 16 values per channel plane (fp32: four 16-byte
// stores, int8: one), wherever h * w % 16 == 0 and both pointers are 16-byte aligned.  Anything else runs the scalar loop: one
// output value per lane and step.
#include "plhip_device.h"
#include "plhip_kernels.h"

namespace plhip {

namespace {

__device__ __forceinline__ float chan_sel(const float (&v)[3], int c) {  // (no dynamic index into the argument: no scratch)
  return c == 0 ? v[0] : (c == 1 ? v[1] : v[2]);
}

template <int CS>
__device__ __forceinline__ float pixel_byte(const uint32_t (&wd)[4 * CS], int k, int c) {  // byte c of pixel k, k and c constant
  const int i = k * CS + c;
  return (float)((wd[i >> 2] >> (8 * (i & 3))) & 0xffu);
}

template <int CS>
__device__ __forceinline__ void load_pixels16(const uint8_t* src, uint32_t (&wd)[4 * CS]) {
  const v4i* s = reinterpret_cast<const v4i*>(src);
#pragma unroll
  for (int j = 0; j < CS; ++j) {
    const v4i v = s[j];
    wd[4 * j] = (uint32_t)v[0];
    wd[4 * j + 1] = (uint32_t)v[1];
    wd[4 * j + 2] = (uint32_t)v[2];
    wd[4 * j + 3] = (uint32_t)v[3];
  }
}

constexpr int64_t kMaxBlocks = 16384;

unsigned stream_blocks(int64_t work) {
  int64_t b = (work + 255) / 256;
  if (b < 1) b = 1;
  if (b > kMaxBlocks) b = kMaxBlocks;
  return (unsigned)b;
}

}  // namespace

// y: fp32 NCHW [n, C, h, w]; vec: h * w % 16 == 0 and 16-byte aligned pointers (host decides, uniform)
template <int CS>
__global__ __launch_bounds__(256) void image_to_tensor_f32_kernel(ImageArgs a, float* __restrict__ y, int vec) {
  constexpr int C = CS == 1 ? 1 : 3;
  const int64_t P = (int64_t)a.h * a.w;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  if (vec) {
    const int64_t groups = (int64_t)a.n * P / 16;
    for (int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; g < groups; g += stride) {
      const int64_t p0 = g * 16, b = p0 / P, q = p0 - b * P;
      uint32_t wd[4 * CS];
      load_pixels16<CS>(a.src + p0 * CS, wd);
#pragma unroll
      for (int c = 0; c < C; ++c) {
        v4f* o = reinterpret_cast<v4f*>(y + (b * C + c) * P + q);
#pragma unroll
        for (int k4 = 0; k4 < 4; ++k4) {
          v4f r;
#pragma unroll
          for (int e = 0; e < 4; ++e) r[e] = (pixel_byte<CS>(wd, 4 * k4 + e, c) - a.mean[c]) * a.scale[c];
          o[k4] = r;
        }
      }
    }
    return;
  }
  const int64_t total = (int64_t)a.n * C * P;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += stride) {
    const int64_t b = i / (C * P), r = i - b * C * P;
    const int c = (int)(r / P);
    const int64_t q = r - c * P;
    y[i] = ((float)a.src[(b * P + q) * CS + c] - chan_sel(a.mean, c)) * chan_sel(a.scale, c);
  }
}

// y: int8 NCHW; the quantiser of calib_f32_to_i8_kernel with inv = 1 / calib scale (launch_calib_f32_to_i8)
template <int CS>
__global__ __launch_bounds__(256) void image_to_tensor_i8_kernel(ImageArgs a, int8_t* __restrict__ y, float inv, int vec) {
  constexpr int C = CS == 1 ? 1 : 3;
  const int64_t P = (int64_t)a.h * a.w;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  if (vec) {
    const int64_t groups = (int64_t)a.n * P / 16;
    for (int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; g < groups; g += stride) {
      const int64_t p0 = g * 16, b = p0 / P, q = p0 - b * P;
      uint32_t wd[4 * CS];
      load_pixels16<CS>(a.src + p0 * CS, wd);
#pragma unroll
      for (int c = 0; c < C; ++c) {
        v4i r;
#pragma unroll
        for (int k4 = 0; k4 < 4; ++k4) {
          int qv[4];
#pragma unroll
          for (int e = 0; e < 4; ++e) qv[e] = round_sat_i8(inv * ((pixel_byte<CS>(wd, 4 * k4 + e, c) - a.mean[c]) * a.scale[c]));
          r[k4] = (int)pack4_i8(qv[0], qv[1], qv[2], qv[3]);
        }
        *reinterpret_cast<v4i*>(y + (b * C + c) * P + q) = r;
      }
    }
    return;
  }
  const int64_t total = (int64_t)a.n * C * P;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += stride) {
    const int64_t b = i / (C * P), r = i - b * C * P;
    const int c = (int)(r / P);
    const int64_t q = r - c * P;
    y[i] = (int8_t)round_sat_i8(inv * (((float)a.src[(b * P + q) * CS + c] - chan_sel(a.mean, c)) * chan_sel(a.scale, c)));
  }
}

static int image_vec(const ImageArgs& a, const void* y) {
  return ((int64_t)a.h * a.w) % 16 == 0 && ((uintptr_t)a.src & 15) == 0 && ((uintptr_t)y & 15) == 0;
}

void launch_image_to_tensor_f32(const ImageArgs& a, float* y, hipStream_t s) {
  const int vec = image_vec(a, y);
  const int64_t P = (int64_t)a.h * a.w;
  const unsigned blocks = stream_blocks(vec ? a.n * P / 16 : a.n * a.c * P);
  if (a.cs == 1) hipLaunchKernelGGL(image_to_tensor_f32_kernel<1>, dim3(blocks), dim3(256), 0, s, a, y, vec);
  else if (a.cs == 3) hipLaunchKernelGGL(image_to_tensor_f32_kernel<3>, dim3(blocks), dim3(256), 0, s, a, y, vec);
  else hipLaunchKernelGGL(image_to_tensor_f32_kernel<4>, dim3(blocks), dim3(256), 0, s, a, y, vec);
}

void launch_image_to_tensor_i8(const ImageArgs& a, int8_t* y, float calib_scale, hipStream_t s) {
  const float inv = 1.f / calib_scale;  // type_trans.cc:45, as launch_calib_f32_to_i8
  const int vec = image_vec(a, y);
  const int64_t P = (int64_t)a.h * a.w;
  const unsigned blocks = stream_blocks(vec ? a.n * P / 16 : a.n * a.c * P);
  if (a.cs == 1) hipLaunchKernelGGL(image_to_tensor_i8_kernel<1>, dim3(blocks), dim3(256), 0, s, a, y, inv, vec);
  else if (a.cs == 3) hipLaunchKernelGGL(image_to_tensor_i8_kernel<3>, dim3(blocks), dim3(256), 0, s, a, y, inv, vec);
  else hipLaunchKernelGGL(image_to_tensor_i8_kernel<4>, dim3(blocks), dim3(256), 0, s, a, y, inv, vec);
}

}  // namespace plhip
