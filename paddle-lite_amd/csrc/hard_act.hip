// hard_act.hip — the fp32 ops MobileNetV3 adds to the int8 programs, for gfx950: hard_swish, hard_sigmoid and the
// squeeze-excite multiply (elementwise_mul with a per-(image, channel) operand).
//
// Replaces (reference, ARM — fp32 only there, the int8 conv fuses relu / relu6 / leaky_relu alone,
// lite/core/mir/fusion/conv_activation_fuse_pass.cc:26-44):
//   hard_swish      HardSwishCompute lite/kernels/arm/activation_compute.cc:150-195 -> act_hard_swish<float>
//                   lite/backends/arm/math/activation.cc:716-731:  min(max(0.f, x + offset), threshold) * x / scale
//                   left to right: one add, one multiply, one IEEE division, each rounded to fp32
//   hard_sigmoid    HardSigmoidCompute (:319-345) -> act_hard_sigmoid<float> activation.cc:678-691:
//                   t = x * slope + offset (TWO roundings, no fma); t = t < 1 ? t : 1; t = t > 0 ? t : 0
//   elementwise_mul ElementwiseMulCompute lite/kernels/arm/elementwise_compute.cc:30-84, the fast-broadcast case
//                   pre = 1, n = N * C, post = H * W:  out[p][i] = x[p][i] * y[p]
// The comparisons are written as the reference writes them (std::max(0.f, v) is 0.f < v ? v : 0.f, std::min(a, t) is
// t < a ? t : a), which fixes the results for NaN and the infinities.
// Every kernel can write the fp32 result, the int8 result of the calib[fp32_to_int8] behind it, or both; the int8 form
// quantises exactly as calib_f32_to_i8_kernel does: round_sat_i8(inv * y), inv = 1 / calib scale (never folded into
// the op's constants).
// Plain HBM streams: 16 bytes per lane where the pointers and the element count allow, a scalar loop otherwise; no LDS.
#include "plhip_device.h"
#include "plhip_kernels.h"

namespace plhip {

namespace {

template <int KIND>
__device__ __forceinline__ float hard_act(float x, float p0, float p1, float p2) {
#pragma clang fp contract(off)
  if (KIND == HARD_ACT_SWISH) {  // p0 threshold, p1 scale, p2 offset
    float t = x + p2;
    t = 0.f < t ? t : 0.f;
    t = p0 < t ? p0 : t;
    const float m = t * x;
    return m / p1;  // a real division: 1 / 6 is not representable, a multiply by the reciprocal gives other bits
  } else {  // p0 slope, p1 offset
    const float m = x * p0;
    float t = m + p1;
    t = t < 1.f ? t : 1.f;
    t = t > 0.f ? t : 0.f;
    return t;
  }
}

__device__ __forceinline__ void store4(float* __restrict__ yf, int8_t* __restrict__ yq, int64_t quad, const v4f& r, float inv) {
  if (yf) reinterpret_cast<v4f*>(yf)[quad] = r;
  if (yq)
    reinterpret_cast<uint32_t*>(yq)[quad] = calib4_i8(r, inv);
}

__device__ __forceinline__ void store1(float* __restrict__ yf, int8_t* __restrict__ yq, int64_t i, float r, float inv) {
  if (yf) yf[i] = r;
  if (yq) yq[i] = (int8_t)round_sat_i8(inv * r);
}

// 16-byte fp32 accesses and 4-byte int8 stores at multiples of 4 elements from the bases
int stream_vec(const float* x, const float* yf, const int8_t* yq) {
  return (((uintptr_t)x | (uintptr_t)yf) & 15) == 0 && ((uintptr_t)yq & 3) == 0;
}

}  // namespace

// yf / yq: either may be null (not both).  vec: host decides, uniform.
template <int KIND>
__global__ __launch_bounds__(256) void hard_act_kernel(const float* __restrict__ x, float* __restrict__ yf, int8_t* __restrict__ yq,
                                                       float p0, float p1, float p2, float inv, int64_t count, int vec) {
  const int64_t nq = vec ? count >> 2 : 0;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < nq; i += stride) {
    const v4f v = reinterpret_cast<const v4f*>(x)[i];
    v4f r;
#pragma unroll
    for (int j = 0; j < 4; ++j) r[j] = hard_act<KIND>(v[j], p0, p1, p2);
    store4(yf, yq, i, r, inv);
  }
  for (int64_t t = (nq << 2) + (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < count; t += stride)
    store1(yf, yq, t, hard_act<KIND>(x[t], p0, p1, p2), inv);
}

void launch_hard_act(int kind, const float* params, const float* x, float* yf, int8_t* yq, float calib_scale, int64_t count,
                     hipStream_t s) {
  const float inv = yq ? 1.f / calib_scale : 0.f;  // type_trans.cc:45, as launch_calib_f32_to_i8
  const int vec = stream_vec(x, yf, yq);
  int64_t b = ((vec ? count >> 2 : count) + 255) / 256;
  if (b < 1) b = 1;
  if (b > 16384) b = 16384;
  if (kind == HARD_ACT_SWISH)
    hipLaunchKernelGGL(hard_act_kernel<HARD_ACT_SWISH>, dim3((unsigned)b), dim3(256), 0, s, x, yf, yq, params[0], params[1], params[2],
                       inv, count, vec);
  else
    hipLaunchKernelGGL(hard_act_kernel<HARD_ACT_SIGMOID>, dim3((unsigned)b), dim3(256), 0, s, x, yf, yq, params[0], params[1], 0.f,
                       inv, count, vec);
}

// out[p][i] = x[p][i] * g[p], p < planes, i < hw.  A group of 1 << LPP lanes owns one plane: the gate is one load per
// lane (LPP == 8: the block owns the plane, the gate is one scalar load), and no lane divides to find its plane.
// vec (host decides: hw % 4 == 0 and aligned bases, so every plane starts 16-byte aligned): a lane takes quads of its plane.
template <int LPP>
__global__ __launch_bounds__(256) void se_scale_kernel(const float* __restrict__ x, const float* __restrict__ g, float* __restrict__ yf,
                                                       int8_t* __restrict__ yq, float inv, int64_t planes, int hw, int vec) {
  const int64_t plane = LPP == 8 ? (int64_t)blockIdx.x : ((int64_t)blockIdx.x * 256 + threadIdx.x) >> LPP;
  if (plane >= planes) return;
  const int sub = threadIdx.x & ((1 << LPP) - 1);
  const float gv = g[plane];
  const int64_t base = plane * hw;
  if (vec) {
    const int nq = hw >> 2;
    const int64_t qbase = base >> 2;
    for (int q = sub; q < nq; q += 1 << LPP) {
      const v4f v = reinterpret_cast<const v4f*>(x)[qbase + q];
      v4f r;
#pragma unroll
      for (int j = 0; j < 4; ++j) r[j] = v[j] * gv;
      store4(yf, yq, qbase + q, r, inv);
    }
    return;
  }
  for (int i = sub; i < hw; i += 1 << LPP) store1(yf, yq, base + i, x[base + i] * gv, inv);
}

void launch_se_scale(const float* x, const float* g, float* yf, int8_t* yq, float calib_scale, int64_t planes, int hw, hipStream_t s) {
  const float inv = yq ? 1.f / calib_scale : 0.f;
  const int vec = (hw & 3) == 0 && stream_vec(x, yf, yq);
  const int work = vec ? hw >> 2 : hw;  // items a plane's lanes share
  const int lpp = work <= 2 ? 0 : work <= 32 ? 4 : work <= 128 ? 6 : 8;
  const unsigned blocks = (unsigned)(((planes << lpp) + 255) / 256);
  if (lpp == 0) hipLaunchKernelGGL(se_scale_kernel<0>, dim3(blocks), dim3(256), 0, s, x, g, yf, yq, inv, planes, hw, vec);
  else if (lpp == 4) hipLaunchKernelGGL(se_scale_kernel<4>, dim3(blocks), dim3(256), 0, s, x, g, yf, yq, inv, planes, hw, vec);
  else if (lpp == 6) hipLaunchKernelGGL(se_scale_kernel<6>, dim3(blocks), dim3(256), 0, s, x, g, yf, yq, inv, planes, hw, vec);
  else hipLaunchKernelGGL(se_scale_kernel<8>, dim3(blocks), dim3(256), 0, s, x, g, yf, yq, inv, planes, hw, vec);
}

}  // namespace plhip
