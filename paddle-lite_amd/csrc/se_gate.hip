// se_gate.hip — the excite stage of a squeeze-excite block in ONE launch, for gfx950.  Input: the pooled fp32 [N, C] that
// plhip_global_avg_pool_f32 wrote.  It runs what the lowered program runs as five instructions
//   calib[fp32_to_int8] -> conv2d 1x1 C -> Cr [int8_out, + activation] -> conv2d 1x1 Cr -> C [fp32_out] -> hard_sigmoid
// and writes the fp32 gate [N, C], bit-identical to them: int32 accumulators are exact whatever the summation order, the
// epilogue is the convs' own epilogue_f32 (fma(float(acc), s_c, b_c), activation), the first conv's output is quantised with
// round_sat_i8 (its folded scales carry the second conv's input scale), the calib is calib_f32_to_i8_kernel's
// round_sat_i8(inv * x), and hard_sigmoid is hard_act.hip's: a multiply and an add, two roundings.
// One block per image.  The two int8 vectors live in LDS (at most 960 + 960 bytes); weights are tiny (at most 2 x 960 x 240
// bytes) and stay in L2.  Packed weights: dword [k / 4][out] = the four input channels 4 (k / 4) .. + 3 of output `out`, zero
// padded in k, so the lanes of a wave (consecutive outputs) read consecutive dwords and any C, Cr works (72, 88, 184, 200 ...).
#include "plhip_device.h"
#include "plhip_kernels.h"

namespace plhip {

// w [out][in] int8 (a 1x1 conv's filter) -> p [(in + 3) / 4][out] dwords
__global__ __launch_bounds__(256) void se_gate_pack_kernel(const int8_t* __restrict__ w, uint32_t* __restrict__ p, int out, int in) {
  const int k4n = (in + 3) >> 2;
  const int total = k4n * out;
  for (int i = blockIdx.x * 256 + threadIdx.x; i < total; i += gridDim.x * 256) {
    const int k4 = i / out, o = i - k4 * out;
    uint32_t v = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int k = k4 * 4 + j;
      if (k < in) v |= (uint32_t)(uint8_t)w[(size_t)o * in + k] << (8 * j);
    }
    p[i] = v;
  }
}

__global__ __launch_bounds__(256) void se_gate_kernel(SeGateArgs a) {
  __shared__ uint32_t xq[SE_GATE_MAX_C / 4];
  __shared__ uint32_t mid[SE_GATE_MAX_C / 4];
  const int n = blockIdx.x;
  const int c4n = (a.c + 3) >> 2, r4n = (a.cr + 3) >> 2;
  const float* __restrict__ xp = a.pooled + (size_t)n * a.c;
  // calib: four channels per lane, zero padded
  for (int q = threadIdx.x; q < c4n; q += 256) {
    int v[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) v[j] = 4 * q + j < a.c ? round_sat_i8(a.inv * xp[4 * q + j]) : 0;
    xq[q] = pack4_i8(v[0], v[1], v[2], v[3]);
  }
  for (int q = threadIdx.x; q < r4n; q += 256) mid[q] = 0;
  __syncthreads();
  // conv 1: C -> Cr, int8 output into LDS bytes
  int8_t* midb = reinterpret_cast<int8_t*>(mid);
  for (int r = threadIdx.x; r < a.cr; r += 256) {
    int acc = 0;
    for (int k = 0; k < c4n; ++k) acc = __builtin_amdgcn_sdot4((int)a.w1[(size_t)k * a.cr + r], (int)xq[k], acc, false);
    const float y = epilogue_f32(acc, a.s1[r], a.b1 ? a.b1[r] : 0.f, a.act1, a.alpha1);
    midb[r] = (int8_t)round_sat_i8(y);
  }
  __syncthreads();
  // conv 2: Cr -> C, fp32, then hard_sigmoid
  for (int c = threadIdx.x; c < a.c; c += 256) {
    int acc = 0;
    for (int k = 0; k < r4n; ++k) acc = __builtin_amdgcn_sdot4((int)a.w2[(size_t)k * a.c + c], (int)mid[k], acc, false);
    const float y = epilogue_f32(acc, a.s2[c], a.b2 ? a.b2[c] : 0.f, a.act2, a.alpha2);
    float t;
    {
#pragma clang fp contract(off)
      const float m = y * a.slope;
      t = m + a.offset;
    }
    t = t < 1.f ? t : 1.f;
    t = t > 0.f ? t : 0.f;
    a.gate[(size_t)n * a.c + c] = t;
  }
}

size_t se_gate_packed_bytes(int c, int cr) { return ((size_t)((c + 3) / 4) * cr + (size_t)((cr + 3) / 4) * c) * 4; }

void launch_se_gate_pack(const int8_t* w1, const int8_t* w2, void* packed, int c, int cr, hipStream_t s) {
  uint32_t* p1 = static_cast<uint32_t*>(packed);
  uint32_t* p2 = p1 + (size_t)((c + 3) / 4) * cr;
  const int t1 = ((c + 3) / 4) * cr, t2 = ((cr + 3) / 4) * c;
  hipLaunchKernelGGL(se_gate_pack_kernel, dim3((t1 + 255) / 256), dim3(256), 0, s, w1, p1, cr, c);
  hipLaunchKernelGGL(se_gate_pack_kernel, dim3((t2 + 255) / 256), dim3(256), 0, s, w2, p2, c, cr);
}

void launch_se_gate(const SeGateArgs& a, int n, hipStream_t s) { hipLaunchKernelGGL(se_gate_kernel, dim3(n), dim3(256), 0, s, a); }

}  // namespace plhip
