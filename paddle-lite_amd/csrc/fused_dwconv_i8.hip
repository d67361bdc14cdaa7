// fused_dwconv_i8.hip — depthwise 3x3 [int8_out] followed by the 1x1 conv that consumes it, with that conv's graph tail, in
// ONE launch (fusion G, plhip_dw_conv1x1_fused_int8).  Shape-general at run time: any n, h, w; C % 16 == 0, C <= 1024;
// M % 8 == 0, M <= 1024; stride 1 | 2; each padding 0 | 1.  Bit-identical to plhip_depthwise_conv_int8 (int8 out) followed by
// plhip_conv2d_int8 (no tail) or plhip_conv2d_int8_fused (tail).
//
// Replaces the instruction pair of the MobileNetV2 blocks
//   depthwise_conv2d[int8_out]                      (lite/kernels/arm/conv_depthwise.cc)
//   conv2d 1x1 [int8_out | fp32_out + residual add + calib]   (lite/kernels/arm/conv_gemmlike.cc + the kHIP conv tail fusion)
// where the int8 depthwise tensor would otherwise make a full HBM round trip.
//
// Structure (a producer / consumer split, so that a GEMM can later be put in front of the producer):
//   * tile = TR whole output rows of ONE image (rows wider than 128 columns: 128-column segments), <= 128 pixels = NT <= 4
//     n tiles of 32; grid.y splits the M output channels when the (32-channel m tile, n tile) pairs of a tile exceed 32 (4 waves
//     x 8 accumulators).  256 threads = 4 waves;
//   * K-step (32 channels) loop, double-buffered, ONE barrier per K-step: while the waves run the depthwise stage of K-step k
//     (VALU: v_dot4) they also issue the input rows of K-step k + 1 (global -> LDS) and the MFMAs of K-step k - 1;
//   * STAGE: the tile's input rows (IR = (TR - 1) stride + 3 per channel) are copied ONCE into LDS [32 ch][IR][WP]: aligned
//     dwords when w % 4 == 0, bytes otherwise; padding rows / columns are zeros written once per block, so the depthwise stage
//     needs no bounds checks and every input byte is fetched once per tile instead of once per tap;
//   * PRODUCE (the rows-in-registers body of the depthwise kernel): a lane = 4 consecutive outputs of one channel row; per
//     filter row 3 (stride 1) or 4 (stride 2) aligned LDS dwords, the four windows cut by v_alignbyte_b32 and multiplied with
//     the packed filter row by v_dot4_i32_i8; the depthwise kernel's requantisation on doubled values (requant4_nn_rtz /
//     pack4_nn_rtz for relu / relu6, requant4 otherwise); 4 bytes into the activation tile [pixel][32 ch + 16 pad].
//     Channels >= C are zeros, so the last K-step of C = 144 adds exactly 0 against the zero-padded weights;
//   * CONSUME: v_mfma_i32_32x32x32_i8, A = the 1x1 conv's weight fragments straight from plhip_pack_conv_weights' order
//     [MT32][KS][64][16] (global, L2-resident), B = 16 channels of one pixel per lane from the tile (ds_read_b128);
//   * epilogue: gemm_epilogue.h's semantics element by element (lane = pixel, so 32 lanes store 32 consecutive pixels of a
//     channel row): int32 accumulators, int8 output, or fp32 with the optional residual add (+ relu), fp32 copy and calib copy.
//     Rows m >= M and pixels outside the tile's rows / columns are never stored.
// Occupancy: LDS 2 x 32 IR WP + 2 x 128 x 48 bytes (<= 64 KiB by the plan: >= 2 blocks per CU); registers decide at NACC = 8
// (2 waves per SIMD = 2 blocks per CU), NACC <= 4 allows 3 or more.
#include "plhip_device.h"
#include "plhip_kernels.h"
#include "dw_common.h"

namespace plhip {

// (DC_APITCH, DC_THREADS: dw_plan.h, which sizes the launch with them)

// bytes O .. O + 3 of the dword array d (compile-time O)
template <int O, int ND>
__device__ __forceinline__ uint32_t dc_window(const uint32_t (&d)[ND]) {
  constexpr int idx = O >> 2, sft = O & 3;
  static_assert(idx + (sft ? 1 : 0) < ND, "window outside the loaded dwords");
  if (sft == 0) return d[idx];
  return __builtin_amdgcn_alignbyte(d[(idx + 1 < ND) ? idx + 1 : idx], d[idx], sft);
}

// S: stride, PL: left padding (compile time: the window offsets 4 - PL + j S of the four outputs of a lane)
template <int NACC, int OUT, int S, int PL>
__global__ __launch_bounds__(DC_THREADS) void dw_conv1x1_fused_kernel(DwConvArgs a) {
  extern __shared__ __attribute__((aligned(16))) uint8_t dc_lds[];  // [2][32][IR][WP] staged rows, [2][NT 32][48] tile
  constexpr int ND = (7 + 3 * S) / 4 + 1;                          // dwords per filter row and lane
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int xsz = 32 * a.IR * a.WP, asz = a.NT * 32 * DC_APITCH;
  uint8_t* const act0 = dc_lds + 2 * xsz;
  const int b = (int)fastdiv_u31(blockIdx.x, a.tpi_m, a.tpi_s);
  const int tt = (int)blockIdx.x - b * a.tpi;
  const int ty = (int)fastdiv_u31((uint32_t)tt, a.ctl_m, a.ctl_s), tx = tt - ty * a.cw_tiles;
  const int oy0 = ty * a.TR, cx0 = tx * a.CW;
  const int TRv = min(a.TR, a.oh - oy0), CWv = min(a.CW, a.ow - cx0);
  const int iy0 = oy0 * S - a.pt;
  const int ixb = cx0 * S - 4;  // input column of byte 0 of a staged row (the left padding column sits at byte 3)
  const int HW = a.oh * a.ow;

  for (int i = tid; i < (2 * xsz) >> 2; i += DC_THREADS) reinterpret_cast<uint32_t*>(dc_lds)[i] = 0u;

  // ---------------------------------------------------------------- stage: input rows of K-step ks -> LDS buffer buf
  int lr = 0, u0 = lane;
  if (a.rpp > 1) {
    lr = lane / a.wu;
    u0 = lane - lr * a.wu;
  }
  auto stage = [&](int ks, int buf) __attribute__((always_inline)) {
    uint8_t* const xs = dc_lds + buf * xsz;
    const int rows = 32 * a.IR;
    for (int rb = wave * a.rpp; rb < rows; rb += 4 * a.rpp) {
      const int rr = rb + lr;
      if (lr >= a.rpp || rr >= rows) continue;
      const int cl = (int)fastdiv_u31((uint32_t)rr, a.ir_m, a.ir_s), t = rr - cl * a.IR;
      const int c = ks * 32 + cl, iy = iy0 + t;
      if (c >= a.C || iy < 0 || iy >= a.h) continue;  // stays zero (padding rows) or is never read (channels >= C)
      const int8_t* const xr = a.x + ((b * a.C + c) * a.h + iy) * a.w;
      uint8_t* const dst = xs + rr * a.WP;
      if (a.dword_stage) {
        for (int u = u0; u < a.wu; u += 64) {
          const int ix = ixb + 4 * u;
          if (ix >= 0 && ix < a.w) *reinterpret_cast<uint32_t*>(dst + 4 * u) = *reinterpret_cast<const uint32_t*>(xr + ix);
        }
      } else {
        for (int u = u0; u < a.wu; u += 64) {
          const int ix = ixb + u;
          if (ix >= 0 && ix < a.w) dst[u] = (uint8_t)xr[ix];
        }
      }
    }
  };

  // ---------------------------------------------------------------- produce: depthwise of K-step ks -> activation tile buf
  const bool dwnn = a.dw_act == ACT_RELU || a.dw_act == ACT_RELU6;
  // (requant_hi2 / requant_leak, plhip_device.h, written out: through the functions this unit's ISA moves)
  const float dw_hi2 = a.dw_act == ACT_RELU6 ? fminf(a.dw_alpha + a.dw_alpha, 254.f) : 254.f;
  const float dw_leak = a.dw_act == ACT_LEAKY ? a.dw_alpha : 1.f;
  const int owq = (a.CW + 3) >> 2;
  const int ptotal = 32 * a.TR * owq;
  auto produce = [&](int ks, int buf) __attribute__((always_inline)) {
    const uint8_t* const xs = dc_lds + buf * xsz;
    uint8_t* const act = act0 + buf * asz;
    for (int it = tid; it < ptotal; it += DC_THREADS) {
      const int rest = (int)fastdiv_u31((uint32_t)it, a.owq_m, a.owq_s), x4 = it - rest * owq;
      const int cl = (int)fastdiv_u31((uint32_t)rest, a.tr_m, a.tr_s), o = rest - cl * a.TR;
      const int x0 = 4 * x4;
      if (o >= TRv || x0 >= CWv) continue;
      const int c = ks * 32 + cl;
      uint32_t pk = 0;
      if (c < a.C) {
        const int8_t* const wp = a.dw_w + c * 9;
        uint32_t wr[3];
        dw_filter_rows3(wp, wr);
        int acc4[4] = {0, 0, 0, 0};
#pragma unroll
        for (int r = 0; r < 3; ++r) {
          const uint32_t* rp = reinterpret_cast<const uint32_t*>(xs + (cl * a.IR + o * S + r) * a.WP + x0 * S);
          uint32_t d[ND];
#pragma unroll
          for (int i = 0; i < ND; ++i) d[i] = rp[i];
          acc4[0] = __builtin_amdgcn_sdot4((int)dc_window<4 - PL + 0 * S, ND>(d), (int)wr[r], acc4[0], false);
          acc4[1] = __builtin_amdgcn_sdot4((int)dc_window<4 - PL + 1 * S, ND>(d), (int)wr[r], acc4[1], false);
          acc4[2] = __builtin_amdgcn_sdot4((int)dc_window<4 - PL + 2 * S, ND>(d), (int)wr[r], acc4[2], false);
          acc4[3] = __builtin_amdgcn_sdot4((int)dc_window<4 - PL + 3 * S, ND>(d), (int)wr[r], acc4[3], false);
        }
        const float s = a.dw_scale[c], bb = a.dw_bias ? a.dw_bias[c] : 0.f;
        pk = dwnn ? requant4_nn_rtz(acc4, s + s, bb + bb, dw_hi2) : requant4<ACT_LEAKY>(acc4, s + s, bb + bb, dw_leak, -254.f, 254.f);
      }
      uint8_t* const ap = act + (o * a.CW + x0) * DC_APITCH + cl;
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if (x0 + j < CWv) ap[j * DC_APITCH] = (uint8_t)(pk >> (8 * j));
    }
  };

  // ---------------------------------------------------------------- consume: MFMAs of K-step ks from tile buf
  const int P = a.mtpb * a.NT;
  const int mg0 = (int)blockIdx.y * a.mtpb;
  int pm[NACC], pn[NACC];
  v16i acc[NACC];
#pragma unroll
  for (int i = 0; i < NACC; ++i) {
    const int idx = wave + 4 * i;
    pm[i] = mg0 + idx % a.mtpb;
    pn[i] = idx / a.mtpb;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[i][r] = 0;
  }
  const uint8_t* const wpk = reinterpret_cast<const uint8_t*>(a.wp);
  const int col = lane & 31, kh = lane >> 5;
  auto consume = [&](int ks, int buf) __attribute__((always_inline)) {
    const uint8_t* const act = act0 + buf * asz;
#pragma unroll
    for (int i = 0; i < NACC; ++i) {
      if (wave + 4 * i < P && pm[i] < a.mt32) {  // wave-uniform
        const v4i av = *reinterpret_cast<const v4i*>(wpk + (((size_t)pm[i] * a.KS + ks) * 64 + lane) * 16);
        const v4i bv = *reinterpret_cast<const v4i*>(act + (pn[i] * 32 + col) * DC_APITCH + 16 * kh);
        acc[i] = __builtin_amdgcn_mfma_i32_32x32x32_i8(av, bv, acc[i], 0, 0, 0);
      }
    }
  };

  __syncthreads();  // the zeroed rows before any staged byte
  stage(0, 0);
  __syncthreads();
  for (int ks = 0; ks < a.KS; ++ks) {
    if (ks + 1 < a.KS) stage(ks + 1, (ks + 1) & 1);
    produce(ks, ks & 1);
    if (ks > 0) consume(ks - 1, (ks - 1) & 1);
    __syncthreads();
  }
  consume(a.KS - 1, (a.KS - 1) & 1);

  // ---------------------------------------------------------------- epilogue
  // D layout: column (pixel) = lane & 31, row (output channel) = 8 (r >> 2) + 4 (lane >> 5) + (r & 3)
  // (requant_hi2 / requant_lo2 and, below, requant4's arithmetic on one value, written out: through the shared functions
  // this unit's ISA moves)
  const float hi2 = a.act == ACT_RELU6 ? fminf(a.alpha + a.alpha, 254.f) : 254.f;
  const float lo2 = (a.act == ACT_RELU || a.act == ACT_RELU6) ? 0.f : -254.f;
#pragma unroll
  for (int i = 0; i < NACC; ++i) {
    if (wave + 4 * i >= P || pm[i] >= a.mt32) continue;  // wave-uniform
    const int q = pn[i] * 32 + col;
    const int o = (int)fastdiv_u31((uint32_t)q, a.cw_m, a.cw_s), xx = q - o * a.CW;
    if (o >= TRv || xx >= CWv) continue;
    const int pp = (oy0 + o) * a.ow + cx0 + xx;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int m = pm[i] * 32 + 8 * (r >> 2) + 4 * kh + (r & 3);
      if (m >= a.M) continue;
      const size_t off = ((size_t)b * a.M + m) * HW + pp;
      const int v = acc[i][r];
      if (OUT == OUT_I32) {
        reinterpret_cast<int*>(a.y)[off] = v;
      } else if (OUT == OUT_I8) {
        const float s = a.scale[m], bb = a.bias ? a.bias[m] : 0.f;
        float y2 = __fmaf_rn((float)v, s + s, bb + bb);
        if (a.act == ACT_LEAKY) y2 = y2 > 0.f ? y2 : a.alpha * y2;
        const int t = (int)__builtin_amdgcn_fmed3f(y2, lo2, hi2);
        reinterpret_cast<int8_t*>(a.y)[off] = (int8_t)((t + 1 + (t >> 31)) >> 1);
      } else {
        const float s = a.scale[m], bb = a.bias ? a.bias[m] : 0.f;
        float f = __fmaf_rn((float)v, s, bb);
        if (a.act == ACT_RELU) f = fmaxf(f, 0.f);
        if (a.act == ACT_RELU6) f = fminf(fmaxf(f, 0.f), a.alpha);
        if (a.act == ACT_LEAKY) f = f > 0.f ? f : a.alpha * f;
        if (a.res) {
          f = f + a.res[off];
          if (a.res_relu) f = f > 0.f ? f : 0.f;
        }
        if (a.y) reinterpret_cast<float*>(a.y)[off] = f;
        if (a.y2) a.y2[off] = (int8_t)round_sat_i8(a.inv_scale2 * f);
      }
    }
  }
}

// executes a plan of dw_conv1x1_launch_plan (dw_plan.h)
void launch_dw_conv1x1(const DwConvArgs& a_in, const DwPlan& p, int out, hipStream_t s) {
  DwConvArgs a = a_in;
  const DwPlan::G& g = p.g;
  a.KS = g.KS; a.mt32 = g.mt32; a.mtpb = g.mtpb; a.mgroups = g.mgroups;
  a.TR = g.TR; a.CW = g.CW; a.NT = g.NT; a.tr_tiles = g.tr_tiles; a.cw_tiles = g.cw_tiles; a.tpi = g.tpi;
  a.IR = g.IR; a.WP = g.WP; a.dword_stage = p.DWORD; a.wu = g.wu; a.rpp = g.rpp; a.nacc = p.NACC;
  a.ir_m = g.ir_m; a.ir_s = g.ir_s; a.owq_m = g.owq_m; a.owq_s = g.owq_s; a.tr_m = g.tr_m; a.tr_s = g.tr_s;
  a.cw_m = g.cw_m; a.cw_s = g.cw_s; a.tpi_m = g.tpi_m; a.tpi_s = g.tpi_s; a.ctl_m = g.ctl_m; a.ctl_s = g.ctl_s;
  a.lds = p.lds;
  const dim3 grid(p.grid_x, p.grid_y), block(p.block);
  with_const<1, 2, 4, 8>(p.NACC, [&](auto nacc) {
    with_const<OUT_I32, OUT_I8, OUT_F32>(out, [&](auto out_c) {
      with_const<1, 2>(p.S, [&](auto st) {
        with_const<0, 1>(p.PL, [&](auto pl) {
          hipLaunchKernelGGL((dw_conv1x1_fused_kernel<decltype(nacc)::value, decltype(out_c)::value, decltype(st)::value, decltype(pl)::value>),
                             grid, block, p.lds, s, a);
        });
      });
    });
  });
}

}  // namespace plhip
