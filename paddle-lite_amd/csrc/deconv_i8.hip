// deconv_i8.hip — int8 conv2d_transpose: the MFMA phase kernel and the direct kernel.
//
// Semantics (lite/tests/utils/naive_math_impl.h:538-635 deconv_basic; shapes lite/operators/conv_transpose_op.cc:45-95): filter
// [cin][cout / groups][kh][kw], acc[n, g Mg + m, iy sh - pt + r dh, ix sw - pl + s dw] += x[n, g Cg + c, iy, ix] * w[g Cg + c, m, r, s];
// outputs no tap reaches are 0 before the epilogue, which is conv's.
//
// Phase route (deconv_plan.h states the envelope and the tile).  In padded output coordinates v = oy + pt, u = ox + pl, output
// (S V + py, S U + px) reads taps (py + S ty, px + S tx) at input (V - ty, U - tx): a stride-1 conv of the input per phase, on
// the quotient grid (V, U) all phases share.  No zero-inserted tensor, no col buffer, no workspace, no atomics.
// block (256 threads) = (image, 32-output-channel M tile, band of TR quotient rows, segment of CWq lane units).  A lane unit is
// 4 / S consecutive U of one V; its S * S phases are S output rows of 4 CONSECUTIVE columns: accumulator (py, j * S + px) of unit
// q is output column 4 q + j * S + px - pl, so the x phases are interleaved in registers and each row goes to gemm_epilogue_act as
// one quad (contiguous 16-byte / 4-byte stores at any alignment; the quad across the left edge passes `skip`).
// The block stages the band's input rows plus halo as conv_grouped_i8.hip does (transposed: 16 channels of a pixel are 16
// consecutive LDS bytes, zero borders written by the staging), pixels stored by residue of the column mod 4 / S so that the 32
// lanes of a k half read consecutive 16-byte slots.  It loops over the Cin / 32 chunks and re-stages per chunk between two
// barriers (one LDS tile: the loads of chunk k + 1 do not overlap the MFMAs of chunk k inside a block; other blocks of the CU
// do); per chunk and phase it runs taps(phase) K-steps of v_mfma_i32_32x32x32_i8, the tap's A fragment read from the packed
// weights ([M tile][chunk][tap][64 lanes][16 B], 1 KiB each, rows >= Cout zero) where it is used (copying a chunk's fragments
// into LDS beside the input rows was measured no faster over the four shapes of DESIGN.md 15, at about 25 more VGPRs).
//
// Direct route: everything else, one lane per output in gather form over its valid taps and its group's input channels, the
// scalar epilogue functions of plhip_device.h.  It is the slow path.
#include "gemm_epilogue.h"
#include "plhip_kernels.h"

namespace plhip {

namespace {

template <int S>
__device__ __forceinline__ void deconv_stage(const DeconvArgs& a, uint8_t* tile, int b, int chunk, int iy0, int ic0) {
  // unit = (staged row, 4 consecutive staged columns, 4 channels): 4 (unaligned) dword loads, a 4x4 byte transpose, 4 LDS dwords
  // (grouped_stage's unit; the staged column p of a row is input column ic0 + p).  The load is a copy of grouped_stage's on
  // purpose: shared through a header it compiled conv_grouped3x3_kernel to different code (another register allocation), which
  // nothing in this change measures
  constexpr int JU = 4 / S, LG = S == 1 ? 2 : 1;
  constexpr int U = 4;  // units of a thread whose loads are issued before the first of them is transposed and stored
  const int WS = JU * a.WQ, wq4 = WS >> 2;
  const int units = a.IR * wq4 * 8;
  const size_t cstride = (size_t)a.h * a.w;
  const int8_t* xc = a.x + ((size_t)b * a.cin + chunk * 32) * cstride;
  auto load = [&](int u, uint32_t (&r)[4]) __attribute__((always_inline)) {
    const int cg = u & 7, rt = u >> 3;
    const int rowl = rt / wq4, t = rt - rowl * wq4;
    const int iy = iy0 + rowl;
    const int icol = ic0 + 4 * t;  // input column of the unit's first pixel
    r[0] = r[1] = r[2] = r[3] = 0u;
    if (iy < 0 || iy >= a.h || icol + 3 < 0 || icol >= a.w) return;
    const int8_t* p = xc + (size_t)(4 * cg) * cstride + (size_t)iy * a.w;
    if (a.w >= 4) {
      // a unit across the plane's left / right edge: the row's first / last dword, shifted so that the columns outside are zero
      const int lo = icol < 0 ? 0 : (icol + 4 > a.w ? a.w - 4 : icol);
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        uint32_t v;
        __builtin_memcpy(&v, p + k * cstride + lo, 4);
        r[k] = icol < lo ? v << (8 * (lo - icol)) : v >> (8 * (icol - lo));
      }
    } else {
#pragma unroll
      for (int k = 0; k < 4; ++k)
#pragma unroll
        for (int i = 0; i < 4; ++i)
          if (icol + i >= 0 && icol + i < a.w) r[k] |= (uint32_t)(uint8_t)p[k * cstride + icol + i] << (8 * i);
    }
  };
  auto store = [&](int u, const uint32_t (&r)[4]) __attribute__((always_inline)) {
    const int cg = u & 7, rt = u >> 3;
    const int rowl = rt / wq4, t = rt - rowl * wq4;
    uint32_t o[4];
    transpose4x4_b8(r[0], r[1], r[2], r[3], o[0], o[1], o[2], o[3]);  // o[i] = pixel i, channels 4 cg .. 4 cg + 3
    uint8_t* row = tile + (size_t)(cg >> 2) * a.half + (size_t)rowl * WS * 16 + 4 * (cg & 3);
#pragma unroll
    for (int i = 0; i < 4; ++i) {  // staged column 4 t + i: residue (4 t + i) % JU, quotient (4 t + i) / JU
      const int res = i & (JU - 1), quo = ((4 * t) >> LG) + (i >> LG);
      *reinterpret_cast<uint32_t*>(row + (res * a.WQ + quo) * 16) = o[i];
    }
  };
  for (int u0 = (int)threadIdx.x; u0 < units; u0 += 256 * U) {
    uint32_t r[U][4];
#pragma unroll
    for (int k = 0; k < U; ++k)
      if (u0 + 256 * k < units) load(u0 + 256 * k, r[k]);
#pragma unroll
    for (int k = 0; k < U; ++k)
      if (u0 + 256 * k < units) store(u0 + 256 * k, r[k]);
  }
}

template <int S, int OUT>
__global__ __launch_bounds__(256) void deconv_phase_kernel(const DeconvArgs a) {
  extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
  constexpr int JU = 4 / S, LG = S == 1 ? 2 : 1;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int c = lane & 31, h = lane >> 5;
  float* lsb = reinterpret_cast<float*>(smem) + wave * 64;
  uint8_t* tile = smem + 1024;

  // XCD x (= blockIdx % 8, round-robin dispatch) gets the x-th eighth of the (image, M tile, band, segment) space, so that bands
  // sharing halo rows sit on one L2; blocks of the grid's round-up have nothing to do (block-uniform exit before any barrier)
  const unsigned per = a.nblocks_per_xcd;
  const unsigned vb = (blockIdx.x & 7) * per + (blockIdx.x >> 3);
  if (vb >= a.nblocks) return;
  const int seg = (int)(vb % (unsigned)a.nseg);
  unsigned tt = vb / (unsigned)a.nseg;
  const int band = (int)(tt % (unsigned)a.bands);
  tt /= (unsigned)a.bands;
  const int mt = (int)(tt % (unsigned)a.MT);
  const int b = (int)(tt / (unsigned)a.MT);

  GemmArgs g;
  g.y = a.y;
  g.scale = a.scale;
  g.bias = a.bias;
  g.M = a.cout;
  g.HWY = a.oh * a.ow;
  g.y_bstride = (size_t)a.cout * a.oh * a.ow;
  g.act = a.act;
  g.alpha = a.alpha;
  g.res = nullptr;
  g.res_relu = 0;
  g.y2 = nullptr;
  g.inv_scale2 = 0.f;
  if (OUT != OUT_I32) stage_scale_bias<1, OUT>(g, mt, lane, lsb);

  // the lane's unit: quotient row V, units 4 / S columns wide; lanes past the tile or the plane duplicate the tile's first unit
  const int WS = JU * a.WQ;
  const int V0 = band * a.TR;
  const int qi = wave * 32 + c;
  int ry = qi / a.CWq, xql = qi - ry * a.CWq;
  const int V = V0 + ry, unit = seg * a.CWq + xql;
  const bool qvalid = ry < a.TR && V < a.NV && unit < a.NUq;
  if (!qvalid) ry = 0, xql = 0;
  const uint8_t* lb = tile + (size_t)h * a.half + ((size_t)ry * WS + xql) * 16;

  v16i acc[S][1][4];
#pragma unroll
  for (int py = 0; py < S; ++py)
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[py][0][j][r] = 0;

  const int kk = a.kh * a.kw;
  for (int chunk = 0; chunk < a.NCH; ++chunk) {
    if (chunk) __syncthreads();  // every wave is done with the previous chunk's tile
    deconv_stage<S>(a, tile, b, chunk, V0 - (a.TY - 1), seg * a.CWq * JU - (a.TX - 1));
    __syncthreads();
    const int8_t* wf = a.wp + ((size_t)(mt * a.NCH + chunk) * kk * 64 + lane) * 16;
#pragma unroll
    for (int py = 0; py < S; ++py) {
      for (int r = py, ty = 0; r < a.kh; r += S, ++ty) {  // tap row r reads input row V - ty: staged row ry + TY - 1 - ty
        const uint8_t* lr = lb + (size_t)(a.TY - 1 - ty) * WS * 16;
#pragma unroll
        for (int px = 0; px < S; ++px) {
          for (int s = px, tx = 0; s < a.kw; s += S, ++tx) {  // tap column s reads input column U - tx: staged column + TX - 1 - tx
            const v4i af = *reinterpret_cast<const v4i*>(wf + (size_t)(r * a.kw + s) * 1024);
            const int dx = a.TX - 1 - tx;
            v4i bf[JU];
#pragma unroll
            for (int j = 0; j < JU; ++j) {
              const int d = j + dx;
              bf[j] = *reinterpret_cast<const v4i*>(lr + ((d & (JU - 1)) * a.WQ + (d >> LG)) * 16);
            }
#pragma unroll
            for (int j = 0; j < JU; ++j)
              acc[py][0][j * S + px] = __builtin_amdgcn_mfma_i32_32x32x32_i8(af, bf[j], acc[py][0][j * S + px], 0, 0, 0);
          }
        }
      }
    }
  }

  if (!qvalid) return;
  const int ox0 = 4 * unit - a.pl;  // the quad's first output column; columns < 0 (left padding) and >= ow are not stored
  const int skip = ox0 < 0 ? -ox0 : 0, room = a.ow - ox0;
  if (skip >= 4 || room <= skip) return;
#pragma unroll
  for (int py = 0; py < S; ++py) {
    const int oy = V * S + py - a.pt;
    if (oy < 0 || oy >= a.oh) continue;
    gemm_epilogue_act<1, OUT, false, false>(g, acc[py], mt, h, b, oy * a.ow + ox0, lsb, room, skip);
  }
}

// A fragments [M tile][chunk][tap r * kw + s][64 lanes][16 B]: lane (m, h) byte j = w[32 chunk + 16 h + j][32 mt + m][r][s],
// 0 for output channels >= cout
__global__ void pack_deconv_phase_kernel(const int8_t* __restrict__ w, int8_t* __restrict__ wp, int cin, int cout, int kk, size_t total) {
  const int nch = cin / 32;
  for (size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (size_t)gridDim.x * blockDim.x) {
    const int j = idx & 15;
    const int lane = (idx >> 4) & 63;
    size_t ct = idx >> 10;
    const int t = (int)(ct % kk);
    ct /= kk;
    const int chunk = (int)(ct % nch);
    const int mt = (int)(ct / nch);
    const int m = mt * 32 + (lane & 31), k = chunk * 32 + 16 * (lane >> 5) + j;
    wp[idx] = m < cout ? w[((size_t)k * cout + m) * kk + t] : (int8_t)0;
  }
}

template <int OUT>
__global__ __launch_bounds__(256) void deconv_direct_kernel(const DeconvArgs a, size_t total) {
  const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= total) return;
  const int ox = (int)(idx % a.ow);
  size_t t = idx / a.ow;
  const int oy = (int)(t % a.oh);
  t /= a.oh;
  const int co = (int)(t % a.cout);
  const int b = (int)(t / a.cout);
  const int cg = a.cin / a.groups, mg = a.cout / a.groups;
  const int grp = co / mg, m = co - grp * mg;
  const size_t plane = (size_t)a.h * a.w, wstep = (size_t)mg * a.kh * a.kw;
  const int8_t* xg = a.x + ((size_t)b * a.cin + (size_t)grp * cg) * plane;
  const int8_t* wg = a.wp + ((size_t)grp * cg * mg + m) * a.kh * a.kw;
  int acc = 0;
  for (int r = 0; r < a.kh; ++r) {  // gather form: iy = (oy + pt - r dh) / sh where that divides and is in range
    const int ty = oy + a.pt - r * a.dh;
    if (ty < 0 || ty % a.sh) continue;
    const int iy = ty / a.sh;
    if (iy >= a.h) continue;
    for (int s = 0; s < a.kw; ++s) {
      const int tx = ox + a.pl - s * a.dw;
      if (tx < 0 || tx % a.sw) continue;
      const int ix = tx / a.sw;
      if (ix >= a.w) continue;
      const int8_t* xp = xg + (size_t)iy * a.w + ix;
      const int8_t* wq = wg + r * a.kw + s;
      for (int ci = 0; ci < cg; ++ci) acc += (int)xp[ci * plane] * (int)wq[ci * wstep];
    }
  }
  if (OUT == OUT_I32) {
    reinterpret_cast<int*>(a.y)[idx] = acc;
    return;
  }
  const float f = epilogue_f32(acc, a.scale[co], a.bias ? a.bias[co] : 0.f, a.act, a.alpha);
  if (OUT == OUT_F32) reinterpret_cast<float*>(a.y)[idx] = f;
  else reinterpret_cast<int8_t*>(a.y)[idx] = (int8_t)round_sat_i8(f);
}

}  // namespace

void launch_pack_deconv_phase(const int8_t* w_iohw, int8_t* wp, const DeconvProblem& p, hipStream_t s) {
  const size_t total = deconv_phase_packed_bytes(p);
  const int blocks = (int)((total + 255) / 256 < 1024 ? (total + 255) / 256 : 1024);
  hipLaunchKernelGGL(pack_deconv_phase_kernel, dim3(blocks), dim3(256), 0, s, w_iohw, wp, p.cin, p.cout, p.kh * p.kw, total);
}

void launch_deconv_phase(const DeconvArgs& a, int out, hipStream_t s) {
  const dim3 grid(a.nblocks_per_xcd * 8), block(256);
#define PLHIP_DECONV(S, O) hipLaunchKernelGGL((deconv_phase_kernel<S, O>), grid, block, a.lds, s, a)
  if (a.sh == 1) {
    if (out == OUT_I32) PLHIP_DECONV(1, OUT_I32);
    else if (out == OUT_F32) PLHIP_DECONV(1, OUT_F32);
    else PLHIP_DECONV(1, OUT_I8);
  } else {
    if (out == OUT_I32) PLHIP_DECONV(2, OUT_I32);
    else if (out == OUT_F32) PLHIP_DECONV(2, OUT_F32);
    else PLHIP_DECONV(2, OUT_I8);
  }
#undef PLHIP_DECONV
}

void launch_deconv_direct(const DeconvArgs& a, int out, hipStream_t s) {
  const size_t total = (size_t)a.n * a.cout * a.oh * a.ow;  // < 2^31 blocks of 256: checked by the caller
  const dim3 grid((unsigned)((total + 255) / 256)), block(256);
  if (out == OUT_I32) hipLaunchKernelGGL((deconv_direct_kernel<OUT_I32>), grid, block, 0, s, a, total);
  else if (out == OUT_F32) hipLaunchKernelGGL((deconv_direct_kernel<OUT_F32>), grid, block, 0, s, a, total);
  else hipLaunchKernelGGL((deconv_direct_kernel<OUT_I8>), grid, block, 0, s, a, total);
}

}  // namespace plhip
