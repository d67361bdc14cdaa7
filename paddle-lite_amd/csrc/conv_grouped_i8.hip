// conv_grouped_i8.hip — grouped 3x3 convolution (ResNeXt / RegNet: 1 < groups < cin) in ONE launch, stride 1 or 2.
//
// Envelope: Cg == Mg (cin / groups == cout / groups) in {4, 8, 16, 32} and cin % 32 == 0.  Then the 32 consecutive output
// channels of one MFMA M tile read exactly the 32 consecutive input channels with the same indices: a CHUNK of 32 / Cg whole
// groups, and the conv is cin / 32 independent dense 32 -> 32 3x3 convs whose weights are block-diagonal.  The packer writes 9 A
// fragments per chunk (one per tap, zero off the diagonal blocks); a wave keeps them in 36 VGPRs and runs 9 K-steps of
// v_mfma_i32_32x32x32_i8 (K-step = one tap over the chunk's 32 channels) per 128 outputs.  Only Cg / 32 of every MFMA is useful
// work; the layer stays bound by its bytes.
//
// block (256 threads) = (image, chunk, band of TR output rows, segment of CWq output column quads).  It stages the band's input
// rows itself, zero borders included (no padded copy, no workspace), TRANSPOSED: 16 channels of a pixel are 16 consecutive LDS
// bytes, so the B operand of (output, tap) is one 16-byte LDS read per lane (channels 16 h .. 16 h + 15 for k half h; the two
// halves of the chunk are two images `half` bytes apart).  The pixels of a staged row are stored by residue: padded column ip
// of the segment sits in slot (ip % Q) * WQ + ip / Q with Q = 4 * stride, so that the 32 lanes of a k half, which own
// consecutive output QUADS (the epilogue's column layout: MFMA tile j of lane c = output 4 c + j), read consecutive 16-byte
// slots for every (tap, j): no bank conflicts at either stride.
#include "gemm_epilogue.h"
#include "plhip_kernels.h"

namespace plhip {

namespace {

constexpr int GROUPED_LDS_TILE_MAX = 40 * 1024;  // staged pixel bytes per block: 3 blocks per CU

template <int STRIDE>
__device__ __forceinline__ void grouped_stage(const GroupedArgs& a, uint8_t* tile, int b, int chunk, int iy0, int ipb) {
  // unit = (staged row, 4 consecutive padded columns, 4 channels): 4 (unaligned) dword loads, a 4x4 byte transpose, 4 LDS dwords.
  // cg runs fastest across the lanes: channel groups 0..3 of a pixel are its 16 contiguous bytes of the first image, 4..7 of
  // the second (half % 128 == 64: the two land on different banks).
  constexpr int Q = 4 * STRIDE;
  constexpr int U = 4;  // units of a thread whose loads are issued before the first of them is transposed and stored
  const int WS = Q * a.WQ, wq4 = WS >> 2;
  const int units = a.IR * wq4 * 8;
  const size_t cstride = (size_t)a.h * a.w;
  const int8_t* xc = a.x + ((size_t)b * a.cin + chunk * 32) * cstride;
  auto load = [&](int u, uint32_t (&r)[4]) __attribute__((always_inline)) {
    const int cg = u & 7, rt = u >> 3;
    const int rowl = rt / wq4, t = rt - rowl * wq4;
    const int iy = iy0 + rowl;
    const int icol = ipb + 4 * t - a.pl;  // input column of the unit's first pixel
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
    // padded column 4 t + i of the segment: residue (4 t + i) % Q, quotient (4 t + i) / Q
    const int res0 = STRIDE == 1 ? 0 : 4 * (t & 1), quo = STRIDE == 1 ? t : t >> 1;
    uint8_t* row = tile + (size_t)(cg >> 2) * a.half + (size_t)rowl * WS * 16 + 4 * (cg & 3);
#pragma unroll
    for (int i = 0; i < 4; ++i) *reinterpret_cast<uint32_t*>(row + ((res0 + i) * a.WQ + quo) * 16) = o[i];
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

template <int STRIDE, int OUT>
__global__ __launch_bounds__(256) void conv_grouped3x3_kernel(const GroupedArgs a) {
  extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
  constexpr int Q = 4 * STRIDE;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int c = lane & 31, h = lane >> 5;
  float* lsb = reinterpret_cast<float*>(smem) + wave * 64;
  uint8_t* tile = smem + 1024;

  // XCD x (= blockIdx % 8, round-robin dispatch) gets the x-th eighth of the (image, chunk, band, segment) space, so that bands
  // sharing halo rows sit on one L2; blocks of the grid's round-up have nothing to do (block-uniform exit before any barrier)
  const unsigned per = a.nblocks_per_xcd;
  const unsigned vb = (blockIdx.x & 7) * per + (blockIdx.x >> 3);
  if (vb >= a.nblocks) return;
  const int seg = (int)(vb % (unsigned)a.nseg);
  unsigned tt = vb / (unsigned)a.nseg;
  const int band = (int)(tt % (unsigned)a.bands);
  tt /= (unsigned)a.bands;
  const int chunk = (int)(tt % (unsigned)a.NCH);
  const int b = (int)(tt / (unsigned)a.NCH);

  // the chunk's 9 A fragments: 36 VGPRs for the whole kernel, requested before the staging loop
  v4i af[9];
#pragma unroll
  for (int t = 0; t < 9; ++t) af[t] = *reinterpret_cast<const v4i*>(a.wp + (((size_t)chunk * 9 + t) * 64 + lane) * 16);

  GemmArgs g;
  g.y = a.y;
  g.scale = a.scale;
  g.bias = a.bias;
  g.M = a.cout;
  g.HWY = a.oh * a.ow;
  g.y_bstride = (size_t)a.cout * a.oh * a.ow;
  g.act = a.act;
  g.alpha = a.alpha;
  g.res = a.res;
  g.res_relu = a.res_relu;
  g.y2 = a.y2;
  g.inv_scale2 = a.inv_scale2;
  if (OUT != OUT_I32) stage_scale_bias<1, OUT>(g, chunk, lane, lsb);

  const int oy0 = band * a.TR;
  grouped_stage<STRIDE>(a, tile, b, chunk, oy0 * STRIDE - a.pt, seg * a.CWq * Q);
  __syncthreads();

  const int WS = Q * a.WQ;
  const int nq = a.TR * a.CWq;  // quads of the tile: (row, column quad), 32 per wave and pass
  for (int q0 = wave * 32; q0 < nq; q0 += 128) {  // wave-uniform
    const int qi = q0 + c;
    int ry = qi / a.CWq, xql = qi - ry * a.CWq;
    const int oy = oy0 + ry, xq = seg * a.CWq + xql;
    const bool qvalid = qi < nq && oy < a.oh && 4 * xq < a.ow;
    if (!qvalid) ry = 0, xql = 0;  // a duplicate of the tile's first quad: computed, not stored
    const uint8_t* lb = tile + (size_t)h * a.half + ((size_t)(ry * STRIDE) * WS + xql) * 16;

    v16i acc[1][4];
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[0][j][r] = 0;
#pragma unroll
    for (int r = 0; r < 3; ++r) {
#pragma unroll
      for (int s = 0; s < 3; ++s) {
        v4i bf[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {  // output 4 xq + j, tap (r, s): padded column Q xql + STRIDE j + s of the segment
          const int d = STRIDE * j + s;
          bf[j] = *reinterpret_cast<const v4i*>(lb + ((size_t)r * WS + (d % Q) * a.WQ + d / Q) * 16);
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[0][j] = __builtin_amdgcn_mfma_i32_32x32x32_i8(af[r * 3 + s], bf[j], acc[0][j], 0, 0, 0);
      }
    }
    if (qvalid) gemm_epilogue_act<1, OUT, false, true>(g, acc, chunk, h, b, oy * a.ow + 4 * xq, lsb, a.ow - 4 * xq);
  }
}

// A fragments [chunk][tap r * 3 + s][64 lanes][16 B]: lane (m, h) byte j = w[32 chunk + m][k % Cg][r][s] for input channel
// k = 16 h + j of the chunk when k and m are in the same group (k / Cg == m / Cg), else 0
__global__ void pack_grouped3x3_kernel(const int8_t* __restrict__ w, int8_t* __restrict__ wp, int cg, size_t total) {
  for (size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (size_t)gridDim.x * blockDim.x) {
    const int j = idx & 15;
    const int lane = (idx >> 4) & 63;
    const size_t ct = idx >> 10;
    const int t = (int)(ct % 9);
    const size_t chunk = ct / 9;
    const int m = lane & 31, k = 16 * (lane >> 5) + j;
    int8_t v = 0;
    if (m / cg == k / cg) v = w[((chunk * 32 + m) * cg + k % cg) * 9 + t];
    wp[idx] = v;
  }
}

}  // namespace

bool conv_grouped3x3_supported(int cin, int cout, int kh, int kw, int sh, int sw, int dh, int dw, int groups, const int pad[4]) {
  if (kh != 3 || kw != 3 || dh != 1 || dw != 1 || sh != sw || (sh != 1 && sh != 2) || groups < 4) return false;
  for (int i = 0; i < 4; ++i)
    if (pad[i] != 0 && pad[i] != 1) return false;
  if (cin != cout || cin % groups || cin % 32) return false;
  const int cg = cin / groups;
  return cg == 4 || cg == 8 || cg == 16 || cg == 32;
}

size_t conv_grouped3x3_packed_bytes(int cin) { return (size_t)(cin / 32) * 9 * 1024; }

void launch_pack_conv_grouped3x3(const int8_t* w_oihw, int8_t* wp, int cin, int groups, hipStream_t s) {
  const size_t total = conv_grouped3x3_packed_bytes(cin);
  const int blocks = (int)((total + 255) / 256 < 1024 ? (total + 255) / 256 : 1024);
  hipLaunchKernelGGL(pack_grouped3x3_kernel, dim3(blocks), dim3(256), 0, s, w_oihw, wp, cin / groups, total);
}

// tile plan: CWq column quads (<= 32, a wave's lanes), TR rows with TR * CWq <= 128 quads (one pass of the 4 waves) and the
// staged rows within GROUPED_LDS_TILE_MAX
bool conv_grouped3x3_plan(GroupedArgs* a) {
  const int Q = 4 * a->stride;
  const int owq = (a->ow + 3) / 4;
  a->NCH = a->cin / 32;
  a->CWq = owq < 32 ? owq : 32;
  a->nseg = (owq + a->CWq - 1) / a->CWq;
  a->WQ = a->CWq + 1;
  int tr = 128 / a->CWq;
  if (tr > a->oh) tr = a->oh;
  while (tr > 1 && (size_t)((tr - 1) * a->stride + 3) * Q * a->WQ * 32 > (size_t)GROUPED_LDS_TILE_MAX) --tr;
  a->TR = tr;
  a->IR = (tr - 1) * a->stride + 3;
  a->bands = (a->oh + tr - 1) / tr;
  a->half = a->IR * Q * a->WQ * 16;
  a->half += (64 - a->half % 128 + 128) % 128;  // half % 128 == 64
  a->lds = 1024 + 2 * (size_t)a->half;
  const size_t nb = (size_t)a->n * a->NCH * a->bands * a->nseg;
  if (nb > ((size_t)1 << 31) - 16) return false;
  a->nblocks = (unsigned)nb;
  a->nblocks_per_xcd = (unsigned)((nb + 7) / 8);
  return true;
}

void launch_conv_grouped3x3(const GroupedArgs& a, int out, hipStream_t s) {
  const dim3 grid(a.nblocks_per_xcd * 8), block(256);
#define PLHIP_GROUPED(S, O) hipLaunchKernelGGL((conv_grouped3x3_kernel<S, O>), grid, block, a.lds, s, a)
  if (a.stride == 1) {
    if (out == OUT_I32) PLHIP_GROUPED(1, OUT_I32);
    else if (out == OUT_F32) PLHIP_GROUPED(1, OUT_F32);
    else PLHIP_GROUPED(1, OUT_I8);
  } else {
    if (out == OUT_I32) PLHIP_GROUPED(2, OUT_I32);
    else if (out == OUT_F32) PLHIP_GROUPED(2, OUT_F32);
    else PLHIP_GROUPED(2, OUT_I8);
  }
#undef PLHIP_GROUPED
}

}  // namespace plhip
