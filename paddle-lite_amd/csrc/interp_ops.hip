// interp_ops.hip — dense prediction for gfx950: bilinear_interp / nearest_interp of fp32 NCHW planes (fp32 and / or the calib
// copy), arg_max along an axis, and interp -> arg_max(axis 1) in one launch that never writes the resampled tensor.
//
// Replaces (reference, ARM):
//   bilinear_interp  lite/backends/arm/math/interpolate.cc:65-463; the clamp of the source index and align_mode 1 (which the ARM
//                    kernel does not implement) by the scalar rule of lite/tests/kernels/interp_compute_test.cc:75-180
//   nearest_interp   interpolate.cc:465-499
//   arg_max          lite/backends/arm/math/argmax.cc:29-61: (value, index) pairs sorted with std::greater, so among equal
//                    maxima the LARGEST index wins
// Per axis with `in`, `out`, output index l and ratio r (an fp32 division done once on the host, interp_args):
//   bilinear  f = float(l) * r (align_corners, or align_mode 1) | max(r * (float(l) + 0.5f) - 0.5f, 0) (align_mode 0);
//             i0 = min((int)f, in - 1), i1 = min(i0 + 1, in - 1), w1 = f - float(i0), w0 = 1.f - w1
//             y = (x[y0][x0] * a0 + x[y0][x1] * a1) * b0 + (x[y1][x0] * a0 + x[y1][x1] * a1) * b1
//   nearest   i = min((int)(double(r * float(l)) + 0.5), in - 1) (align_corners) | min((int)(r * float(l)), in - 1)
// Every product and every sum is rounded on its own, as the ARM kernel's two unfused passes do: this file is compiled with
// floating-point contraction OFF (the pragma below), so no v_fma / v_fmac is made of them.  The int8 copy and the labels depend
// on the last bit of these values.
// These are write-bound streams (the source is up to 64 times smaller than the output): a lane owns W = 4 consecutive outputs
// of a row where the host finds every row aligned (16-byte fp32, 4-byte int8, 16-byte label stores), W = 1 otherwise; the x
// taps are computed once per lane and reused over the rows (interp) or the channels (interp -> arg_max) the lane walks.
#include "plhip_device.h"
#include "plhip_kernels.h"

#pragma clang fp contract(off)

namespace plhip {

namespace {

typedef long v2l __attribute__((ext_vector_type(2)));

// one axis of one output index: the two source indices and their weights (nearest: i1 == i0, w0 == 1)
struct Tap {
  int i0, i1;
  float w0, w1;
};

__host__ __device__ __forceinline__ Tap tap(int l, int n_in, float r, int bilinear, int half, int round_up) {
  Tap t;
  if (bilinear) {
    float f;
    if (half) {
      f = r * ((float)l + 0.5f) - 0.5f;  // l + 0.5 is exact; the product and the difference round separately
      f = f < 0.f ? 0.f : f;
    } else {
      f = (float)l * r;
    }
    const int i = (int)f;
    t.i0 = i < n_in - 1 ? i : n_in - 1;
    t.i1 = t.i0 + 1 < n_in - 1 ? t.i0 + 1 : n_in - 1;
    t.w1 = f - (float)t.i0;
    t.w0 = 1.f - t.w1;
  } else {
    const float f = r * (float)l;
    // align_corners: the reference adds the double constant 0.5, so the sum is a DOUBLE addition (exact here: f has 24
    // significant bits); an fp32 addition would round up just below k + 0.5.  Done in double, as the reference does.
    const int i = round_up ? (int)((double)f + 0.5) : (int)f;
    t.i0 = t.i1 = i < n_in - 1 ? i : n_in - 1;
    t.w0 = 1.f;
    t.w1 = 0.f;
  }
  return t;
}

// THE interpolated value: plhip_interp_f32 writes it and plhip_interp_argmax_f32 compares it.  p: a plane (or a window of one)
// with rows of `stride` floats; the taps are relative to p.
__device__ __forceinline__ float interp_value(const float* p, int stride, const Tap& ty, const Tap& tx, int bilinear) {
  const float* r0p = p + ty.i0 * stride;
  if (!bilinear) return r0p[tx.i0];
  const float* r1p = p + ty.i1 * stride;
  const float r0 = r0p[tx.i0] * tx.w0 + r0p[tx.i1] * tx.w1;
  const float r1 = r1p[tx.i0] * tx.w0 + r1p[tx.i1] * tx.w1;
  return r0 * ty.w0 + r1 * ty.w1;
}

// THE comparison of arg_max: channels are walked upwards and `>=` lets the larger index win a tie.  A NaN is never >= anything
// and nothing is >= a NaN: a NaN in channel 0 stays, any other is skipped; the index is always a channel that was seen.
__device__ __forceinline__ void keep_max(float v, int ch, float& best, int& idx) {
  if (v >= best) {
    best = v;
    idx = ch;
  }
}

template <typename T>
__device__ __forceinline__ void store_labels4(T* y, int i0, int i1, int i2, int i3) {
  if constexpr (sizeof(T) == 8) {
    v2l lo, hi;
    lo[0] = i0; lo[1] = i1; hi[0] = i2; hi[1] = i3;
    reinterpret_cast<v2l*>(y)[0] = lo;
    reinterpret_cast<v2l*>(y)[1] = hi;
  } else {
    v4i v;
    v[0] = i0; v[1] = i1; v[2] = i2; v[3] = i3;
    *reinterpret_cast<v4i*>(y) = v;
  }
}

bool al16(const void* p) { return ((uintptr_t)p & 15) == 0; }

constexpr int ROWS = 4;     // output rows a lane of interp_kernel walks with one set of x taps
constexpr int TILE = 32;    // interp_argmax_kernel: a block's output tile is TILE x TILE, 8 lanes x 4 outputs across
constexpr int LDS_MAX = 65536;

}  // namespace

// grid: x = items of W outputs of a row (1 << lg per block), y = rows ((256 >> lg) * ROWS per block), z = planes (loop).
// The host covers every item and every row with gridDim.x / y (both at most 2^15); lanes past the edge leave.
template <int W>
__global__ __launch_bounds__(256) void interp_kernel(InterpArgs a, float* __restrict__ yf, int8_t* __restrict__ yq, float inv,
                                                     int64_t planes, int lg) {
  const int l0 = (int)((blockIdx.x << lg) + (threadIdx.x & ((1 << lg) - 1))) * W;
  const int row0 = (int)(blockIdx.y * (256 >> lg) + (threadIdx.x >> lg)) * ROWS;
  if (l0 >= a.ow || row0 >= a.oh) return;  // W == 4 only where it divides ow: l0 + 3 < ow
  Tap tx[W];
#pragma unroll
  for (int j = 0; j < W; ++j) tx[j] = tap(l0 + j, a.iw, a.rx, a.bilinear, a.half, a.round_up);
  const int64_t in_plane = (int64_t)a.ih * a.iw, out_plane = (int64_t)a.oh * a.ow;
  for (int64_t p = blockIdx.z; p < planes; p += gridDim.z) {
    const float* __restrict__ src = a.x + p * in_plane;
#pragma unroll
    for (int k = 0; k < ROWS; ++k) {
      const int row = row0 + k;
      if (row >= a.oh) break;
      const Tap ty = tap(row, a.ih, a.ry, a.bilinear, a.half, a.round_up);
      const int64_t o = p * out_plane + (int64_t)row * a.ow + l0;
      if constexpr (W == 4) {
        v4f v;
#pragma unroll
        for (int j = 0; j < 4; ++j) v[j] = interp_value(src, a.iw, ty, tx[j], a.bilinear);
        if (yf) *reinterpret_cast<v4f*>(yf + o) = v;
        if (yq) *reinterpret_cast<uint32_t*>(yq + o) = calib4_i8(v, inv);
      } else {
        const float v = interp_value(src, a.iw, ty, tx[0], a.bilinear);
        if (yf) yf[o] = v;
        if (yq) yq[o] = (int8_t)round_sat_i8(inv * v);
      }
    }
  }
}

// grid: x = slices of 256 items of W inner positions (loop), y = outer (loop)
template <int W, typename T>
__global__ __launch_bounds__(256) void arg_max_kernel(const float* __restrict__ x, T* __restrict__ y, int64_t outer, int c, int64_t inner) {
  const int64_t items = inner / W;  // the host takes W == 4 only where it divides inner
  const int64_t step = (int64_t)gridDim.x * 256;
  for (int64_t o = blockIdx.y; o < outer; o += gridDim.y) {
    const float* __restrict__ src = x + o * c * inner;
    T* __restrict__ dst = y + o * inner;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < items; i += step) {
      if constexpr (W == 4) {
        const v4f first = *reinterpret_cast<const v4f*>(src + 4 * i);
        float best[4] = {first[0], first[1], first[2], first[3]};
        int idx[4] = {0, 0, 0, 0};
        for (int ch = 1; ch < c; ++ch) {
          const v4f v = *reinterpret_cast<const v4f*>(src + ch * inner + 4 * i);
#pragma unroll
          for (int j = 0; j < 4; ++j) keep_max(v[j], ch, best[j], idx[j]);
        }
        store_labels4(dst + 4 * i, idx[0], idx[1], idx[2], idx[3]);
      } else {
        float best = src[i];
        int idx = 0;
        for (int ch = 1; ch < c; ++ch) keep_max(src[ch * inner + i], ch, best, idx);
        dst[i] = (T)idx;
      }
    }
  }
}

// The channel walk of one lane of interp_argmax_kernel: p the first channel's plane (or the staged window of it), `plane` floats
// to the next channel's.  Called once with the LDS tile and once with global memory, so that each call has loads of one kind.
__device__ __forceinline__ void walk_channels(const float* p, int plane, int stride, const Tap& ty, const Tap (&tx)[4], int bilinear,
                                              int c, int (&idx)[4]) {
  float best[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    best[j] = interp_value(p, stride, ty, tx[j], bilinear);
    idx[j] = 0;
  }
  for (int ch = 1; ch < c; ++ch) {
    p += plane;
#pragma unroll
    for (int j = 0; j < 4; ++j) keep_max(interp_value(p, stride, ty, tx[j], bilinear), ch, best[j], idx[j]);
  }
}

// grid: x / y = TILE x TILE output tiles (the host covers all of them), z = image (loop).  A block finds the source window of its
// tile from the taps of the tile's first and last row and column (the taps are monotone in l: every step of tap() is a monotone
// rounded operation), stages the window of ALL c channels in LDS where c * window <= lds_floats (what the host sized the launch's
// dynamic LDS for), and reads global memory otherwise; then lane (tx, ty) walks the channels for outputs (row ty, cols 4 tx ..).
// vec: ow % 4 == 0 and y 16-byte aligned: the four labels go out in 16-byte stores.
template <typename T>
__global__ __launch_bounds__(256) void interp_argmax_kernel(InterpArgs a, T* __restrict__ y, int n, int c, int lds_floats, int vec) {
  extern __shared__ float tile[];
  const int col0 = blockIdx.x * TILE, row0 = blockIdx.y * TILE;
  const int col_last = col0 + TILE - 1 < a.ow - 1 ? col0 + TILE - 1 : a.ow - 1;
  const int row_last = row0 + TILE - 1 < a.oh - 1 ? row0 + TILE - 1 : a.oh - 1;
  const int sx0 = tap(col0, a.iw, a.rx, a.bilinear, a.half, a.round_up).i0;
  const int sy0 = tap(row0, a.ih, a.ry, a.bilinear, a.half, a.round_up).i0;
  const int tw = tap(col_last, a.iw, a.rx, a.bilinear, a.half, a.round_up).i1 - sx0 + 1;
  const int th = tap(row_last, a.ih, a.ry, a.bilinear, a.half, a.round_up).i1 - sy0 + 1;
  const int win = th * tw;
  const bool staged = (int64_t)c * win <= (int64_t)lds_floats;

  const int row = row0 + (threadIdx.x >> 3), l0 = col0 + 4 * (threadIdx.x & 7);
  const bool mine = row < a.oh && l0 < a.ow;
  // taps of the lane's outputs; a column past the edge takes the last column's (inside the window, never stored)
  Tap ty = tap(row < a.oh ? row : a.oh - 1, a.ih, a.ry, a.bilinear, a.half, a.round_up);
  Tap tx[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) tx[j] = tap(l0 + j < a.ow ? l0 + j : a.ow - 1, a.iw, a.rx, a.bilinear, a.half, a.round_up);
  const int in_plane = a.ih * a.iw;  // at most 2^30
  if (staged) {  // the taps relative to the window
    ty.i0 -= sy0; ty.i1 -= sy0;
#pragma unroll
    for (int j = 0; j < 4; ++j) tx[j].i0 -= sx0, tx[j].i1 -= sx0;
  }
  for (int img = blockIdx.z; img < n; img += gridDim.z) {
    const float* __restrict__ src = a.x + (int64_t)img * c * in_plane;
    int idx[4] = {0, 0, 0, 0};
    if (staged) {
      __syncthreads();  // the previous image's walk is over
      for (int e = threadIdx.x; e < c * win; e += 256) {
        const int ch = e / win, r = e - ch * win;
        const int yy = r / tw, xx = r - yy * tw;
        tile[e] = src[(int64_t)ch * in_plane + (int64_t)(sy0 + yy) * a.iw + (sx0 + xx)];
      }
      __syncthreads();
      if (mine) walk_channels(tile, win, tw, ty, tx, a.bilinear, c, idx);
    } else if (mine) {
      walk_channels(src, in_plane, a.iw, ty, tx, a.bilinear, c, idx);
    }
    if (mine) {
      T* dst = y + ((int64_t)img * a.oh + row) * a.ow + l0;
      if (vec) {
        store_labels4(dst, idx[0], idx[1], idx[2], idx[3]);
      } else {
#pragma unroll
        for (int j = 0; j < 4; ++j)
          if (l0 + j < a.ow) dst[j] = (T)idx[j];
      }
    }
  }
}

InterpArgs interp_args(const float* x, int ih, int iw, int oh, int ow, int method, int align_corners, int align_mode) {
  InterpArgs a;
  a.x = x;
  a.ih = ih; a.iw = iw; a.oh = oh; a.ow = ow;
  if (ih == oh && iw == ow) {  // a copy of the bits: one source pixel at ratio 1, (int)(1.f * l) == l
    a.ry = a.rx = 1.f;
    a.bilinear = a.half = a.round_up = 0;
    return a;
  }
  a.ry = align_corners ? (oh > 1 ? (float)(ih - 1) / (float)(oh - 1) : 0.f) : (float)ih / (float)oh;
  a.rx = align_corners ? (ow > 1 ? (float)(iw - 1) / (float)(ow - 1) : 0.f) : (float)iw / (float)ow;
  a.bilinear = method == 0;
  a.half = a.bilinear && !align_corners && align_mode == 0;
  a.round_up = !a.bilinear && align_corners;
  return a;
}

void launch_interp(const InterpArgs& a, int64_t planes, float* yf, int8_t* yq, float calib_scale, hipStream_t s) {
  const float inv = yq ? 1.f / calib_scale : 0.f;  // type_trans.cc:45, as launch_calib_f32_to_i8
  // every row of every plane starts at a multiple of ow elements: with ow % 4 == 0 all of them are as aligned as the bases
  const bool vec = (a.ow & 3) == 0 && al16(yf) && ((uintptr_t)yq & 3) == 0;
  const int items = vec ? a.ow >> 2 : a.ow;
  int lg = 2;  // lanes across a row: the power of two from 4 to 64 that covers the items
  while (lg < 6 && (1 << lg) < items) ++lg;
  const int rows_per_block = (256 >> lg) * ROWS;
  const dim3 grid((unsigned)((items + (1 << lg) - 1) >> lg), (unsigned)((a.oh + rows_per_block - 1) / rows_per_block),
                  (unsigned)(planes < 65535 ? planes : 65535));
  if (vec) hipLaunchKernelGGL(interp_kernel<4>, grid, dim3(256), 0, s, a, yf, yq, inv, planes, lg);
  else hipLaunchKernelGGL(interp_kernel<1>, grid, dim3(256), 0, s, a, yf, yq, inv, planes, lg);
}

void launch_arg_max(const float* x, int64_t outer, int c, int64_t inner, void* y, int i64, hipStream_t s) {
  const bool vec = (inner & 3) == 0 && al16(x) && al16(y);
  const int64_t items = vec ? inner >> 2 : inner;
  const int64_t slices = (items + 255) / 256;
  const dim3 grid((unsigned)(slices < (1 << 20) ? slices : (1 << 20)), (unsigned)(outer < 65535 ? outer : 65535));
  if (vec && i64) hipLaunchKernelGGL((arg_max_kernel<4, int64_t>), grid, dim3(256), 0, s, x, (int64_t*)y, outer, c, inner);
  else if (vec) hipLaunchKernelGGL((arg_max_kernel<4, int32_t>), grid, dim3(256), 0, s, x, (int32_t*)y, outer, c, inner);
  else if (i64) hipLaunchKernelGGL((arg_max_kernel<1, int64_t>), grid, dim3(256), 0, s, x, (int64_t*)y, outer, c, inner);
  else hipLaunchKernelGGL((arg_max_kernel<1, int32_t>), grid, dim3(256), 0, s, x, (int32_t*)y, outer, c, inner);
}

// the largest source extent a TILE of outputs reads along one axis, by the kernel's own rule
static int window_bound(int n_in, int n_out, float r, const InterpArgs& a) {
  int most = 1;
  for (int first = 0; first < n_out; first += TILE) {
    const int last = first + TILE - 1 < n_out - 1 ? first + TILE - 1 : n_out - 1;
    const int ext = tap(last, n_in, r, a.bilinear, a.half, a.round_up).i1 - tap(first, n_in, r, a.bilinear, a.half, a.round_up).i0 + 1;
    most = ext > most ? ext : most;
  }
  return most;
}

void launch_interp_argmax(const InterpArgs& a, int n, int c, void* y, int i64, hipStream_t s) {
  // the dynamic LDS holds the largest window of all c channels, where that fits; the kernel compares each block's own window
  // with lds_floats before it stages, so a window this bound missed reads global memory and never writes past the tile
  const int64_t need = (int64_t)c * window_bound(a.ih, a.oh, a.ry, a) * window_bound(a.iw, a.ow, a.rx, a);
  const int lds_floats = need * 4 <= LDS_MAX ? (int)need : 0;
  const int vec = (a.ow & 3) == 0 && al16(y);
  const dim3 grid((unsigned)((a.ow + TILE - 1) / TILE), (unsigned)((a.oh + TILE - 1) / TILE), (unsigned)(n < 65535 ? n : 65535));
  if (i64) hipLaunchKernelGGL(interp_argmax_kernel<int64_t>, grid, dim3(256), (size_t)lds_floats * 4, s, a, (int64_t*)y, n, c, lds_floats, vec);
  else hipLaunchKernelGGL(interp_argmax_kernel<int32_t>, grid, dim3(256), (size_t)lds_floats * 4, s, a, (int32_t*)y, n, c, lds_floats, vec);
}

}  // namespace plhip
