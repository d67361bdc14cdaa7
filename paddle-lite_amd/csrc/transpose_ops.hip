// transpose_ops.hip — transpose of fp32 tensors of rank 2 to 4 for gfx950, and the join of an SSD head's feature maps
// (transpose(0,2,3,1) -> reshape([0,-1,k]) -> concat(axis 1)) in one launch.
//
// Replaces (reference, ARM): lite/kernels/arm/transpose_compute.cc (any permutation: output index (i0 .. ) reads input index
// perm-gathered) and, for the join, that kernel followed by reshape (no data) and ConcatCompute.
// Values are MOVED (dword copies: NaN payloads and -0.0 keep their bits).
// The host first drops axes of extent 1 and merges source axes that stay adjacent and in order; what is left has
//   * its innermost source axis innermost in the destination too: rows are copied whole, transpose_rows_kernel (one lane per
//     output element, consecutive lanes on consecutive floats of both sides), or
//   * the innermost source axis S somewhere else, and another source axis D innermost in the destination: a batch of 2-D
//     transposes, transpose_tile_kernel: a block moves a 64 x 64 tile through LDS (pitch 65 floats: the column walk of the
//     write phase touches 64 different banks), reading whole rows along S and writing whole rows along D.  With both extents
//     multiples of 4 and both bases on 16 bytes a lane reads and writes quads.  NCHW -> NHWC of an SSD head is this case with
//     D = C and S = H * W; (0, 2, 1) on [N, P, C] with D = P and S = C.
#include "plhip_device.h"
#include "plhip_kernels.h"

namespace plhip {

namespace {

constexpr int TILE = 64, PITCH = TILE + 1;

bool al16(const void* p) { return ((uintptr_t)p & 15) == 0; }

// One 64 x 64 tile of a 2-D transpose through `tile` ([TILE][PITCH] floats of LDS): dst[s][d] = src[d][s] for d0 <= d < d0 + 64,
// s0 <= s < s0 + 64 inside D x S.  src rows (fixed d) are sd floats apart, dst rows (fixed s) dd floats apart.  All 256 lanes
// of the block call it; it ends with a barrier, so the tile may be reused at once.
template <int VEC>
__device__ __forceinline__ void transpose_tile(const float* __restrict__ src, int64_t sd, float* __restrict__ dst, int64_t dd, int64_t D,
                                               int64_t S, int64_t d0, int64_t s0, float* tile) {
  const int nd = D - d0 < TILE ? (int)(D - d0) : TILE, ns = S - s0 < TILE ? (int)(S - s0) : TILE;
  if (VEC) {
    // 16 lanes x 4 floats per row, 16 rows per pass
    const int c = (threadIdx.x & 15) * 4;
    for (int r = threadIdx.x >> 4; r < nd; r += 16)
      if (c < ns) {
        const v4f v = *reinterpret_cast<const v4f*>(src + (d0 + r) * sd + s0 + c);
        float* t = tile + r * PITCH + c;
        t[0] = v[0]; t[1] = v[1]; t[2] = v[2]; t[3] = v[3];
      }
    __syncthreads();
    for (int r = threadIdx.x >> 4; r < ns; r += 16)
      if (c < nd) {
        v4f v;
        v[0] = tile[c * PITCH + r]; v[1] = tile[(c + 1) * PITCH + r]; v[2] = tile[(c + 2) * PITCH + r]; v[3] = tile[(c + 3) * PITCH + r];
        *reinterpret_cast<v4f*>(dst + (s0 + r) * dd + d0 + c) = v;
      }
  } else {
    const int c = threadIdx.x & 63;
    for (int r = threadIdx.x >> 6; r < nd; r += 4)
      if (c < ns) tile[r * PITCH + c] = src[(d0 + r) * sd + s0 + c];
    __syncthreads();
    for (int r = threadIdx.x >> 6; r < ns; r += 4)
      if (c < nd) dst[(s0 + r) * dd + d0 + c] = tile[c * PITCH + r];
  }
  __syncthreads();
}

}  // namespace

// rows copied whole: output axes (o0, o1, o2, o3), o3 innermost on both sides; axis k of the output has source stride ss[k]
__global__ __launch_bounds__(256) void transpose_rows_kernel(TransposeArgs a) {
  const int64_t step = (int64_t)gridDim.x * 256;
  for (int64_t o = (int64_t)blockIdx.x * 256 + threadIdx.x; o < a.total; o += step) {
    int64_t rest = o;
    const int64_t i3 = rest % a.od[3]; rest /= a.od[3];
    const int64_t i2 = rest % a.od[2]; rest /= a.od[2];
    const int64_t i1 = rest % a.od[1]; rest /= a.od[1];
    a.y[o] = a.x[rest * a.ss[0] + i1 * a.ss[1] + i2 * a.ss[2] + i3 * a.ss[3]];
  }
}

// batch of 2-D transposes: grid x = tiles of the D x S plane (loop), y = batch index (loop) = b0 * B1 + b1
template <int VEC>
__global__ __launch_bounds__(256) void transpose_tile_kernel(TransposeArgs a) {
  __shared__ float tile[TILE * PITCH];
  const int64_t tiles_s = (a.S + TILE - 1) / TILE, tiles = tiles_s * ((a.D + TILE - 1) / TILE);
  for (int64_t b = blockIdx.y; b < a.B0 * a.B1; b += gridDim.y) {
    const int64_t b0 = b / a.B1, b1 = b - b0 * a.B1;
    const float* src = a.x + b0 * a.bs[0] + b1 * a.bs[1];
    float* dst = a.y + b0 * a.bd[0] + b1 * a.bd[1];
    for (int64_t t = blockIdx.x; t < tiles; t += gridDim.x) {
      const int64_t td = t / tiles_s, ts = t - td * tiles_s;
      transpose_tile<VEC>(src, a.sd, dst, a.dd, a.D, a.S, td * TILE, ts * TILE, tile);
    }
  }
}

void launch_transpose(const float* x, const int64_t* dims, const int* perm, int rank, float* y, hipStream_t s) {
  // source strides, then the output's axes without those of extent 1
  int64_t sstride[4], od[4], ss[4];
  int src_axis[4];
  int64_t total = 1;
  for (int k = rank - 1; k >= 0; --k) {
    sstride[k] = total;
    total *= dims[k];
  }
  int order[4], seen = 0;  // order[axis]: the source axis's place among the source axes of extent > 1
  for (int k = 0; k < rank; ++k) order[k] = dims[k] == 1 ? -1 : seen++;
  int r = 0;
  for (int k = 0; k < rank; ++k) {
    if (dims[perm[k]] == 1) continue;
    // merged with the output axis in front of it when the two are neighbours, in this order, in the source as well
    if (r > 0 && order[src_axis[r - 1]] + 1 == order[perm[k]]) {
      od[r - 1] *= dims[perm[k]];
      ss[r - 1] = sstride[perm[k]];
      src_axis[r - 1] = perm[k];
      continue;
    }
    od[r] = dims[perm[k]];
    ss[r] = sstride[perm[k]];
    src_axis[r] = perm[k];
    ++r;
  }
  if (r == 0) {  // one element
    od[0] = 1; ss[0] = 1; r = 1;
  }
  TransposeArgs a;
  a.x = x; a.y = y; a.total = total;
  if (ss[r - 1] == 1) {
    for (int k = 0; k < 4; ++k) {
      const int from = k - (4 - r);
      a.od[k] = from >= 0 ? od[from] : 1;
      a.ss[k] = from >= 0 ? ss[from] : 0;
    }
    const int64_t blocks = (total + 255) / 256;
    hipLaunchKernelGGL(transpose_rows_kernel, dim3((unsigned)(blocks > (1 << 20) ? (1 << 20) : blocks)), dim3(256), 0, s, a);
    return;
  }
  // output strides of the reduced axes; D = the innermost output axis, S = the output axis whose source stride is 1
  int64_t ds[4], t = 1;
  for (int k = r - 1; k >= 0; --k) {
    ds[k] = t;
    t *= od[k];
  }
  int q = 0;
  while (ss[q] != 1) ++q;  // exists: the innermost source axis has extent > 1 here, or it would have been dropped / merged
  a.D = od[r - 1]; a.sd = ss[r - 1];
  a.S = od[q]; a.dd = ds[q];
  a.B0 = a.B1 = 1;
  a.bs[0] = a.bs[1] = a.bd[0] = a.bd[1] = 0;
  int nb = 0;
  for (int k = 0; k < r - 1; ++k) {
    if (k == q) continue;
    (nb == 0 ? a.B0 : a.B1) = od[k];
    a.bs[nb] = ss[k];
    a.bd[nb] = ds[k];
    ++nb;
  }
  if (nb == 1) {  // the one batch axis as B1 (b = b0 * B1 + b1 with B0 = 1)
    a.B1 = a.B0; a.bs[1] = a.bs[0]; a.bd[1] = a.bd[0];
    a.B0 = 1; a.bs[0] = a.bd[0] = 0;
  }
  const int64_t tiles = ((a.D + TILE - 1) / TILE) * ((a.S + TILE - 1) / TILE), batch = a.B0 * a.B1;
  const dim3 grid((unsigned)(tiles > (1 << 20) ? (1 << 20) : tiles), (unsigned)(batch > 65535 ? 65535 : batch));
  // every row start of both sides is a multiple of 4 floats from its base when both extents are (all outer strides are
  // multiples of D or of S)
  const bool vec = al16(x) && al16(y) && (a.D & 3) == 0 && (a.S & 3) == 0 && (a.sd & 3) == 0 && (a.dd & 3) == 0 &&
                   ((a.bs[0] | a.bs[1] | a.bd[0] | a.bd[1]) & 3) == 0;
  if (vec) hipLaunchKernelGGL(transpose_tile_kernel<1>, grid, dim3(256), 0, s, a);
  else hipLaunchKernelGGL(transpose_tile_kernel<0>, grid, dim3(256), 0, s, a);
}

// The join of an SSD head: operand p is NCHW [n][c[p]][hw[p]]; image b of it lands, as [hw[p]][c[p]], at y + b * stride + off[p]
// (stride = sum of c * hw): byte for byte transpose(0,2,3,1) -> reshape([0,-1,k]) -> concat(axis 1) for any k that divides
// every c[p].  grid: x = tiles of one operand's plane (loop), y = image (loop), z = operand.
template <int VEC>
__global__ __launch_bounds__(256) void concat_nhwc_kernel(ConcatNhwcArgs a) {
  __shared__ float tile[TILE * PITCH];
  const int p = blockIdx.z;
  const int64_t D = a.c[p], S = a.hw[p];
  const int64_t tiles_s = (S + TILE - 1) / TILE, tiles = tiles_s * ((D + TILE - 1) / TILE);
  for (int64_t b = blockIdx.y; b < a.n; b += gridDim.y) {
    const float* src = a.part[p] + b * D * S;
    float* dst = a.y + b * a.stride + a.off[p];
    for (int64_t t = blockIdx.x; t < tiles; t += gridDim.x) {
      const int64_t td = t / tiles_s, ts = t - td * tiles_s;
      transpose_tile<VEC>(src, S, dst, D, D, S, td * TILE, ts * TILE, tile);
    }
  }
}

void launch_concat_nhwc(const float* const* xs, const int64_t* channels, const int64_t* hw, int count, int64_t n, float* y, hipStream_t s) {
  int64_t stride = 0;
  bool vec = al16(y);
  for (int i = 0; i < count; ++i) {
    stride += channels[i] * hw[i];
    vec = vec && al16(xs[i]) && (channels[i] & 3) == 0 && (hw[i] & 3) == 0;
  }
  int64_t off = 0;
  for (int first = 0; first < count; first += CONCAT_MAX_PARTS) {
    ConcatNhwcArgs a;
    const int np = count - first < CONCAT_MAX_PARTS ? count - first : CONCAT_MAX_PARTS;
    int64_t most = 1;
    for (int p = 0; p < CONCAT_MAX_PARTS; ++p) {
      const bool used = p < np;
      a.part[p] = used ? xs[first + p] : nullptr;
      a.c[p] = used ? channels[first + p] : 0;
      a.hw[p] = used ? hw[first + p] : 0;
      a.off[p] = off;
      if (used) off += a.c[p] * a.hw[p];
      const int64_t tiles = ((a.c[p] + TILE - 1) / TILE) * ((a.hw[p] + TILE - 1) / TILE);
      most = tiles > most ? tiles : most;
    }
    a.y = y; a.stride = stride; a.n = n;
    const dim3 grid((unsigned)(most > (1 << 16) ? (1 << 16) : most), (unsigned)(n > 65535 ? 65535 : n), (unsigned)np);
    if (vec) hipLaunchKernelGGL(concat_nhwc_kernel<1>, grid, dim3(256), 0, s, a);
    else hipLaunchKernelGGL(concat_nhwc_kernel<0>, grid, dim3(256), 0, s, a);
  }
}

}  // namespace plhip
