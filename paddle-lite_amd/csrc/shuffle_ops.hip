// shuffle_ops.hip — the fp32 ops that join, part and permute tensors along an axis, for gfx950: concat, split,
// shuffle_channel, the tail of a ShuffleNetV2 unit (concat -> shuffle_channel(2) -> split -> calib) in one launch, and
// concat -> calib in one launch (the tail of a fire / inception module).
//
// Replaces (reference, ARM):
//   concat           ConcatCompute lite/kernels/arm/concat_compute.cc:37-57 (-> concat_func): `count` inputs [outer][c_i][inner]
//                    are copied into [outer][sum c_i][inner], in order
//   split            lite/backends/arm/math/split.cc:54-82: the inverse, output i takes c_i of the axis
//   shuffle_channel  lite/backends/arm/math/shuffle_channel.cc:24-55: per image, plane i * (c / group) + j goes to plane
//                    j * group + i (a memcpy of hw elements)
// Every op is a permutation of ROWS of contiguous floats (a plane of hw floats, or c_i * inner floats of one operand), so all
// four kernels are the same move: a group of 1 << LPP lanes owns one row, a block finds its rows from the grid (blockIdx and
// shifts of threadIdx; no lane divides), each input byte is read once and each output byte written once.  No LDS.
// fp32 values are MOVED (dword copies: NaN payloads and -0.0 keep their bits).  The int8 form of shuffle_channel and of the unit
// tail quantises exactly as calib_f32_to_i8_kernel does: round_sat_i8(inv * v), inv = 1.f / calib scale.
// vec (host decides once per launch: every row of every operand starts 16-byte aligned, int8 rows 4-byte aligned): a lane moves
// quads, 16 bytes of fp32 and 4 bytes of int8; otherwise a scalar loop (7x7 planes, bases off by one element).
#include "plhip_device.h"
#include "plhip_kernels.h"

namespace plhip {

namespace {

// one row of `len` floats from src to df (fp32, may be null) and dq (int8, may be null): this lane takes the items (quads with vec,
// else elements) first, first + step, ...; the lanes that share the row cover every item once
__device__ __forceinline__ void move_row(const float* __restrict__ src, float* __restrict__ df, int8_t* __restrict__ dq, int64_t len,
                                         int64_t first, int64_t step, int vec, float inv) {
  if (vec) {
    const int64_t nq = len >> 2;
    for (int64_t q = first; q < nq; q += step) {
      const v4f v = reinterpret_cast<const v4f*>(src)[q];
      if (df) reinterpret_cast<v4f*>(df)[q] = v;
      if (dq) reinterpret_cast<uint32_t*>(dq)[q] = calib4_i8(v, inv);
    }
    return;
  }
  for (int64_t i = first; i < len; i += step) {
    const float v = src[i];
    if (df) df[i] = v;
    if (dq) dq[i] = (int8_t)round_sat_i8(inv * v);
  }
}

// lanes per row (log2) for `work` items a row's lanes share: as launch_se_scale picks it
int lanes_log2(int64_t work) { return work <= 2 ? 0 : work <= 32 ? 4 : work <= 128 ? 6 : 8; }

bool al16(const void* p) { return ((uintptr_t)p & 15) == 0; }

unsigned grid_dim(int64_t v, int64_t cap) { return (unsigned)(v < 1 ? 1 : v > cap ? cap : v); }

}  // namespace

// concat (SPLIT == 0): part p's row o, a.len[p] floats, goes to whole + o * stride + off[p]; split (SPLIT == 1): the other way.
// grid: x = rows (1 << (8 - LPP) per block), y = slices of a row (LPP == 8 only: gridDim.y blocks share a long row, so that a
// concat with few rows, batch 1 or axis 0, still fills the device), z = the part.  Rows beyond gridDim.x's reach are taken in a loop.
template <int LPP, int SPLIT>
__global__ __launch_bounds__(256) void concat_split_kernel(ConcatArgs a) {
  const int p = blockIdx.z;
  const int64_t sub = (int64_t)blockIdx.y * (1 << LPP) + (threadIdx.x & ((1 << LPP) - 1));
  const int64_t lanes = (int64_t)gridDim.y << LPP;
  float* part = a.part[p];
  const int64_t len = a.len[p], off = a.off[p];
  const int64_t step = (int64_t)gridDim.x << (8 - LPP);
  for (int64_t row = ((int64_t)blockIdx.x << (8 - LPP)) + (threadIdx.x >> LPP); row < a.outer; row += step) {
    float* w = a.whole + row * a.stride + off;
    float* r = part + row * len;
    if (SPLIT) move_row(w, r, nullptr, len, sub, lanes, a.vec, 0.f);
    else move_row(r, w, nullptr, len, sub, lanes, a.vec, 0.f);
  }
}

template <int SPLIT>
static void launch_concat_split(const ConcatArgs& a, int nparts, hipStream_t s) {
  int64_t longest = 0;
  for (int p = 0; p < nparts; ++p) longest = a.len[p] > longest ? a.len[p] : longest;
  const int64_t work = a.vec ? longest >> 2 : longest;
  const int lpp = lanes_log2(work);
  // a block that owns a row alone takes about four items per lane; longer rows are shared by up to 1024 blocks
  const unsigned slices = lpp == 8 ? grid_dim((work + 1023) / 1024, 1024) : 1;
  const dim3 grid(grid_dim((a.outer + (256 >> lpp) - 1) / (256 >> lpp), 1 << 20), slices, (unsigned)nparts);
  if (lpp == 0) hipLaunchKernelGGL((concat_split_kernel<0, SPLIT>), grid, dim3(256), 0, s, a);
  else if (lpp == 4) hipLaunchKernelGGL((concat_split_kernel<4, SPLIT>), grid, dim3(256), 0, s, a);
  else if (lpp == 6) hipLaunchKernelGGL((concat_split_kernel<6, SPLIT>), grid, dim3(256), 0, s, a);
  else hipLaunchKernelGGL((concat_split_kernel<8, SPLIT>), grid, dim3(256), 0, s, a);
}

// parts[i]: `outer` rows of extents[i] * inner floats; whole: `outer` rows of sum(extents) * inner.  At most CONCAT_MAX_PARTS
// parts travel in one launch's argument struct; more parts are more launches (no pointer table in device memory, no copy).
void launch_concat_split(float* const* parts, const int64_t* extents, int count, int64_t outer, int64_t inner, float* whole,
                         int split, hipStream_t s) {
  int64_t total = 0;
  bool vec = al16(whole);
  for (int i = 0; i < count; ++i) {
    total += extents[i];
    vec = vec && al16(parts[i]) && ((extents[i] * inner) & 3) == 0;
  }
  int64_t off = 0;
  for (int first = 0; first < count; first += CONCAT_MAX_PARTS) {
    ConcatArgs a;
    const int np = count - first < CONCAT_MAX_PARTS ? count - first : CONCAT_MAX_PARTS;
    for (int p = 0; p < CONCAT_MAX_PARTS; ++p) {
      const bool used = p < np;
      a.part[p] = used ? parts[first + p] : nullptr;
      a.len[p] = used ? extents[first + p] * inner : 0;
      a.off[p] = off;
      if (used) off += a.len[p];
    }
    a.whole = whole;
    a.stride = total * inner;
    a.outer = outer;
    a.vec = vec ? 1 : 0;
    if (split) launch_concat_split<1>(a, np, s);
    else launch_concat_split<0>(a, np, s);
  }
}

// concat -> calib[fp32_to_int8]: part p's row o, a.len[p] floats, goes to yq (int8) and, where a.yf is given, yf (fp32, the bits
// moved) at o * stride + off[p].  Unlike move_row's lanes, which have one quad in flight, a lane takes one ITEM of W consecutive
// floats of a row: W == 16: four 16-byte loads in flight, one 16-byte int8 store (and four 16-byte fp32 stores); W == 4: a quad;
// W == 1: an element.  grid: x = slices of 256 items of a row (a long row is shared by several blocks; what gridDim.x cannot
// reach is taken in a loop), y = the row (loop), z = the part.  The part comes from blockIdx; no lane divides.
template <int LOGW>
__global__ __launch_bounds__(256) void concat_calib_kernel(ConcatCalibArgs a) {
  constexpr int W = 1 << LOGW;
  const int p = blockIdx.z;
  const float* __restrict__ part = a.part[p];
  const int64_t len = a.len[p], off = a.off[p];
  const int64_t items = len >> LOGW;  // the host takes W only where it divides every len
  const int64_t step = (int64_t)gridDim.x * 256;
  const float inv = a.inv;
  for (int64_t row = blockIdx.y; row < a.outer; row += gridDim.y) {
    const float* __restrict__ src = part + row * len;
    const int64_t dst = row * a.stride + off;
    float* __restrict__ df = a.yf ? a.yf + dst : nullptr;
    int8_t* __restrict__ dq = a.yq + dst;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < items; i += step) {
      if constexpr (W == 16) {
        const v4f* s4 = reinterpret_cast<const v4f*>(src) + 4 * i;
        const v4f v0 = s4[0], v1 = s4[1], v2 = s4[2], v3 = s4[3];
        if (df) {
          v4f* d4 = reinterpret_cast<v4f*>(df) + 4 * i;
          d4[0] = v0; d4[1] = v1; d4[2] = v2; d4[3] = v3;
        }
        v4i q;
        q[0] = (int)calib4_i8(v0, inv); q[1] = (int)calib4_i8(v1, inv); q[2] = (int)calib4_i8(v2, inv); q[3] = (int)calib4_i8(v3, inv);
        reinterpret_cast<v4i*>(dq)[i] = q;
      } else if constexpr (W == 4) {
        const v4f v = reinterpret_cast<const v4f*>(src)[i];
        if (df) reinterpret_cast<v4f*>(df)[i] = v;
        reinterpret_cast<uint32_t*>(dq)[i] = calib4_i8(v, inv);
      } else {
        const float v = src[i];
        if (df) df[i] = v;
        dq[i] = (int8_t)round_sat_i8(inv * v);
      }
    }
  }
}

// parts[i]: `outer` rows of extents[i] * inner floats; yf (may be null) / yq: `outer` rows of sum(extents) * inner.  The item
// width is decided once per call: 16 where every operand row and every output row offset is a multiple of 16 elements and every
// base is aligned for 16-byte accesses, 4 likewise for quads (yq: 4 bytes), else 1.  CONCAT_MAX_PARTS parts per launch, as concat.
void launch_concat_calib(const float* const* parts, const int64_t* extents, int count, int64_t outer, int64_t inner, float* yf,
                         int8_t* yq, float calib_scale, hipStream_t s) {
  int64_t total = 0, all = 0;
  bool al = al16(yf);
  for (int i = 0; i < count; ++i) {
    const int64_t len = extents[i] * inner;
    total += extents[i];
    all |= len;  // a low bit clear here is clear in every len, so in every row offset and in the output stride
    al = al && al16(parts[i]);
  }
  const int logw = al && (all & 15) == 0 && al16(yq) ? 4 : al && (all & 3) == 0 && ((uintptr_t)yq & 3) == 0 ? 2 : 0;
  const float inv = 1.f / calib_scale;  // type_trans.cc:45, as launch_calib_f32_to_i8
  int64_t off = 0;
  for (int first = 0; first < count; first += CONCAT_MAX_PARTS) {
    ConcatCalibArgs a;
    const int np = count - first < CONCAT_MAX_PARTS ? count - first : CONCAT_MAX_PARTS;
    int64_t longest = 0;
    for (int p = 0; p < CONCAT_MAX_PARTS; ++p) {
      const bool used = p < np;
      a.part[p] = used ? parts[first + p] : nullptr;
      a.len[p] = used ? extents[first + p] * inner : 0;
      a.off[p] = off;
      if (used) off += a.len[p];
      longest = a.len[p] > longest ? a.len[p] : longest;
    }
    a.yf = yf;
    a.yq = yq;
    a.stride = total * inner;
    a.outer = outer;
    a.inv = inv;
    const dim3 grid(grid_dim(((longest >> logw) + 255) / 256, 1 << 16), grid_dim(outer, 65535), (unsigned)np);
    if (logw == 4) hipLaunchKernelGGL(concat_calib_kernel<4>, grid, dim3(256), 0, s, a);
    else if (logw == 2) hipLaunchKernelGGL(concat_calib_kernel<2>, grid, dim3(256), 0, s, a);
    else hipLaunchKernelGGL(concat_calib_kernel<0>, grid, dim3(256), 0, s, a);
  }
}

// out[b][j * group + i] = in[b][i * cg + j], planes of hw floats.  grid: x = j (1 << (8 - LPP) planes per block), y = i, z = b;
// what the grid's y / z cannot reach is taken in loops.
template <int LPP>
__global__ __launch_bounds__(256) void shuffle_channel_kernel(const float* __restrict__ x, float* __restrict__ yf, int8_t* __restrict__ yq,
                                                              float inv, int n, int group, int cg, int hw, int vec) {
  const int j = (blockIdx.x << (8 - LPP)) + (threadIdx.x >> LPP);
  if (j >= cg) return;
  const int sub = threadIdx.x & ((1 << LPP) - 1);
  for (int b = blockIdx.z; b < n; b += gridDim.z)
    for (int i = blockIdx.y; i < group; i += gridDim.y) {
      const int64_t base = (int64_t)b * group * cg;
      const int64_t src = (base + (int64_t)i * cg + j) * hw, dst = (base + (int64_t)j * group + i) * hw;
      move_row(x + src, yf ? yf + dst : nullptr, yq ? yq + dst : nullptr, hw, sub, 1 << LPP, vec, inv);
    }
}

void launch_shuffle_channel(const float* x, float* yf, int8_t* yq, float calib_scale, int n, int c, int hw, int group, hipStream_t s) {
  const float inv = yq ? 1.f / calib_scale : 0.f;  // type_trans.cc:45, as launch_calib_f32_to_i8
  const int vec = (hw & 3) == 0 && al16(x) && al16(yf) && ((uintptr_t)yq & 3) == 0;
  const int lpp = lanes_log2(vec ? hw >> 2 : hw);
  const int cg = c / group;
  const dim3 grid((unsigned)((cg + (256 >> lpp) - 1) / (256 >> lpp)), grid_dim(group, 65535), grid_dim(n, 65535));
  if (lpp == 0) hipLaunchKernelGGL(shuffle_channel_kernel<0>, grid, dim3(256), 0, s, x, yf, yq, inv, n, group, cg, hw, vec);
  else if (lpp == 4) hipLaunchKernelGGL(shuffle_channel_kernel<4>, grid, dim3(256), 0, s, x, yf, yq, inv, n, group, cg, hw, vec);
  else if (lpp == 6) hipLaunchKernelGGL(shuffle_channel_kernel<6>, grid, dim3(256), 0, s, x, yf, yq, inv, n, group, cg, hw, vec);
  else hipLaunchKernelGGL(shuffle_channel_kernel<8>, grid, dim3(256), 0, s, x, yf, yq, inv, n, group, cg, hw, vec);
}

// The tail of a ShuffleNetV2 unit: shuffled channel c' = 2 * j + side is plane j of (side ? b : a); c' < split_at goes to lo_f32
// [n][split_at][hw], the rest to hi_f32 and / or hi_i8 [n][2 * h - split_at][hw].  grid: x = j, y = side, z = image (loop).
template <int LPP>
__global__ __launch_bounds__(256) void shuffle_unit_kernel(const float* __restrict__ a, const float* __restrict__ b, float* __restrict__ lo,
                                                           float* __restrict__ hf, int8_t* __restrict__ hq, float inv, int n, int h,
                                                           int hw, int split_at, int vec) {
  const int j = (blockIdx.x << (8 - LPP)) + (threadIdx.x >> LPP);
  if (j >= h) return;
  const int sub = threadIdx.x & ((1 << LPP) - 1);
  const int side = blockIdx.y;
  const float* src0 = side ? b : a;
  const int cs = 2 * j + side;  // the shuffled channel
  const int hi_c = 2 * h - split_at;
  for (int img = blockIdx.z; img < n; img += gridDim.z) {
    const float* src = src0 + ((int64_t)img * h + j) * hw;
    if (cs < split_at) {
      move_row(src, lo + ((int64_t)img * split_at + cs) * hw, nullptr, hw, sub, 1 << LPP, vec, 0.f);
    } else {
      const int64_t dst = ((int64_t)img * hi_c + (cs - split_at)) * hw;
      move_row(src, hf ? hf + dst : nullptr, hq ? hq + dst : nullptr, hw, sub, 1 << LPP, vec, inv);
    }
  }
}

void launch_shuffle_unit(const float* a, const float* b, float* lo, float* hf, int8_t* hq, float calib_scale, int n, int h, int hw,
                         int split_at, hipStream_t s) {
  const float inv = hq ? 1.f / calib_scale : 0.f;  // type_trans.cc:45, as launch_calib_f32_to_i8
  const int vec = (hw & 3) == 0 && al16(a) && al16(b) && al16(lo) && al16(hf) && ((uintptr_t)hq & 3) == 0;
  const int lpp = lanes_log2(vec ? hw >> 2 : hw);
  const dim3 grid((unsigned)((h + (256 >> lpp) - 1) / (256 >> lpp)), 2, grid_dim(n, 65535));
  if (lpp == 0) hipLaunchKernelGGL(shuffle_unit_kernel<0>, grid, dim3(256), 0, s, a, b, lo, hf, hq, inv, n, h, hw, split_at, vec);
  else if (lpp == 4) hipLaunchKernelGGL(shuffle_unit_kernel<4>, grid, dim3(256), 0, s, a, b, lo, hf, hq, inv, n, h, hw, split_at, vec);
  else if (lpp == 6) hipLaunchKernelGGL(shuffle_unit_kernel<6>, grid, dim3(256), 0, s, a, b, lo, hf, hq, inv, n, h, hw, split_at, vec);
  else hipLaunchKernelGGL(shuffle_unit_kernel<8>, grid, dim3(256), 0, s, a, b, lo, hf, hq, inv, n, h, hw, split_at, vec);
}

}  // namespace plhip
