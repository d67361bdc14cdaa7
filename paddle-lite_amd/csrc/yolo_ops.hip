// yolo_ops.hip — yolo_box for gfx950: the decode of a YOLOv3 head's feature map into boxes and class scores, as the single-scale
// op in the reference's output layout and as the multi-scale head that writes what multiclass_nms reads.
//
// Replaces (reference, ARM): lite/backends/arm/math/yolo_box.cc:24-178 behind lite/kernels/arm/yolo_box_compute.cc:25-51, and for
// the head that kernel once per scale -> concat(axis 1) of the Boxes -> concat(axis 1) of the Scores -> transpose(0,2,1).
// X is [N][an * (5 + C)][H][W]: entry e (x, y, w, h, objectness, C classes) of anchor a is the plane (a * (5 + C) + e).
//   conf = sigmoid(x4); a cell with conf < conf_thresh is skipped: its box and scores are zeros (a NaN conf is kept)
//   cx = (l + sigmoid(x0) * scale + bias) * img_w / H          cy = (k + sigmoid(x1) * scale + bias) * img_h / H   (H for both)
//   bw = exp(x2) * anchor_w * img_w / (ratio * H)              bh = exp(x3) * anchor_h * img_h / (ratio * H)
//   box = (cx - bw / 2, cy - bh / 2, cx + bw / 2, cy + bh / 2), clipped as `v > 0 ? v : 0` and `v < img - 1 ? v : img - 1`
//   score[c] = conf * sigmoid(x[5 + c])
// fp32 in the reference's order of operations; the file is compiled with contraction OFF, exp is the library's expf.  Both
// kernels evaluate a cell with the SAME device functions (yolo_conf, yolo_cell_box, yolo_cell_score), so the head's bytes are
// the single-scale op's bytes moved.  Every output element is written by the launch that owns it, the zeros of skipped cells
// included: no memset, no atomics, no dependence on what the outputs held.
//
// yolo_box_kernel (reference layout, Scores [N][an * H * W][C] is the transposed side): a block owns 64 cells of one (image,
// anchor).  Wave 0 decodes the boxes, one 16-byte store each.  All four waves walk the classes in tiles of 64: a row of X (one
// class, 64 consecutive cells) is read by 64 consecutive lanes, scored and staged in LDS (pitch 65, as transpose_ops.hip), and
// written with consecutive lanes on the consecutive classes of a cell.
// yolo_head_kernel (Scores [N][C][P]): elementwise with H * W innermost on both sides.  grid x = (scale, anchor, chunk of
// cells), y = group of 8 class rows, z = image: what a block works on comes from its block index with compares and
// subtractions on the scalar side, no division.  A lane owns 4 consecutive cells where the scale allows 16-byte accesses (the
// `vec` bit), else one; the objectness is read once per block and kept in registers for its 8 class rows; the blocks of
// group 0 also decode the boxes, where the one per-lane division (cell -> row, column) is.
#include "plhip_device.h"
#include "plhip_kernels.h"

#pragma clang fp contract(off)

namespace plhip {

namespace {

constexpr int TILE = 64, PITCH = TILE + 1;
constexpr int HEAD_ROWS = 8;  // class rows of one block of the head kernel

bool al16(const void* p) { return ((uintptr_t)p & 15) == 0; }

// what a cell's arithmetic needs beside its five entries; uniform over a block
struct YoloImage {
  int img_h, img_w;     // ImgSize of the image
  int grid, input;      // H, downsample_ratio * H
  float scale, bias;    // scale_x_y, -0.5 * (scale_x_y - 1) narrowed
  float thresh;
  int clip;
};

__device__ __forceinline__ float yolo_sigmoid(float x) { return 1.f / (1.f + expf(-x)); }

// yolo_box.cc:139-142: the objectness and whether the cell is written (NaN < t is false: kept)
__device__ __forceinline__ float yolo_conf(float x4, const YoloImage& g, bool* keep) {
  const float conf = yolo_sigmoid(x4);
  *keep = !(conf < g.thresh);
  return conf;
}

// yolo_box.cc:40-46 and 65-81 for cell (row k, column l) with anchor (aw, ah)
__device__ __forceinline__ v4f yolo_cell_box(float x0, float x1, float x2, float x3, int k, int l, int aw, int ah, const YoloImage& g) {
  const float cx = ((float)l + yolo_sigmoid(x0) * g.scale + g.bias) * (float)g.img_w / (float)g.grid;
  const float cy = ((float)k + yolo_sigmoid(x1) * g.scale + g.bias) * (float)g.img_h / (float)g.grid;
  const float bw = expf(x2) * (float)aw * (float)g.img_w / (float)g.input;
  const float bh = expf(x3) * (float)ah * (float)g.img_h / (float)g.input;
  v4f o;
  o[0] = cx - bw / 2.f;
  o[1] = cy - bh / 2.f;
  o[2] = cx + bw / 2.f;
  o[3] = cy + bh / 2.f;
  if (g.clip) {
    const float mw = (float)(g.img_w - 1), mh = (float)(g.img_h - 1);
    o[0] = o[0] > 0.f ? o[0] : 0.f;
    o[1] = o[1] > 0.f ? o[1] : 0.f;
    o[2] = o[2] < mw ? o[2] : mw;
    o[3] = o[3] < mh ? o[3] : mh;
  }
  return o;
}

// yolo_box.cc:92
__device__ __forceinline__ float yolo_cell_score(float conf, float xc) { return conf * yolo_sigmoid(xc); }

__device__ __forceinline__ void store_box(float* __restrict__ boxes, int64_t box, const v4f& v, int vec) {
  if (vec) {
    reinterpret_cast<v4f*>(boxes)[box] = v;
    return;
  }
  float* p = boxes + 4 * box;
  p[0] = v[0]; p[1] = v[1]; p[2] = v[2]; p[3] = v[3];
}

__device__ __forceinline__ YoloImage yolo_image(const YoloCommon& c, const YoloScale& s, const int* __restrict__ img_size, int64_t b) {
  YoloImage g;
  g.img_h = img_size[2 * b];
  g.img_w = img_size[2 * b + 1];
  g.grid = s.h;
  g.input = s.ratio * s.h;
  g.scale = c.scale; g.bias = c.bias; g.thresh = c.thresh; g.clip = c.clip;
  return g;
}

}  // namespace

// grid: x = tiles of 64 cells of a plane, y = anchor, z = image (loop)
__global__ __launch_bounds__(256) void yolo_box_kernel(YoloBoxArgs a) {
  __shared__ float tile[TILE * PITCH];
  const YoloScale& s = a.s;
  const int hw = s.h * s.w, C = a.c.classes;
  const int an = blockIdx.y;
  const int cell0 = blockIdx.x * TILE;
  const int ncell = hw - cell0 < TILE ? hw - cell0 : TILE;
  const int col = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int aw = s.anchors[2 * an], ah = s.anchors[2 * an + 1];
  for (int64_t b = blockIdx.z; b < a.c.n; b += gridDim.z) {
    const YoloImage g = yolo_image(a.c, s, a.c.img_size, b);
    const float* __restrict__ x = s.x + (b * s.an + an) * (int64_t)(5 + C) * hw + cell0;
    const int64_t first = (b * s.an + an) * (int64_t)hw + cell0;  // the block's first box of [N][an * H * W]
    bool keep = false;
    float conf = 0.f;
    if (col < ncell) conf = yolo_conf(x[4 * (int64_t)hw + col], g, &keep);
    if (wave == 0 && col < ncell) {
      v4f o = {0.f, 0.f, 0.f, 0.f};
      if (keep) {
        const int cell = cell0 + col, k = cell / s.w, l = cell - k * s.w;
        o = yolo_cell_box(x[col], x[(int64_t)hw + col], x[2 * (int64_t)hw + col], x[3 * (int64_t)hw + col], k, l, aw, ah, g);
      }
      store_box(a.boxes, first + col, o, a.vec);
    }
    for (int c0 = 0; c0 < C; c0 += TILE) {
      const int ncls = C - c0 < TILE ? C - c0 : TILE;
      for (int r = wave; r < ncls; r += 4)
        if (col < ncell) tile[r * PITCH + col] = keep ? yolo_cell_score(conf, x[(5 + c0 + r) * (int64_t)hw + col]) : 0.f;
      __syncthreads();
      for (int r = wave; r < ncell; r += 4)
        if (col < ncls) a.scores[(first + r) * C + c0 + col] = tile[col * PITCH + r];
      __syncthreads();
    }
  }
}

// One lane's VEC cells of the head: VEC == 4 reads and writes quads (the host checked the alignment), VEC == 1 dwords.
template <int VEC>
__device__ __forceinline__ void yolo_head_cells(const YoloHeadArgs& a, const YoloScale& s, int an, int chunk, int group, int64_t b) {
  const int hw = s.h * s.w, C = a.c.classes;
  const int cell = (chunk * 256 + threadIdx.x) * VEC;
  if (cell >= hw) return;  // hw is a multiple of VEC: a lane's cells are all inside or all outside
  const YoloImage g = yolo_image(a.c, s, a.c.img_size, b);
  const float* __restrict__ x = s.x + (b * s.an + an) * (int64_t)(5 + C) * hw + cell;
  const int64_t p = s.p_off + (int64_t)an * hw + cell;  // the lane's first prior of the image's P
  float xv[VEC], conf[VEC];
  bool keep[VEC];
  auto load = [&](int row) {
    if (VEC == 4) {
      const v4f v = *reinterpret_cast<const v4f*>(x + row * (int64_t)hw);
      for (int i = 0; i < VEC; ++i) xv[i] = v[i];
    } else {
      xv[0] = x[row * (int64_t)hw];
    }
  };
  load(4);
  for (int i = 0; i < VEC; ++i) conf[i] = yolo_conf(xv[i], g, &keep[i]);
  const int c1 = (group + 1) * HEAD_ROWS < C ? (group + 1) * HEAD_ROWS : C;
  for (int c = group * HEAD_ROWS; c < c1; ++c) {
    load(5 + c);
    float* __restrict__ y = a.scores + (b * C + c) * (int64_t)a.P + p;
    if (VEC == 4) {
      v4f o;
      for (int i = 0; i < VEC; ++i) o[i] = keep[i] ? yolo_cell_score(conf[i], xv[i]) : 0.f;
      *reinterpret_cast<v4f*>(y) = o;
    } else {
      y[0] = keep[0] ? yolo_cell_score(conf[0], xv[0]) : 0.f;
    }
  }
  if (group != 0) return;
  float e[4][VEC];
  for (int r = 0; r < 4; ++r) {
    load(r);
    for (int i = 0; i < VEC; ++i) e[r][i] = xv[i];
  }
  const int aw = s.anchors[2 * an], ah = s.anchors[2 * an + 1];
  const int k0 = cell / s.w;
  int k = k0, l = cell - k0 * s.w;
  for (int i = 0; i < VEC; ++i) {
    v4f o = {0.f, 0.f, 0.f, 0.f};
    if (keep[i]) o = yolo_cell_box(e[0][i], e[1][i], e[2][i], e[3][i], k, l, aw, ah, g);
    store_box(a.boxes, b * a.P + p + i, o, a.box_vec);
    if (++l == s.w) { l = 0; ++k; }
  }
}

// grid: x = (scale, anchor, chunk of 256 lanes' cells) in this order, y = group of HEAD_ROWS classes, z = image (loop)
__global__ __launch_bounds__(256) void yolo_head_kernel(YoloHeadArgs a) {
  int si = 0;
  while (si + 1 < a.count && (int)blockIdx.x >= a.first[si + 1]) ++si;
  const YoloScale& s = a.s[si];
  int chunk = blockIdx.x - a.first[si], an = 0;
  while (chunk >= s.chunks) { chunk -= s.chunks; ++an; }
  for (int64_t b = blockIdx.z; b < a.c.n; b += gridDim.z) {
    if (s.vec) yolo_head_cells<4>(a, s, an, chunk, blockIdx.y, b);
    else yolo_head_cells<1>(a, s, an, chunk, blockIdx.y, b);
  }
}

void launch_yolo_box(YoloBoxArgs a, hipStream_t s) {
  const int hw = a.s.h * a.s.w;
  a.vec = al16(a.boxes);
  const dim3 grid((unsigned)((hw + TILE - 1) / TILE), (unsigned)a.s.an, (unsigned)(a.c.n > 65535 ? 65535 : a.c.n));
  hipLaunchKernelGGL(yolo_box_kernel, grid, dim3(256), 0, s, a);
}

void launch_yolo_head(YoloHeadArgs a, hipStream_t s) {
  int P = 0;
  for (int i = 0; i < a.count; ++i) {
    a.s[i].p_off = P;
    P += a.s[i].an * a.s[i].h * a.s[i].w;
  }
  a.P = P;
  a.box_vec = al16(a.boxes);
  // a row of scores starts (image * C + class) * P + p_off + anchor * hw floats behind the base: quads need every term on 4
  const bool rows16 = al16(a.scores) && ((P & 3) == 0 || (int64_t)a.c.n * a.c.classes == 1);
  int blocks = 0;
  for (int i = 0; i < YOLO_MAX_SCALES; ++i) {
    YoloScale& sc = a.s[i];
    a.first[i] = blocks;
    if (i >= a.count) continue;
    const int hw = sc.h * sc.w;
    sc.vec = rows16 && al16(sc.x) && (hw & 3) == 0 && (sc.p_off & 3) == 0;
    const int per_block = sc.vec ? 1024 : 256;
    sc.chunks = (hw + per_block - 1) / per_block;
    blocks += sc.an * sc.chunks;
  }
  const dim3 grid((unsigned)blocks, (unsigned)((a.c.classes + HEAD_ROWS - 1) / HEAD_ROWS), (unsigned)(a.c.n > 65535 ? 65535 : a.c.n));
  hipLaunchKernelGGL(yolo_head_kernel, grid, dim3(256), 0, s, a);
}

}  // namespace plhip
