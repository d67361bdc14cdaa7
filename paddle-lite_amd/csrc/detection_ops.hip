// detection_ops.hip — the tail of a detection network for gfx950: box_coder (decode_center_size) and multiclass_nms, both on the
// device, without a host synchronisation and with outputs of a fixed size, so that a step with a detection head can still be
// captured and replayed as a launch graph.
//
// Replaces (reference):
//   box_coder       lite/kernels/arm/box_coder_compute.cc:92-158 (DecodeCenterSize<axis, var_size>)
//   multiclass_nms  lite/kernels/host/multiclass_nms_compute.cc:31-322, the 3-D score form.  The reference runs it on the HOST and
//                   writes a tensor whose length is the number of detections; here the rows go into [N][keep_top_k][6], padded
//                   with -1, and the lengths into count[N].
// The NMS result depends on the last bit of every overlap (a candidate is kept iff overlap <= nms_threshold), so this file is
// compiled with floating-point contraction OFF and the overlap is written exactly as JaccardOverlap is: the early 0 for disjoint
// boxes, area 0 for an inverted box, inter / (a1 + a2 - inter).  0 / 0 is NaN and `NaN <= t` is false: the test is
// !(overlap <= t), never overlap > t.
//
// multiclass_nms, two launches, no atomics (every result is a function of the inputs alone):
//   A  grid (class, image), 256 lanes.  A1: the candidates (score > score_threshold, so never a NaN) are compacted in prior order
//      with ballot / popcount prefixes into 64-bit LDS keys: high word = the score's bits mapped so that unsigned ascending order
//      is descending score (-0 folded onto +0), low word = the prior.  Keys are unique, so any correct sort IS the reference's
//      stable_sort.  A2: bitonic sort of the next power of two.  A3: the boxes of the first K = min(count, nms_top_k) keys are
//      staged in LDS (over the dead tail of the keys).  A4: greedy scan: for i in order, skip if removed (one LDS word, read by
//      all lanes: the branch is uniform), else all lanes evaluate overlap(j, i) for j > i and mark !(overlap <= t); one barrier
//      per KEPT box.  A5: the kept (score, prior) list goes to the workspace, cut at min(K, keep_top_k) entries: entry r of a class
//      has r entries of its own class in front of it in the image's order, so later ones never reach the image's top keep_top_k.
//   B  one block per image: gathers the lists in (label, position) order, sorts by (score descending, label, position), cuts at
//      keep_top_k, sorts the survivors by (label, position) and writes rows, count and index; the rest is padded with -1.
#include "plhip_device.h"
#include "plhip_kernels.h"

#pragma clang fp contract(off)

namespace plhip {

namespace {

// four consecutive floats: one 16-byte access where the host found the base aligned, else four dword accesses
__device__ __forceinline__ v4f load4(const float* __restrict__ p, int64_t quad, int vec) {
  if (vec) return reinterpret_cast<const v4f*>(p)[quad];
  v4f v;
  v[0] = p[4 * quad]; v[1] = p[4 * quad + 1]; v[2] = p[4 * quad + 2]; v[3] = p[4 * quad + 3];
  return v;
}

__device__ __forceinline__ void store4(float* __restrict__ p, int64_t quad, const v4f& v, int vec) {
  if (vec) {
    reinterpret_cast<v4f*>(p)[quad] = v;
    return;
  }
  p[4 * quad] = v[0]; p[4 * quad + 1] = v[1]; p[4 * quad + 2] = v[2]; p[4 * quad + 3] = v[3];
}

bool al16(const void* p) { return ((uintptr_t)p & 15) == 0; }

}  // namespace

// ------------------------------------------------------------------ box_coder, decode_center_size
// One lane per box.  target / y [rows][cols][4]; the prior box and its variance are row (axis 0: j, axis 1: i) of prior / pvar.
// var 2: pvar tensor, 1: the four attribute values, 0: none (the reference multiplies by 1.f, which changes no bit).
__global__ __launch_bounds__(256) void box_coder_decode_kernel(BoxCoderArgs a) {
  const float nn = a.normalized ? 0.f : 1.f;  // (normalized == false) of the reference
  const int64_t step = (int64_t)gridDim.x * 256;
  for (int64_t b = (int64_t)blockIdx.x * 256 + threadIdx.x; b < a.boxes; b += step) {
    const int64_t i = b / a.cols, j = b - i * a.cols;
    const int64_t pr = a.axis == 0 ? j : i;
    const v4f p = load4(a.prior, pr, a.vec);
    const v4f t = load4(a.target, b, a.vec);
    v4f var;
    if (a.var == 2) var = load4(a.pvar, pr, a.vec);
    else var = a.variance;
    const float pw = p[2] - p[0] + nn;
    const float ph = p[3] - p[1] + nn;
    const float pcx = p[0] + pw / 2.f;
    const float pcy = p[1] + ph / 2.f;
    const float cx = var[0] * t[0] * pw + pcx;
    const float cy = var[1] * t[1] * ph + pcy;
    const float w = expf(var[2] * t[2]) * pw;
    const float h = expf(var[3] * t[3]) * ph;
    v4f o;
    o[0] = cx - w / 2.f;
    o[1] = cy - h / 2.f;
    o[2] = cx + w / 2.f - nn;
    o[3] = cy + h / 2.f - nn;
    store4(a.y, b, o, a.vec);
  }
}

void launch_box_coder_decode(BoxCoderArgs a, hipStream_t s) {
  a.boxes = a.rows * a.cols;
  a.vec = al16(a.prior) && al16(a.target) && al16(a.y) && (a.var != 2 || al16(a.pvar));
  const int64_t blocks = (a.boxes + 255) / 256;
  hipLaunchKernelGGL(box_coder_decode_kernel, dim3((unsigned)(blocks > (1 << 20) ? (1 << 20) : blocks)), dim3(256), 0, s, a);
}

// ------------------------------------------------------------------ multiclass_nms
namespace {

// BBoxArea / JaccardOverlap of multiclass_nms_compute.cc:51-87, operation for operation (std::max(a, b) is a < b ? b : a,
// std::min(a, b) is b < a ? b : a).  b1: the candidate, b2: a box kept before it.
__device__ __forceinline__ float bbox_area(const v4f& b, int normalized) {
  if (b[2] < b[0] || b[3] < b[1]) return 0.f;
  const float w = b[2] - b[0];
  const float h = b[3] - b[1];
  return normalized ? w * h : (w + 1.f) * (h + 1.f);
}

__device__ __forceinline__ float jaccard_overlap(const v4f& b1, const v4f& b2, int normalized) {
  if (b2[0] > b1[2] || b2[2] < b1[0] || b2[1] > b1[3] || b2[3] < b1[1]) return 0.f;
  const float ixmin = b1[0] < b2[0] ? b2[0] : b1[0];
  const float iymin = b1[1] < b2[1] ? b2[1] : b1[1];
  const float ixmax = b2[2] < b1[2] ? b2[2] : b1[2];
  const float iymax = b2[3] < b1[3] ? b2[3] : b1[3];
  const float norm = normalized ? 0.f : 1.f;
  const float iw = ixmax - ixmin + norm;
  const float ih = iymax - iymin + norm;
  const float inter = iw * ih;
  const float a1 = bbox_area(b1, normalized);
  const float a2 = bbox_area(b2, normalized);
  return inter / (a1 + a2 - inter);
}

// the high word of a key: unsigned ascending order of it is descending order of the score; -0.0 and +0.0 share one value
__device__ __forceinline__ uint32_t descending_bits(float s) {
  uint32_t b = __float_as_uint(s);
  if (b == 0x80000000u) b = 0u;
  const uint32_t asc = (b & 0x80000000u) ? ~b : (b | 0x80000000u);
  return ~asc;
}

// The block's 256 lanes append the keys of the lanes with `pred`, in lane order, behind the `running` keys dst holds; returns the
// new length.  Every lane of the block calls it; wcnt: 4 ints of LDS.  Two barriers.
__device__ __forceinline__ int block_append(bool pred, uint64_t key, uint64_t* dst, int running, int* wcnt) {
  const uint64_t bal = __ballot(pred);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int before = __popcll(bal & ((1ull << lane) - 1ull));
  if (lane == 0) wcnt[wave] = __popcll(bal);
  __syncthreads();
  int off = running, total = 0;
  for (int w = 0; w < 4; ++w) {
    const int c = wcnt[w];
    if (w < wave) off += c;
    total += c;
  }
  if (pred) dst[off + before] = key;
  __syncthreads();
  return running + total;
}

// ascending bitonic sort of k[0 .. n2), n2 a power of two, by the block's 256 lanes; the keys are visible to all lanes on entry
// (a barrier behind the last write) and on return
__device__ __forceinline__ void bitonic_sort(uint64_t* k, int n2) {
  for (int size = 2; size <= n2; size <<= 1)
    for (int j = size >> 1; j > 0; j >>= 1) {
      for (int t = threadIdx.x; t < (n2 >> 1); t += 256) {
        const int i = ((t & ~(j - 1)) << 1) | (t & (j - 1));
        const int p = i | j;
        const uint64_t lo = k[i], hi = k[p];
        const bool up = (i & size) == 0;
        if ((lo > hi) == up) {
          k[i] = hi;
          k[p] = lo;
        }
      }
      __syncthreads();
    }
}

// pads k[n .. n2) with keys that sort last and sorts; returns with the keys visible
__device__ __forceinline__ void pad_and_sort(uint64_t* k, int n) {
  int n2 = 1;
  while (n2 < n) n2 <<= 1;
  for (int i = n + threadIdx.x; i < n2; i += 256) k[i] = ~0ull;
  __syncthreads();
  bitonic_sort(k, n2);
}

}  // namespace

// stage A: one block per (class, image)
__global__ __launch_bounds__(256) void nms_class_kernel(NmsArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char nms_lds[];
  const int cls = blockIdx.x, img = blockIdx.y;
  const int64_t slot = (int64_t)img * a.C + cls;
  if (cls == a.bg) {
    if (threadIdx.x == 0) a.ws_len[slot] = 0;
    return;
  }
  uint64_t* keys = reinterpret_cast<uint64_t*>(nms_lds);           // [pow2 >= P]
  v4f* box = reinterpret_cast<v4f*>(nms_lds + a.box_off);           // [kmax], over keys[kmax ..), dead once sorted
  int* kept = reinterpret_cast<int*>(nms_lds + a.kept_off);         // [cap]
  int* wcnt = reinterpret_cast<int*>(nms_lds + a.wcnt_off);         // [4]
  unsigned char* removed = nms_lds + a.removed_off;                 // [kmax]
  const float* __restrict__ sc = a.scores + (int64_t)img * a.C * a.P + (int64_t)cls * a.ssc;
  const float* __restrict__ gb = a.boxes + (int64_t)img * a.P * 4;

  // A1: candidates in prior order
  int cnt = 0;
  for (int base = 0; base < a.P; base += 256) {
    const int p = base + threadIdx.x;
    const float s = p < a.P ? sc[(int64_t)p * a.ssp] : 0.f;
    const bool pred = p < a.P && s > a.sthr;
    cnt = block_append(pred, ((uint64_t)descending_bits(s) << 32) | (uint32_t)p, keys, cnt, wcnt);
  }
  // A2
  pad_and_sort(keys, cnt);
  // A3
  const int K = cnt < a.kmax ? cnt : a.kmax;
  for (int i = threadIdx.x; i < K; i += 256) {
    box[i] = load4(gb, (uint32_t)keys[i], a.vec);
    removed[i] = 0;
  }
  __syncthreads();
  // A4: removed[i] is final once every kept box in front of i has had its barrier
  int nk = 0;
  for (int i = 0; i < K && nk < a.cap; ++i) {
    if (__builtin_amdgcn_readfirstlane((int)removed[i])) continue;
    if (threadIdx.x == 0) kept[nk] = i;
    ++nk;
    const v4f bi = box[i];
    for (int j = i + 1 + threadIdx.x; j < K; j += 256) {
      if (removed[j]) continue;
      const float ov = jaccard_overlap(box[j], bi, a.normalized);
      if (!(ov <= a.nthr)) removed[j] = 1;
    }
    __syncthreads();
  }
  // A5: the score's own bits (a -0.0 stays -0.0 in the output row)
  uint64_t* list = a.ws_list + slot * a.cap;
  for (int r = threadIdx.x; r < nk; r += 256) {
    const uint32_t prior = (uint32_t)keys[kept[r]];
    list[r] = ((uint64_t)__float_as_uint(sc[(int64_t)prior * a.ssp]) << 32) | prior;
  }
  if (threadIdx.x == 0) a.ws_len[slot] = nk;
}

// stage B: one block per image
__global__ __launch_bounds__(256) void nms_image_kernel(NmsArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char nms_lds[];
  const int img = blockIdx.x;
  uint64_t* keys = reinterpret_cast<uint64_t*>(nms_lds);      // [pow2 >= nact * cap]
  int* wcnt = reinterpret_cast<int*>(nms_lds + a.wcnt_off_b);  // [4]
  const int* __restrict__ lens = a.ws_len + (int64_t)img * a.C;
  const uint64_t* __restrict__ lists = a.ws_list + (int64_t)img * a.C * a.cap;
  const bool has_bg = a.bg >= 0 && a.bg < a.C;
  const int S = (a.C - (has_bg ? 1 : 0)) * a.cap;  // slot s = (rank of the label among the classes that ran) * cap + position

  int T = 0;
  for (int base = 0; base < S; base += 256) {
    const int s = base + threadIdx.x;
    bool pred = false;
    uint64_t key = 0;
    if (s < S) {
      const int rank = s / a.cap, pos = s - rank * a.cap;
      const int label = rank + (has_bg && rank >= a.bg ? 1 : 0);
      if (pos < lens[label]) {
        pred = true;
        const float score = __uint_as_float((uint32_t)(lists[(int64_t)label * a.cap + pos] >> 32));
        key = ((uint64_t)descending_bits(score) << 32) | (uint32_t)s;
      }
    }
    T = block_append(pred, key, keys, T, wcnt);
  }
  pad_and_sort(keys, T);  // (score descending, label, position)
  const int Kk = T < a.keep ? T : a.keep;
  int n2 = 1;
  while (n2 < Kk) n2 <<= 1;
  for (int i = threadIdx.x; i < n2; i += 256) keys[i] = i < Kk ? (keys[i] & 0xffffffffull) : ~0ull;
  __syncthreads();
  bitonic_sort(keys, n2);  // (label, position)

  const float* __restrict__ gb = a.boxes + (int64_t)img * a.P * 4;
  float* __restrict__ out = a.out + (int64_t)img * a.keep * 6;
  int* __restrict__ index = a.index ? a.index + (int64_t)img * a.keep : nullptr;
  for (int r = threadIdx.x; r < a.keep; r += 256) {
    float row[6] = {-1.f, -1.f, -1.f, -1.f, -1.f, -1.f};
    int idx = -1;
    if (r < Kk) {
      const int s = (int)(uint32_t)keys[r];
      const int rank = s / a.cap, pos = s - rank * a.cap;
      const int label = rank + (has_bg && rank >= a.bg ? 1 : 0);
      const uint64_t e = lists[(int64_t)label * a.cap + pos];
      const uint32_t prior = (uint32_t)e;
      const v4f b = load4(gb, prior, a.vec);
      row[0] = (float)label;
      row[1] = __uint_as_float((uint32_t)(e >> 32));
      row[2] = b[0]; row[3] = b[1]; row[4] = b[2]; row[5] = b[3];
      idx = img * a.P + (int)prior;
    }
    for (int k = 0; k < 6; ++k) out[(int64_t)r * 6 + k] = row[k];
    if (index) index[r] = idx;
  }
  if (threadIdx.x == 0) a.count[img] = Kk;
}

namespace {
int64_t pow2_at_least(int64_t v) {
  int64_t p = 1;
  while (p < v) p <<= 1;
  return p;
}
int64_t rup16(int64_t v) { return (v + 15) & ~(int64_t)15; }
}  // namespace

// kmax = min(nms_top_k, P) (nms_top_k < 0: P), cap = min(kmax, keep_top_k), nact = classes other than the background
void nms_sizes(int C, int P, int bg, int nms_top_k, int keep_top_k, int* kmax, int* cap, int* nact) {
  *kmax = nms_top_k < 0 || nms_top_k > P ? P : nms_top_k;
  *cap = *kmax < keep_top_k ? *kmax : keep_top_k;
  *nact = C - (bg >= 0 && bg < C ? 1 : 0);
}

void launch_multiclass_nms(NmsArgs a, int N, hipStream_t s) {
  // stage A's LDS: [keys: pow2 >= P | boxes from byte 8 kmax on, 16 kmax bytes][kept: 4 cap][wcnt: 16][removed: kmax]
  const int64_t keys_a = 8 * pow2_at_least(a.P);
  a.box_off = (int)rup16(8 * (int64_t)a.kmax);
  const int64_t body = keys_a > a.box_off + 16 * (int64_t)a.kmax ? keys_a : a.box_off + 16 * (int64_t)a.kmax;
  a.kept_off = (int)rup16(body);
  a.wcnt_off = (int)rup16(a.kept_off + 4 * (int64_t)a.cap);
  a.removed_off = a.wcnt_off + 16;
  const int lds_a = (int)rup16(a.removed_off + (int64_t)a.kmax);
  // stage B's: [keys: pow2 >= nact * cap][wcnt: 16]
  a.wcnt_off_b = (int)(8 * pow2_at_least((int64_t)a.nact * a.cap));
  const int lds_b = a.wcnt_off_b + 16;
  a.vec = al16(a.boxes);
  (void)hipFuncSetAttribute((const void*)nms_class_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, lds_a);
  (void)hipFuncSetAttribute((const void*)nms_image_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, lds_b);
  hipLaunchKernelGGL(nms_class_kernel, dim3((unsigned)a.C, (unsigned)N), dim3(256), (size_t)lds_a, s, a);
  hipLaunchKernelGGL(nms_image_kernel, dim3((unsigned)N), dim3(256), (size_t)lds_b, s, a);
}

}  // namespace plhip
