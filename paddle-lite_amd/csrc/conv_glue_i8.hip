// conv_glue_i8.hip — the kernels around the GEMM routes of a convolution: the weight pre-pack, im2col, the strided 1x1 gather and
// the zero-padded copies of the implicit-GEMM route, with their launchers (called from plhip_capi_conv.hip).
//
// Replaces (reference, ARM): prepackA_int8 (lite/backends/arm/math/gemm_prepacked_int8.cc:109-224) and im2col<int8_t>
// (lite/backends/arm/math/conv_impl.cc:103-153).
#include "plhip_device.h"
#include "plhip_kernels.h"
#include "dw_common.h"

namespace plhip {

// ---- weight pre-pack: [G][Mg][Kg] row-major (OIHW flattened) -> [G][MT32][KS][64 lanes][16 B] ----
// lane (r = lane&31, h = lane>>5), byte j  <-  W[g][mt32*32 + r][ks*32 + 16h + j]   (0 outside).
__global__ void pack_weights_kernel(const int8_t* __restrict__ w, int8_t* __restrict__ wp, int G, int Mg, int Kg,
                                    int MT32, int KS) {
  const size_t total = (size_t)G * MT32 * KS * 1024;
  for (size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (size_t)gridDim.x * blockDim.x) {
    const int j = idx & 15;
    const int lane = (idx >> 4) & 63;
    size_t t = idx >> 10;
    const int ks = t % KS;
    t /= KS;
    const int mt32 = t % MT32;
    const int grp = (int)(t / MT32);
    const int m = mt32 * 32 + (lane & 31);
    const int k = ks * 32 + 16 * (lane >> 5) + j;
    int8_t v = 0;
    if (m < Mg && k < Kg) v = w[((size_t)grp * Mg + m) * Kg + k];
    wp[idx] = v;
  }
}

// ---- im2col: x NCHW -> col[b][g][Kg][Np], Np = roundup(oh*ow, 4), pad columns and OOB taps = 0 ----
// Row index k = c*kh*kw + r*kw + q (conv_impl.cc:103-153).  One thread writes one dword (4 columns).
// grid = (column-quad tiles, Kg, batch*groups): the row (image, group, channel, tap) is block-uniform, so its decode runs
// on the scalar unit; a thread does ONE 32-bit division (its first column -> (oy, ox)) and walks the other three columns
// with a carry.  Stride-1 quads that stay inside one input row are fetched as one unaligned dword.  (The former
// 1-D form decoded everything per thread with 64-bit divisions: 128 us for the 57.8 MB buffer of BASELINE config #2.)
__global__ __launch_bounds__(256) void im2col_i8_kernel(Im2colArgs a) {
  const int np4 = a.Np >> 2;
  const int q4 = blockIdx.x * 256 + threadIdx.x;
  if (q4 >= np4) return;
  const int k = blockIdx.y;
  const int bg = blockIdx.z;
  const int b = bg / a.G, grp = bg - b * a.G;
  const int khkw = a.kh * a.kw;
  const int ci = k / khkw, rs = k - ci * khkw;
  const int kr = rs / a.kw, kq = rs - kr * a.kw;
  const int8_t* xp = a.x + ((size_t)b * a.cin + (size_t)grp * a.cin_g + ci) * a.h * a.w;
  const size_t row = (size_t)bg * a.Kg + k;
  int n = q4 * 4;
  int oy = (int)((uint32_t)n / (uint32_t)a.ow), ox = n - oy * a.ow;
  uint32_t out = 0;
  const int ih0 = oy * a.sh - a.pt + kr * a.dh, iw0 = ox * a.sw - a.pl + kq * a.dw;
  if (a.sw == 1 && n + 3 < a.N && ox + 3 < a.ow && ih0 >= 0 && ih0 < a.h && iw0 >= 0 && iw0 + 3 < a.w) {
    __builtin_memcpy(&out, xp + (size_t)ih0 * a.w + iw0, 4);
  } else if (a.sw == 2 && n + 3 < a.N && ox + 3 < a.ow && ih0 >= 0 && ih0 < a.h && iw0 >= 0 && iw0 + 7 < a.w) {
    // stride 2 (ResNet50's 1x1 stride-2 shortcuts): columns iw0, +2, +4, +6 of one row: one unaligned 8-byte fetch,
    // every other byte kept (the byte-by-byte walk below ran the three shortcut copies at ~1 TB/s)
    uint32_t d[2];
    __builtin_memcpy(d, xp + (size_t)ih0 * a.w + iw0, 8);
    out = __builtin_amdgcn_perm(d[1], d[0], 0x06040200u);
  } else {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      if (n + i < a.N) {
        const int ih = oy * a.sh - a.pt + kr * a.dh, iw = ox * a.sw - a.pl + kq * a.dw;
        if (ih >= 0 && ih < a.h && iw >= 0 && iw < a.w) out |= (uint32_t)(uint8_t)xp[(size_t)ih * a.w + iw] << (8 * i);
      }
      if (++ox == a.ow) {
        ox = 0;
        ++oy;
      }
    }
  }
  *reinterpret_cast<uint32_t*>(a.col + row * a.Np + (size_t)q4 * 4) = out;
}

void launch_pack_weights(const int8_t* w, int8_t* wp, int G, int Mg, int Kg, int MT32, int KS, hipStream_t s) {
  const size_t total = (size_t)G * MT32 * KS * 1024;
  const unsigned blocks = (unsigned)((total + 255) / 256 > 4096 ? 4096 : (total + 255) / 256);
  hipLaunchKernelGGL(pack_weights_kernel, dim3(blocks), dim3(256), 0, s, w, wp, G, Mg, Kg, MT32, KS);
}

// Zero-padded copy of the input for the implicit-GEMM route: xp[plane][ph][pw] = x[plane][ph - pt][pw - pl] or 0.
// One thread = one aligned dword of the flat padded buffer (two divisions, then carry propagation byte by byte).
__global__ void pad_input_i8_kernel(PadArgs a) {
  const long nq = a.total >> 2;
  const int plane_sz = a.ph * a.pw;
  for (long q = (long)blockIdx.x * blockDim.x + threadIdx.x; q < nq; q += (long)gridDim.x * blockDim.x) {
    // the padded buffer is < 2^31 bytes (conv_geom): magic-number divisions (two hardware divide sequences per dword made
    // this copy VALU-bound: 35 us for ResNet50's 55 MB res2 planes)
    const uint32_t o = (uint32_t)q << 2;
    int plane = (int)fastdiv_u31(o, a.div_plane_m, a.div_plane_s);
    const int rem = (int)(o - (uint32_t)plane * (uint32_t)plane_sz);
    int ph = (int)fastdiv_u31((uint32_t)rem, a.div_pw_m, a.div_pw_s), pw = rem - ph * a.pw;
    uint32_t v = 0;
    {  // interior dword (the common case): one unaligned 4-byte load
      const int ih = ph - a.pt, iw = pw - a.pl;
      if (plane < a.planes && pw + 3 < a.pw && ih >= 0 && ih < a.h && iw >= 0 && iw + 3 < a.w) {
        __builtin_memcpy(&v, a.x + ((size_t)plane * a.h + ih) * a.w + iw, 4);
        reinterpret_cast<uint32_t*>(a.xp)[q] = v;
        continue;
      }
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int ih = ph - a.pt, iw = pw - a.pl;
      if (plane < a.planes && ih >= 0 && ih < a.h && iw >= 0 && iw < a.w)
        v |= (uint32_t)(uint8_t)a.x[((size_t)plane * a.h + ih) * a.w + iw] << (8 * i);
      if (++pw == a.pw) {
        pw = 0;
        if (++ph == a.ph) {
          ph = 0;
          ++plane;
        }
      }
    }
    reinterpret_cast<uint32_t*>(a.xp)[q] = v;
  }
}

// Phase-split padded copy for the stride-2 implicit GEMM: xp[plane][p][q][y][x] = padded[plane][2y + p][2x + q].
// One thread = one aligned dword (4 consecutive x of one phase row): 4 source bytes at stride 2.
__global__ void pad_input_phase2_i8_kernel(PadArgs a) {
  const long nq = a.total >> 2;
  const int pwq = a.pw >> 2;  // launcher: phase rows are padded to a multiple of 4 columns
  for (long q = (long)blockIdx.x * blockDim.x + threadIdx.x; q < nq; q += (long)gridDim.x * blockDim.x) {
    // q < 2^29 (the buffer is < 2^31 bytes): 32-bit magic-number divisions, no 64-bit divide sequences
    const uint32_t t1 = fastdiv_u31((uint32_t)q, a.div_pwq_m, a.div_pwq_s);
    const int xq = (int)((uint32_t)q - t1 * (uint32_t)pwq);
    const uint32_t t2 = fastdiv_u31(t1, a.div_ph_m, a.div_ph_s);
    const int y = (int)(t1 - t2 * (uint32_t)a.ph);
    const int ph = (int)(t2 & 3);
    const long plane = (long)(t2 >> 2);
    uint32_t v = 0;
    if (plane < a.planes) {
      const int iy = 2 * y + (ph >> 1) - a.pt;
      if (iy >= 0 && iy < a.h) {
        const int8_t* row = a.x + ((size_t)plane * a.h + iy) * a.w;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const int ix = 2 * (4 * xq + i) + (ph & 1) - a.pl;
          if (ix >= 0 && ix < a.w) v |= (uint32_t)(uint8_t)row[ix] << (8 * i);
        }
      }
    }
    reinterpret_cast<uint32_t*>(a.xp)[q] = v;
  }
}

void launch_pad_input(const PadArgs& a_in, hipStream_t s) {
  PadArgs a = a_in;
  fastdiv_magic((long)a.ph * a.pw, a.div_plane_m, a.div_plane_s);
  fastdiv_magic(a.pw, a.div_pw_m, a.div_pw_s);
  fastdiv_magic(a.pw >> 2 > 0 ? a.pw >> 2 : 1, a.div_pwq_m, a.div_pwq_s);
  fastdiv_magic(a.ph, a.div_ph_m, a.div_ph_s);
  if (a.stride == 2) {
    long blocks2 = ((a.total >> 2) + 255) / 256;
    if (blocks2 > 65536) blocks2 = 65536;
    hipLaunchKernelGGL(pad_input_phase2_i8_kernel, dim3((unsigned)blocks2), dim3(256), 0, s, a);
    return;
  }
  long blocks = ((a.total >> 2) + 255) / 256;
  if (blocks > 65536) blocks = 65536;
  hipLaunchKernelGGL(pad_input_i8_kernel, dim3((unsigned)blocks), dim3(256), 0, s, a);
}

// 1x1 stride-2 convs (ResNet50's downsampling shortcuts: lite/backends/arm/math/conv_impl.cc:490-598 runs them through
// im2col too): the "im2col" is a strided gather, col[b][c][oy * ow + ox] = x[b][c][2 oy][2 ox].  One thread = 16 output
// bytes = 4 quads, each ONE unaligned 8-byte fetch with every other byte kept, one 16-byte store (the dword-per-thread
// form above ran the three shortcut copies of a ResNet50 step at 2.3 TB/s, 0.33 ms per 256 images: 4-byte stores).
// Needs kh = kw = 1, no padding in use, sw = 2.
__global__ __launch_bounds__(256) void subsample2_1x1_i8_kernel(Im2colArgs a) {
  // flat index -> (row = (image, group, channel), 16-byte chunk): a (chunks, channels, images) grid of mostly empty 256-thread
  // blocks (49 chunks per 28x28 row) was bound by the workgroup dispatch rate: 65 k blocks for 51 MB
  const int nch = (a.Np + 15) >> 4;
  const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= a.rows * (size_t)nch) return;
  const uint32_t rowi = (uint32_t)(idx / (uint32_t)nch);
  const int q16 = (int)(idx - (size_t)rowi * nch);
  const int bg = (int)(rowi / (uint32_t)a.Kg), k = (int)(rowi - (uint32_t)bg * a.Kg);
  const int b = bg / a.G, grp = bg - b * a.G;
  const int8_t* xp = a.x + ((size_t)b * a.cin + (size_t)grp * a.cin_g + k) * a.h * a.w;
  const size_t row = (size_t)bg * a.Kg + k;
  const int n0 = q16 * 16;
  int oy = (int)((uint32_t)n0 / (uint32_t)a.ow), ox = n0 - oy * a.ow;
  uint32_t out[4] = {0u, 0u, 0u, 0u};
#pragma unroll
  for (int d = 0; d < 4; ++d) {
    const int n = n0 + 4 * d;
    if (n + 3 < a.N && ox + 3 < a.ow && ox * 2 + 7 < a.w) {  // the quad inside one output row, its 8 source bytes inside the input row
      uint32_t dd[2];
      __builtin_memcpy(dd, xp + (size_t)(oy * a.sh) * a.w + ox * 2, 8);
      out[d] = __builtin_amdgcn_perm(dd[1], dd[0], 0x06040200u);
      ox += 4;
      if (ox >= a.ow) {
        ox -= a.ow;
        ++oy;
      }
    } else {  // a quad across two output rows (14- and 7-wide planes), the row's last quad when w is odd, the plane's tail
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        if (n + i < a.N) out[d] |= (uint32_t)(uint8_t)xp[(size_t)(oy * a.sh) * a.w + ox * 2] << (8 * i);
        if (++ox == a.ow) {
          ox = 0;
          ++oy;
        }
      }
    }
  }
  int8_t* dst = a.col + row * a.Np + (size_t)n0;
  if (n0 + 16 <= a.Np) {
    const v4i v = {(int)out[0], (int)out[1], (int)out[2], (int)out[3]};
    __builtin_memcpy(dst, &v, 16);  // (rows are 4-byte aligned: Np % 4 == 0)
  } else {
#pragma unroll
    for (int d = 0; d < 4; ++d)
      if (n0 + 4 * d < a.Np) __builtin_memcpy(dst + 4 * d, &out[d], 4);
  }
}

void launch_im2col(const Im2colArgs& a, hipStream_t s) {
  // rows = batch * G * Kg; Kg and batch*G ride on grid.y / grid.z (<= 65535 each, checked by the caller)
  const unsigned bg = (unsigned)(a.rows / (size_t)a.Kg);
  const int sub_env = knob("SUBSAMPLE_1X1", 1);  // 0 = the generic im2col kernel (A/B runs)
  if (sub_env && a.kh == 1 && a.kw == 1 && a.pt == 0 && a.pl == 0 && a.sw == 2 && a.Kg == a.cin_g &&
      (a.oh - 1) * a.sh < a.h && (a.ow - 1) * 2 < a.w) {  // (no tap in a bottom / right padding)
    const size_t threads = a.rows * (size_t)((a.Np + 15) >> 4);
    if (threads < ((size_t)1 << 31) * 256) {
      hipLaunchKernelGGL(subsample2_1x1_i8_kernel, dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, s, a);
      return;
    }
  }
  hipLaunchKernelGGL(im2col_i8_kernel, dim3((unsigned)(((a.Np >> 2) + 255) / 256), (unsigned)a.Kg, bg), dim3(256), 0, s, a);
}

}  // namespace plhip