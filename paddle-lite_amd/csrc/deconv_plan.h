// deconv_plan.h — which conv2d_transpose kernel runs a problem (deconv_i8.hip), with which tile and grid: pure host functions.
//
// Output geometry (lite/operators/conv_transpose_op.cc:45-95), the envelope of the MFMA phase route and its launch plan.  The C
// entries (plhip_capi_deconv.hip) and the launcher ask these functions, so name, pack and run cannot disagree.  Plain C++17, no
// HIP: a stand-alone program compiles it with g++ alone.
//
// Phase route.  In padded output coordinates v = oy + pt, u = ox + pl, output (v, u) = (S V + py, S U + px) reads the taps
// r = py + S ty, s = px + S tx of the filter at input (V - ty, U - tx): per phase (py, px) a stride-1 conv of the INPUT with a
// sub-filter, on the quotient grid (V, U) that all S * S phases share.  A lane owns 4 / S consecutive U of one V and every phase
// of them: S rows of 4 consecutive output columns.
#pragma once
#include <stddef.h>

namespace plhip {

constexpr int DECONV_LDS_TILE_MAX = 40 * 1024;  // staged pixel bytes per block: 3 blocks per CU

struct DeconvProblem {
  int n, cin, cout, h, w, kh, kw;
  int pad[4];  // top, bottom, left, right
  int sh, sw, dh, dw, groups;
  int out_h, out_w;  // output_size, 0 = the default
};

// OH = (H - 1) sh - pt - pb + dh (kh - 1) + 1; an output_size entry o with OH <= o < OH + sh replaces it.  false: a
// non-positive default or an entry outside that range
inline bool deconv_out_dims(const DeconvProblem& p, int* oh, int* ow) {
  const long dflt_h = (long)(p.h - 1) * p.sh - p.pad[0] - p.pad[1] + (long)p.dh * (p.kh - 1) + 1;
  const long dflt_w = (long)(p.w - 1) * p.sw - p.pad[2] - p.pad[3] + (long)p.dw * (p.kw - 1) + 1;
  if (dflt_h < 1 || dflt_w < 1 || dflt_h + p.sh > 0x7fffffffL || dflt_w + p.sw > 0x7fffffffL) return false;
  if (p.out_h && (p.out_h < dflt_h || p.out_h >= dflt_h + p.sh)) return false;
  if (p.out_w && (p.out_w < dflt_w || p.out_w >= dflt_w + p.sw)) return false;
  *oh = p.out_h ? p.out_h : (int)dflt_h;
  *ow = p.out_w ? p.out_w : (int)dflt_w;
  return true;
}

// the envelope of deconv_phase_int8_mfma32x32x32
inline bool deconv_phase_supported(const DeconvProblem& p) {
  if (p.groups != 1 || p.cin % 32 || p.dh != 1 || p.dw != 1 || p.kh > 4 || p.kw > 4) return false;
  if (p.sh != p.sw || (p.sh != 1 && p.sh != 2)) return false;
  return p.pad[0] < p.kh && p.pad[1] < p.kh && p.pad[2] < p.kw && p.pad[3] < p.kw;
}

// A fragments [M tile][chunk][tap r * kw + s][64 lanes][16 B]
inline size_t deconv_phase_packed_bytes(const DeconvProblem& p) {
  return (size_t)((p.cout + 31) / 32) * (p.cin / 32) * p.kh * p.kw * 1024;
}

// The tile of a block: TR rows of the quotient grid x CWq lane units (<= 32, a wave's lanes) with TR * CWq <= 128 (one unit per
// lane of the 4 waves, so the accumulators live across the K chunks); the staged input rows IR = TR + TY - 1 of WS = JU * WQ
// pixels (the segment's 4 / S * CWq columns + TX - 1 halo, rounded up to 4) within DECONV_LDS_TILE_MAX.
struct DeconvPlan {
  int S, NCH, MT, TY, TX, NV, NUq, TR, CWq, bands, nseg, IR, WQ, half;
  unsigned nblocks, nblocks_per_xcd;
  size_t lds;
};
inline bool deconv_phase_plan(const DeconvProblem& p, int oh, int ow, DeconvPlan* q) {
  const int S = p.sh, JU = 4 / S;
  q->S = S;
  q->NCH = p.cin / 32;
  q->MT = (p.cout + 31) / 32;
  q->TY = (p.kh + S - 1) / S;
  q->TX = (p.kw + S - 1) / S;
  q->NV = (oh - 1 + p.pad[0]) / S + 1;
  q->NUq = (ow - 1 + p.pad[2]) / 4 + 1;
  q->CWq = q->NUq < 32 ? q->NUq : 32;
  q->nseg = (q->NUq + q->CWq - 1) / q->CWq;
  const int WS = (q->CWq * JU + q->TX - 1 + 3) / 4 * 4;
  q->WQ = WS / JU;
  int tr = 128 / q->CWq;
  if (tr > q->NV) tr = q->NV;
  while (tr > 1 && (size_t)(tr + q->TY - 1) * WS * 32 > (size_t)DECONV_LDS_TILE_MAX) --tr;
  q->TR = tr;
  q->IR = tr + q->TY - 1;
  q->bands = (q->NV + tr - 1) / tr;
  q->half = q->IR * WS * 16;
  q->half += (64 - q->half % 128 + 128) % 128;  // half % 128 == 64: the two channel halves of a pixel on different banks
  q->lds = 1024 + 2 * (size_t)q->half;
  const size_t nb = (size_t)p.n * q->MT * q->bands * q->nseg;
  if (nb > ((size_t)1 << 31) - 16) return false;
  q->nblocks = (unsigned)nb;
  q->nblocks_per_xcd = (unsigned)((nb + 7) / 8);
  return true;
}

}  // namespace plhip
