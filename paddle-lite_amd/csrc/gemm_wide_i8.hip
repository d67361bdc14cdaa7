// gemm_wide_i8.hip — the 1x1-convolution GEMM, third generation: ONE wide tile per CU, every operand byte in flight at once.
//
// Replaces the same reference code as gemm_i8.hip / gemm_tr_i8.hip (gemm_prepack_int8, lite/backends/arm/math/
// gemm_prepacked_int8.cc:2582-2744 hot loop, :643-796 epilogue; packb_int8 :3285; the batch loop of conv1x1s1_gemm_int8,
// conv_impl.cc:260-331) for the layers whose GEMM is SMALL per CU: MobileNetV1's 14x14 and 7x7 pointwise convs
// (512 -> 512: 50 k outputs x K 512 per CU at batch 128).
//
// Why a third kernel (round-2 evidence, profiles/r02_final_gemm_timeline_pw8.txt + tools/ingest_bench.hip, round 3):
//   * the ring kernels keep 3-4 K-steps (48-64 KB per CU) in flight and re-fetch the weight panel once per 128-column
//     tile: 430 KB of operand ingest per CU for the 512 -> 512 layer, taken in at ~21 B/clk;
//   * that rate is NOT what a CU can take in: LDS-DMA and register loads of 1-KiB pieces run at 56-59 B/clk/CU from L2
//     (tools/ingest_bench.hip); a K-step takes ~1000 cycles because the next one's bytes are still travelling
//     (64 KB in flight / 21 B/clk = 3000 cycles of loaded latency), and prologue, K loop and epilogue of the 424 short
//     blocks add up instead of overlapping.
// Here a block owns a 256 (m) x 32*NTT (n) tile = the whole share of one CU (1 block per CU, 8 waves), so
//   * the weight panel is read ONCE per CU: wave w loads ITS 32 rows x K straight into registers (fragment order, as
//     pack_weights_kernel wrote them: 1 KiB contiguous per load, the fastest form there is), K <= 1024;
//   * the activation tile (K x 32*NTT bytes, <= 128 KiB) is LDS-resident for the whole K loop: every DMA piece has its own
//     slot, so ALL loads of the tile are issued before the first MFMA (no ring, no slot reuse, no issue inside the loop)
//     and a K-step only waits for bytes that were requested K-steps * 2 instructions ago;
//   * operand reads as in gemm_tr_i8.hip: ds_read_b64_tr_b8 on the raw NCHW rows (no VALU in the K loop), activations
//     are the A operand, so a lane owns ONE output channel and 16 consecutive columns per 32 x 32 tile after two
//     v_permlane32_swap; the int8 tile leaves through a wave-private LDS image as 16-byte pieces of whole rows.
// LDS image of one K-step: [group of 8 chunks (128 columns)][kg = k/8][row q = k%8][slot s][16 B], chunk j = s ^ 2(q>>1).
// One DMA instruction = one (group, kg): 8 lanes walk 128 contiguous bytes of ONE k row (consecutive lanes on different
// rows measured 2-4x slower from L2, tools/ingest_bench.hip rows128T); the XOR keeps the transposed read conflict-free
// (a half-wave reads chunk pair (2t, 2t+1) of rows 0..7: slots 2((t&3) ^ (q>>1)) + parity, 16 distinct 16-byte bank slots).
// Column space, end-aligned last 16-byte chunk of an image, `skip`: as in gemm_i8_dma_kernel (gemm_i8.hip).
#include "gemm_wide_kernel.h"

namespace plhip {

int gemm_wide_stamp_lds() { return WIDE_STAMP_LDS; }

// the tile (n tiles per block so that the blocks fill the CUs once with as little idle tail as possible) is gemm_plan's choice
void run_gemm_wide(const GemmPlan& p, GemmArgs g, hipStream_t s) {
  PLHIP_SET_STAMPS(g, "wide", sizeof(unsigned long long) * 512 * 8 * WIDE_STAMP_SLOTS);
  if (p.NTT == 4) launch_wide_n4(p, g, s);
  else if (p.NTT == 7) launch_wide_n7(p, g, s);
  else launch_wide_n8(p, g, s);
}

}  // namespace plhip
