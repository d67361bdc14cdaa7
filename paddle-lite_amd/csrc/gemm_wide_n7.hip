// gemm_wide_n7.hip — the wide-tile GEMM (gemm_wide_i8.hip / gemm_wide_kernel.h) with 7 n tiles per block: its own
// translation unit so that the instantiations compile in parallel.
#include "gemm_wide_kernel.h"

namespace plhip {

void launch_wide_n7(const GemmPlan& p, const GemmArgs& g, hipStream_t s) {
  if (g.KS == 4) launch_wide_t<7, 4>(p, g, s);
  else if (g.KS == 8) launch_wide_t<7, 8>(p, g, s);
  else if (g.KS == 16) launch_wide_t<7, 16>(p, g, s);
}

}  // namespace plhip
