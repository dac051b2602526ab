// gg_coh_many_step_fast.hip — k_c_step_many<true> (gg_coh_many_step.inc):
// the ensemble step kernel of configurations whose queues are all register
// history trees and whose caches track no miss types, and its launcher.
#include "gg_coh_many.h"

namespace ggc {

#include "gg_coh_many_step.inc"

void launch_step_many_fast(const CP& P, const ManyPair* pairs, uint32_t live, size_t lds, hipStream_t s, uint32_t L)
{
  hipLaunchKernelGGL(k_c_step_many<true>, dim3(P.L, live), dim3(64), lds, s, pairs, L);
}
hipError_t step_many_fast_set_lds(size_t lds)
{
  return hipFuncSetAttribute((const void*)k_c_step_many<true>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
}

}  // namespace ggc
