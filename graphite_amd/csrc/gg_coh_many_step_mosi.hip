// gg_coh_many_step_mosi.hip — k_c_step_many<false, 1> (gg_coh_many_step.inc):
// the ensemble step kernel of the MOSI protocol, and its launcher.
#include "gg_coh_many.h"
namespace ggc {
#include "gg_coh_many_step.inc"
void launch_step_many_mosi(const CP& P, const ManyPair* pairs, uint32_t live, size_t lds, hipStream_t s, uint32_t L)
{
  hipLaunchKernelGGL((k_c_step_many<false, 1>), dim3(P.L, live), dim3(64), lds, s, pairs, L);
}
hipError_t step_many_mosi_set_lds(size_t lds)
{
  return hipFuncSetAttribute((const void*)k_c_step_many<false, 1>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
}
}  // namespace ggc
