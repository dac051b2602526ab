// gg_coh_many_step_shl2.hip — k_c_step_many<false, 2> and <false, 3>
// (gg_coh_many_step.inc): the ensemble step kernels of the shared-L2
// protocols (pr_l1_sh_l2_msi, pr_l1_sh_l2_mesi), and their launcher.
#include "gg_coh_many.h"
namespace ggc {
#include "gg_coh_many_step.inc"
void launch_step_many_shl2(const CP& P, const ManyPair* pairs, uint32_t live, size_t lds, hipStream_t s, uint32_t L)
{
  if (P.mesi) hipLaunchKernelGGL((k_c_step_many<false, 3>), dim3(P.L, live), dim3(64), lds, s, pairs, L);
  else hipLaunchKernelGGL((k_c_step_many<false, 2>), dim3(P.L, live), dim3(64), lds, s, pairs, L);
}
hipError_t step_many_shl2_set_lds(size_t lds)
{
  hipError_t e = hipFuncSetAttribute((const void*)k_c_step_many<false, 2>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
  if (e == hipSuccess) e = hipFuncSetAttribute((const void*)k_c_step_many<false, 3>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
  return e;
}
}  // namespace ggc
