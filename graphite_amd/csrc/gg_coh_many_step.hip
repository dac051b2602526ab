// gg_coh_many_step.hip — k_c_step_many<false> (gg_coh_many_step.inc: every
// queue form and the miss-type hooks) and the ensemble's step launcher, which
// picks the variant as launch_step does for a single run.
#include "gg_coh_many.h"

namespace ggc {

#include "gg_coh_many_step.inc"

void launch_step_many(const CP& P, const ManyPair* pairs, uint32_t live, size_t lds, hipStream_t s, uint32_t L)
{
  if (P.mosi) launch_step_many_mosi(P, pairs, live, lds, s, L);
  else if (P.shl2) launch_step_many_shl2(P, pairs, live, lds, s, L);
  else if (P.fast) launch_step_many_fast(P, pairs, live, lds, s, L);
  else hipLaunchKernelGGL(k_c_step_many<false>, dim3(P.L, live), dim3(64), lds, s, pairs, L);
}
hipError_t step_many_set_lds(size_t lds)
{
  hipError_t e = hipFuncSetAttribute((const void*)k_c_step_many<false>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
  if (e == hipSuccess) e = step_many_fast_set_lds(lds);
  if (e == hipSuccess) e = step_many_mosi_set_lds(lds);
  if (e == hipSuccess) e = step_many_shl2_set_lds(lds);
  return e;
}

}  // namespace ggc
