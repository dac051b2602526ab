// gg_coh_many_walk.hip — the ensemble's hop-by-hop walker kernels
// k_c_walk_many<PIPE, RQ>: k_c_walk's body (walk_body) for the live instances
// of an ensemble, grid (runs, live instances), and their host launcher.
// Device code: gg_coh_dev.h.
#include "gg_coh_many.h"

namespace ggc {

template <bool PIPE, bool RQ>
__global__ void __launch_bounds__(PIPE ? 64 * kMaxWalkWaves : 64) k_c_walk_many(const ManyPair* __restrict__ pairs, uint32_t L, int stage)
{
  const ManyPair pr = pairs[blockIdx.y];             // wave-uniform (see k_c_step_many)
  many_walk_one<PIPE, RQ>(pr.P, pr.S, L, stage);
}

void launch_walk_many(bool pipe, bool rq, uint32_t blocks, uint32_t threads, const ManyPair* pairs, uint32_t live,
                      size_t lds, hipStream_t s, uint32_t L, int stage)
{
  if (pipe && rq) hipLaunchKernelGGL((k_c_walk_many<true, true>), dim3(blocks, live), dim3(threads), lds, s, pairs, L, stage);
  else if (pipe) hipLaunchKernelGGL((k_c_walk_many<true, false>), dim3(blocks, live), dim3(threads), lds, s, pairs, L, stage);
  else if (rq) hipLaunchKernelGGL((k_c_walk_many<false, true>), dim3(blocks, live), dim3(64), lds, s, pairs, L, stage);
  else hipLaunchKernelGGL((k_c_walk_many<false, false>), dim3(blocks, live), dim3(64), lds, s, pairs, L, stage);
}
hipError_t walk_many_set_lds(size_t lds)
{
  for (const void* f : {(const void*)k_c_walk_many<true, true>, (const void*)k_c_walk_many<true, false>,
                        (const void*)k_c_walk_many<false, true>, (const void*)k_c_walk_many<false, false>})
    if (hipError_t e = hipFuncSetAttribute(f, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds)) return e;
  return hipSuccess;
}

}  // namespace ggc
