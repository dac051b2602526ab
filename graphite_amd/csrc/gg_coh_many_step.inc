// gg_coh_many_step.inc — k_c_step_many<F, PR>: k_c_step's body (step_body,
// device-driven quantum loop) for the live instances of an ensemble, grid
// (owned tiles, live instances), one wave per tile.  Included by
// gg_coh_many_step.hip (F = false), gg_coh_many_step_fast.hip (F = true),
// gg_coh_many_step_mosi.hip (PR = 1) and gg_coh_many_step_shl2.hip (PR = 2,
// 3), one unit per variant as for k_c_step.
// The instance's pair is indexed by blockIdx.y alone (wave-uniform: a scalar
// load); P and S stay behind its pointers, read where they are used (see
// gg_coh_step.inc).  quantum_end counts arrivals with gridDim.x, the
// instance's own tile count.  No in-kernel timing, no step trace.
template <bool F, int PR = 0>
__global__ void __launch_bounds__(64) k_c_step_many(const ManyPair* __restrict__ pairs, uint32_t L)
{
  const ManyPair pr = pairs[blockIdx.y];
  many_step_one<F, PR>(pr.P, pr.S, L);
}
