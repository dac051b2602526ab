// gg_coh_many.h — the ensemble launches of gg_coherent_run_many (DESIGN.md
// §4f): many independent coherent runs side by side in one grid, the instance
// chosen by blockIdx.y.  The kernels are the bodies of k_c_step / k_c_walk
// (gg_coh_dev.h) behind another wrapper; nothing here is on the path of the
// single-run kernels.
#pragma once
#include "gg_coh_dev.h"

namespace ggc {

// one live instance of an ensemble launch: the device copies of its launch
// state (gg_coh_state::Pd / Sd)
struct ManyPair { const CP* P; const CS* S; };
// what the host looks at after a batch, per live instance (k_many_poll)
struct ManyPoll { uint64_t done; uint32_t err; uint32_t err_line; };

// k_c_step's P and S are restrict kernel arguments, so its loads of the
// launch state are known unclobbered and stay scalar loads.  Pointers loaded
// from the pair array carry no such promise (and the bodies are too large for
// the inliner's capture analysis to grant it), so the walkers' loads behind
// their barriers and atomics turned into vector loads (+15 VGPRs, spills to
// scratch).  The two structs are written by the host at gg_coherent_begin only
// — constant for every kernel — so they are read through the constant address
// space, which says exactly that.
template <class T> __device__ __forceinline__ const T* launch_const(const T* p)
{
  typedef const T __attribute__((address_space(4))) * CT;
  return (const T*)(CT)(uintptr_t)p;          // (through an integer: a plain cast chain is folded away)
}
template <bool F, int PR>
__device__ __forceinline__ void many_step_one(const CP* Pp, const CS* Sp, uint32_t L)
{
  const CP& P = *launch_const(Pp);
  const CS& S = *launch_const(Sp);
  kwarm(&P, &S);
  TraceWin W{~0ull, 0, 0};
  step_body<false, false, F, PR>(P, S, L, 1u, (uint64_t)0, W);
}
template <bool PIPE, bool RQ>
__device__ __forceinline__ void many_walk_one(const CP* Pp, const CS* Sp, uint32_t L, int stage)
{
  const CP& P = *launch_const(Pp);
  const CS& S = *launch_const(Sp);
  kwarm(&P, &S);
  walk_body<PIPE, RQ>(P, S, L, stage, blockIdx.x);
}

// ---- launchers (gg_coh_many_step*.hip, gg_coh_many_walk.hip) ----
// grid (owned tiles | runs, live instances); the variant is the one the
// single-run launchers pick from the same CP
void launch_step_many(const CP& P, const ManyPair* pairs, uint32_t live, size_t lds, hipStream_t s, uint32_t L);
void launch_step_many_fast(const CP& P, const ManyPair* pairs, uint32_t live, size_t lds, hipStream_t s, uint32_t L);
void launch_step_many_mosi(const CP& P, const ManyPair* pairs, uint32_t live, size_t lds, hipStream_t s, uint32_t L);
void launch_step_many_shl2(const CP& P, const ManyPair* pairs, uint32_t live, size_t lds, hipStream_t s, uint32_t L);
hipError_t step_many_set_lds(size_t lds);
hipError_t step_many_fast_set_lds(size_t lds);
hipError_t step_many_mosi_set_lds(size_t lds);
hipError_t step_many_shl2_set_lds(size_t lds);
void launch_walk_many(bool pipe, bool rq, uint32_t blocks, uint32_t threads, const ManyPair* pairs, uint32_t live,
                      size_t lds, hipStream_t s, uint32_t L, int stage);
hipError_t walk_many_set_lds(size_t lds);

}  // namespace ggc
