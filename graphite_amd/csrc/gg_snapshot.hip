// gg_snapshot.hip — the packed sections of a coherent run's snapshot
// (gg_coherent_snapshot / _restore in gg_coherent.hip) on
// MI355X (gfx950).  The directory arrays are the bulk of a context's state
// and mostly never used; the sharer words of a never-used slot are not even
// initialised (gg_coh_dev.h, dfind).  So they leave the device as records
// {slot, entry, sharer words, Random word} of the slots in use, in slot order:
//   count    one workgroup per owned tile, 16-B entry loads, a wave sum
//   scan     exclusive over the tiles (one wave, DPP prefix)
//   pack     one workgroup per owned tile: ballot ranks inside a wave, the
//            waves' totals through LDS, so a tile's records keep slot order
// and come back by a scatter after the usual reset (unpack).  The miss-type
// address tables (~0 = empty) take the same three passes.
#include "gg_coh_dev.h"

namespace ggc {

constexpr uint32_t kSnapThreads = 256;

// slots [0, lim) of tile lt that a snapshot keeps
__device__ __forceinline__ uint32_t snap_limit(const PackSrc& s, uint32_t lt)
{
  return s.mode == PK_REP ? min(s.ts[lt].nrep, s.n) : s.n;
}
// PK_DIR: any field off its reset value {INV_ADDR, -1, UNCACHED, 0} (k_c_reset):
// an entry with a real address and no sharers holds its way, and a slot the
// engine opened had its sharer words zeroed then.  PK_REP: the live entries of
// the replaced list.  PK_TAB: an address-set slot that is not empty.
__device__ __forceinline__ bool snap_used(const PackSrc& s, uint32_t lt, uint32_t i, uint32_t lim)
{
  if (i >= lim) return false;
  if (s.mode == PK_REP) return true;
  const size_t g = (size_t)lt * s.n + i;
  if (s.mode == PK_TAB) return reinterpret_cast<const uint64_t*>(s.ent)[g] != ~0ull;
  const uint4 e = reinterpret_cast<const uint4*>(s.ent)[g];     // {addr lo, addr hi, owner, dstate | nsh << 16}
  return !(e.x == 0xFFFFFFFFu && e.y == 0xFFFFFFFFu && e.z == 0xFFFFFFFFu && e.w == 0u);
}

__global__ void __launch_bounds__(kSnapThreads) k_snap_count(PackSrc s, uint32_t* counts)
{
  __shared__ uint32_t tot;
  const uint32_t lt = blockIdx.x, tid = threadIdx.x;
  if (lt >= s.L) return;
  if (tid == 0) tot = 0;
  __syncthreads();
  const uint32_t lim = snap_limit(s, lt);
  uint32_t c = 0;
  for (uint32_t i = tid; i < lim; i += kSnapThreads) c += snap_used(s, lt, i, lim) ? 1u : 0u;
  c = wave_sum(c);
  if ((tid & 63) == 0 && c) atomicAdd(&tot, c);
  __syncthreads();
  if (tid == 0) counts[lt] = tot;
}

// base[lt] = records of the tiles before lt, base[L] = all (one wave)
__global__ void __launch_bounds__(64) k_snap_scan(const uint32_t* counts, uint32_t L, uint64_t* base)
{
  const uint32_t ln = threadIdx.x;
  uint64_t carry = 0;
  for (uint32_t c = 0; c < L; c += 64) {
    const uint32_t v = c + ln < L ? counts[c + ln] : 0u;
    const uint32_t ex = wave_excl_scan(v, ln);
    if (c + ln < L) base[c + ln] = carry + ex;
    carry += wave_sum(v);
  }
  if (ln == 0) base[L] = carry;
}

__global__ void __launch_bounds__(kSnapThreads) k_snap_pack(PackSrc s, const uint64_t* base, uint64_t cap, uint64_t* out)
{
  __shared__ uint32_t wt[kSnapThreads / 64];
  const uint32_t lt = blockIdx.x, tid = threadIdx.x, ln = tid & 63, wv = tid >> 6;
  if (lt >= s.L) return;
  const uint32_t lim = snap_limit(s, lt);
  const uint64_t b0 = base[lt];
  uint32_t run = 0;
  for (uint32_t c = 0; c < lim; c += kSnapThreads) {     // (uniform bounds: every thread takes every barrier)
    const uint32_t i = c + tid;
    const bool u = snap_used(s, lt, i, lim);
    const uint64_t m = __ballot(u);
    const uint32_t rank = (uint32_t)__popcll(m & ((1ull << ln) - 1ull));
    if (ln == 0) wt[wv] = (uint32_t)__popcll(m);
    __syncthreads();
    uint32_t pre = 0, all = 0;
#pragma unroll
    for (uint32_t w = 0; w < kSnapThreads / 64; ++w) { pre += w < wv ? wt[w] : 0u; all += wt[w]; }
    const uint64_t r = b0 + run + pre + rank;
    if (u && r < cap) {                                  // (cap = base[L] of the count pass: the state is at rest)
      const size_t g = (size_t)lt * s.n + i;
      uint64_t* o = out + r * s.rw;
      o[0] = g;
      if (s.mode == PK_TAB) o[1] = reinterpret_cast<const uint64_t*>(s.ent)[g];
      else {
        const uint4 e = reinterpret_cast<const uint4*>(s.ent)[g];
        o[1] = (uint64_t)e.x | ((uint64_t)e.y << 32);
        o[2] = (uint64_t)e.z | ((uint64_t)e.w << 32);
        for (uint32_t w = 0; w < s.W; ++w) o[3 + w] = s.sh[g * s.W + w];
        if (s.rng) o[3 + s.W] = s.rng[g];
      }
    }
    run += all;
    __syncthreads();
  }
}

// records back into their slots (after the run's reset); a slot index past
// the arrays is skipped (the host has checked them: defence in depth)
__global__ void __launch_bounds__(kSnapThreads) k_snap_unpack(PackSrc s, const uint64_t* recs, uint64_t n)
{
  const uint64_t r = (uint64_t)blockIdx.x * kSnapThreads + threadIdx.x;
  if (r >= n) return;
  const uint64_t* o = recs + r * s.rw;
  const uint64_t g = o[0];
  if (g >= (uint64_t)s.L * s.n) return;
  if (s.mode == PK_TAB) { reinterpret_cast<uint64_t*>(s.ent)[g] = o[1]; return; }
  reinterpret_cast<uint4*>(s.ent)[g] = make_uint4((uint32_t)o[1], (uint32_t)(o[1] >> 32), (uint32_t)o[2], (uint32_t)(o[2] >> 32));
  for (uint32_t w = 0; w < s.W; ++w) s.sh[g * s.W + w] = o[3 + w];
  if (s.rng) s.rng[g] = o[3 + s.W];
}

hipError_t snap_count(const PackSrc& s, uint32_t* counts, uint64_t* base, hipStream_t st)
{
  hipLaunchKernelGGL(k_snap_count, dim3(s.L), dim3(kSnapThreads), 0, st, s, counts);
  hipLaunchKernelGGL(k_snap_scan, dim3(1), dim3(64), 0, st, (const uint32_t*)counts, s.L, base);
  return hipGetLastError();
}
hipError_t snap_pack(const PackSrc& s, const uint64_t* base, uint64_t cap, uint64_t* out, hipStream_t st)
{
  hipLaunchKernelGGL(k_snap_pack, dim3(s.L), dim3(kSnapThreads), 0, st, s, base, cap, out);
  return hipGetLastError();
}
hipError_t snap_unpack(const PackSrc& s, const uint64_t* recs, uint64_t n, hipStream_t st)
{
  if (n == 0) return hipSuccess;
  hipLaunchKernelGGL(k_snap_unpack, dim3((uint32_t)((n + kSnapThreads - 1) / kSnapThreads)), dim3(kSnapThreads), 0, st, s,
                     recs, n);
  return hipGetLastError();
}

}  // namespace ggc
