// gg_noc_stage.h — pieces the staged NoC kernels share (gg_noc.hip: the mesh
// stages; gg_noc_atac.hip: the ATAC port and receive stages): the (time,
// index) sort key, the in-workgroup sorts and the bucket scan / fill kernels.
#ifndef GG_NOC_STAGE_H
#define GG_NOC_STAGE_H
#include "gg_dev.h"

namespace {
using namespace gg;

constexpr uint32_t kQMaxNoc = 128;                // history-tree intervals a RegQueue holds
struct SK { uint64_t t; uint32_t i, pad; };
static_assert(sizeof(SK) == 16, "16-byte sort keys");
__device__ __forceinline__ bool sk_lt(const SK& a, const SK& b) { return a.t < b.t || (a.t == b.t && a.i < b.i); }
__device__ __forceinline__ void nsync()   // LDS ordering between the lanes of one wave of a multi-wave workgroup
{
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
}
__device__ __forceinline__ uint64_t wave_sum64n(uint64_t v)
{
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += (uint64_t)__shfl_xor((long long)v, o);
  return v;
}

// ascending bitonic sort of a[0, M), M a power of two, all threads of the block
template <class T, class Lt>
__device__ void block_bitonic(T* a, uint32_t M, Lt lt)
{
  for (uint32_t k = 2; k <= M; k <<= 1)
    for (uint32_t j = k >> 1; j > 0; j >>= 1) {
      for (uint32_t i = threadIdx.x; i < M; i += blockDim.x) {
        const uint32_t l = i ^ j;
        if (l > i) {
          const T x = a[i], y = a[l];
          if (((i & k) == 0) == lt(y, x)) { a[i] = y; a[l] = x; }
        }
      }
      __syncthreads();
    }
}

__device__ __forceinline__ uint64_t batch_n(uint64_t n, const uint32_t* n_dev) { return n_dev ? min((uint64_t)*n_dev, n) : n; }

// (the bodies are shared with the ensemble launches of gg_noc_many.hip)
__device__ __forceinline__ void scan_counts_body(const uint32_t* counts, uint32_t nb, uint64_t* off, uint32_t* cursor)
{
  // single block; nb is small (<= 2 * 4096)
  __shared__ uint64_t part[1024];
  const uint32_t t = threadIdx.x, per = (nb + blockDim.x - 1) / blockDim.x;
  uint64_t s = 0;
  for (uint32_t i = t * per; i < min(nb, (t + 1) * per); ++i) s += counts[i];
  part[t] = s;
  __syncthreads();
  if (t == 0) { uint64_t a = 0; for (uint32_t i = 0; i < blockDim.x; ++i) { uint64_t v = part[i]; part[i] = a; a += v; } off[nb] = a; }
  __syncthreads();
  uint64_t a = part[t];
  for (uint32_t i = t * per; i < min(nb, (t + 1) * per); ++i) { off[i] = a; cursor[i] = 0; a += counts[i]; }
}
__global__ void k_scan_counts(const uint32_t* counts, uint32_t nb, uint64_t* off, uint32_t* cursor)
{
  scan_counts_body(counts, nb, off, cursor);
}

__device__ __forceinline__ void bucket_body(const uint32_t* __restrict__ keys, uint64_t cap, const uint32_t* n_dev,
                                            const uint64_t* __restrict__ off, uint32_t* cursor, uint32_t* ids, uint64_t k)
{
  const uint64_t n = batch_n(cap, n_dev);
  if (k >= n) return;
  const uint32_t key = keys[k];
  if (key == ~0u) return;
  ids[off[key] + atomicAdd(&cursor[key], 1u)] = (uint32_t)k;
}
__global__ void k_bucket(const uint32_t* __restrict__ keys, uint64_t cap, const uint32_t* n_dev,
                         const uint64_t* __restrict__ off, uint32_t* cursor, uint32_t* ids)
{
  bucket_body(keys, cap, n_dev, off, cursor, ids, (uint64_t)blockIdx.x * blockDim.x + threadIdx.x);
}

}  // namespace
#endif
