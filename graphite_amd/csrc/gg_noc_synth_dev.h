// gg_noc_synth_dev.h — the device bodies of the synthetic-traffic kernels
// (gg_noc_synth.hip: one context; gg_noc_many.hip: an ensemble).
#ifndef GG_NOC_SYNTH_DEV_H
#define GG_NOC_SYNTH_DEV_H
#include "gg_noc_many.h"

namespace {

constexpr uint64_t kMix = 0x9E3779B97F4A7C15ull;
constexpr uint64_t kStopCycle = (1ull << 32) - 64;       // a tile gives up here (never reached inside the host's bounds)
constexpr int kGenWaves = 4;                             // tiles (waves) per generator workgroup
constexpr int kRedThreads = 256, kRedWaves = kRedThreads / GG_WAVE;
constexpr uint32_t kRedMaxBlocks = 1024;
constexpr int kRedSums = 7;                              // GG_NLS_PACKETS .. GG_NLS_LAST_ARRIVAL_PS

typedef gg_synth_plan synth_plan;

__host__ __device__ inline uint64_t splitmix64_at(uint64_t seed, uint64_t i)
{
  uint64_t z = seed + (i + 1) * kMix;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

// The single destination of a tile under the five fixed patterns
// (synthetic_network.cc:288-341; positions and ids: :350-359).
__host__ __device__ inline uint32_t fixed_destination(uint32_t pattern, uint32_t t, uint32_t T, uint32_t w, uint32_t h)
{
  const uint32_t sx = t % w, sy = t / w;
  switch (pattern) {
    case GG_TP_BIT_COMPLEMENT: return ~t & (T - 1);
    case GG_TP_SHUFFLE: {
      if (T < 2) return 0;
      uint32_t nbits = 0;
      while (T >> (nbits + 1)) ++nbits;                                           // floorLog2(T)
      return ((t >> (nbits - 1)) & 1u) | ((t << 1) & (T - 1));
    }
    case GG_TP_TRANSPOSE: return sx * w + sy;
    case GG_TP_TORNADO: return ((sy + h / 2) % h) * w + (sx + w / 2) % w;
    default: return ((sy + 1) % h) * w + (sx + 1) % w;                            // GG_TP_NEAREST_NEIGHBOR
  }
}

// One wave per tile, 64 cycles a round: lane l decides cycle base + l, the
// ballot of the decisions gives every sending lane its packet ordinal.  The
// loop state (base, count) is the same in every lane.  blk: the block's index
// in its instance's grid; orbit: uniform_random's 2T-entry table; P.aux: the
// stop flag.
__device__ __forceinline__ void synth_generate_body(const synth_plan& P, const uint32_t* orbit, uint32_t blk)
{
  const uint32_t lane = threadIdx.x & (GG_WAVE - 1);
  const uint32_t t = __builtin_amdgcn_readfirstlane(blk * kGenWaves + (threadIdx.x >> 6));
  if (t >= P.T) return;
  const uint64_t tile_seed = splitmix64_at(P.seed, t);
  const uint32_t fixed = P.pattern == GG_TP_UNIFORM_RANDOM ? 0u : fixed_destination(P.pattern, t, P.T, P.w, P.h);
  const uint64_t below = (1ull << lane) - 1;
  const uint64_t out0 = (uint64_t)t * P.N;
  uint64_t count = 0;
  for (uint64_t base = 0;; base += GG_WAVE) {
    if (base >= kStopCycle) {
      if (lane == 0) atomicOr(P.aux, 1u);
      break;
    }
    const uint64_t c = base + lane;
    const bool send = (splitmix64_at(tile_seed, c) >> 11) < P.thr;
    const uint64_t mask = __ballot(send);
    const uint64_t ord = count + (uint64_t)__popcll(mask & below);
    if (send && ord < P.N) {
      const uint64_t o = out0 + ord;
      P.src[o] = t;
      P.dst[o] = P.pattern == GG_TP_UNIFORM_RANDOM ? orbit[(uint32_t)ord % P.T + t] : fixed;   // (ord < N < 2^32)
      P.len[o] = P.bits;
      P.time[o] = c * P.cycle_ps;
      if (ord == P.N - 1 && P.last_cycle) P.last_cycle[t] = c;
    }
    count += (uint64_t)__popcll(mask);
    if (count >= P.N) break;
  }
}

__device__ inline uint64_t wave_sum(uint64_t v)
{
  for (int d = GG_WAVE / 2; d; d >>= 1) v += (uint64_t)__shfl_xor((unsigned long long)v, d, GG_WAVE);
  return v;
}
__device__ inline uint64_t wave_max(uint64_t v)
{
  for (int d = GG_WAVE / 2; d; d >>= 1) {
    const uint64_t o = (uint64_t)__shfl_xor((unsigned long long)v, d, GG_WAVE);
    v = o > v ? o : v;
  }
  return v;
}

// One pass over a routed batch.  Each lane keeps its sums and maxima in
// registers; a wave adds its histogram bins to LDS once per distinct bin; the
// workgroup's totals go to `red` with one 64-bit atomic per word.  The batch is
// strided over nblk blocks of kRedThreads, this one being blk (every word is a
// sum or a maximum of integers: any nblk gives the same words).
__device__ __forceinline__ void noc_latency_stats_body(const uint32_t* __restrict__ src,
    const uint32_t* __restrict__ dst, const uint64_t* __restrict__ time, const uint64_t* __restrict__ arr,
    const uint64_t* __restrict__ zl, const uint64_t* __restrict__ ct, uint64_t n, unsigned long long* red,
    uint32_t blk, uint32_t nblk)
{
  __shared__ uint32_t hist[65];
  __shared__ uint64_t part[kRedWaves][kRedSums];
  const uint32_t lane = threadIdx.x & (GG_WAVE - 1);
  const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  if (threadIdx.x < 65) hist[threadIdx.x] = 0;
  __syncthreads();
  uint64_t acc[kRedSums] = {0, 0, 0, 0, 0, 0, 0};
  const uint64_t stride = (uint64_t)nblk * kRedThreads;
  for (uint64_t base = (uint64_t)blk * kRedThreads + wave * GG_WAVE; base < n; base += stride) {
    const uint64_t i = base + lane;
    bool counted = false;
    uint32_t bin = 0;
    if (i < n) {
      if (src[i] == dst[i]) {
        acc[GG_NLS_SELF_PACKETS] += 1;
      } else {
        const uint64_t a = arr[i], lat = a - time[i];
        counted = true;
        bin = lat ? 64u - (uint32_t)__clzll((long long)lat) : 0u;
        acc[GG_NLS_PACKETS] += 1;
        acc[GG_NLS_LATENCY_PS] += lat;
        acc[GG_NLS_ZERO_LOAD_PS] += zl[i];
        acc[GG_NLS_CONTENTION_PS] += ct[i];
        acc[GG_NLS_MAX_LATENCY_PS] = lat > acc[GG_NLS_MAX_LATENCY_PS] ? lat : acc[GG_NLS_MAX_LATENCY_PS];
        acc[GG_NLS_LAST_ARRIVAL_PS] = a > acc[GG_NLS_LAST_ARRIVAL_PS] ? a : acc[GG_NLS_LAST_ARRIVAL_PS];
      }
    }
    uint64_t todo = __ballot(counted);
    while (todo) {                                     // one round per distinct bin of the wave
      const int leader = __ffsll((unsigned long long)todo) - 1;
      const uint32_t b = (uint32_t)__builtin_amdgcn_readlane((int)bin, leader);
      const uint64_t same = __ballot(counted && bin == b);
      if (lane == (uint32_t)leader) atomicAdd(&hist[b], (uint32_t)__popcll(same));
      todo &= ~same;
    }
  }
  for (int k = 0; k < kRedSums; ++k) {
    const uint64_t v = (k == GG_NLS_MAX_LATENCY_PS || k == GG_NLS_LAST_ARRIVAL_PS) ? wave_max(acc[k]) : wave_sum(acc[k]);
    if (lane == 0) part[wave][k] = v;
  }
  __syncthreads();
  if (threadIdx.x < kRedSums) {
    const int k = (int)threadIdx.x;
    const bool is_max = k == GG_NLS_MAX_LATENCY_PS || k == GG_NLS_LAST_ARRIVAL_PS;
    uint64_t v = part[0][k];
    for (int w = 1; w < kRedWaves; ++w) v = is_max ? (part[w][k] > v ? part[w][k] : v) : v + part[w][k];
    if (v) {
      if (is_max) atomicMax(&red[k], (unsigned long long)v);
      else atomicAdd(&red[k], (unsigned long long)v);
    }
  }
  if (threadIdx.x >= GG_WAVE && threadIdx.x < GG_WAVE + 65 && hist[threadIdx.x - GG_WAVE])
    atomicAdd(&red[GG_NLS_HIST + threadIdx.x - GG_WAVE], (unsigned long long)hist[threadIdx.x - GG_WAVE]);
}

// blocks of the reduction over n packets
inline uint32_t noc_stats_blocks(uint64_t n)
{
  const uint64_t blocks = (n + kRedThreads - 1) / kRedThreads;
  return (uint32_t)(blocks < kRedMaxBlocks ? blocks : kRedMaxBlocks);
}

}  // namespace
#endif
