// gg_mem_synth.hip — synthetic memory traffic on the device:
// the instruction stream of the reference's coherent-memory benchmark
// (tests/benchmarks/synthetic_memory/synthetic_memory.cc:135-399) as a
// gg_trace, the one-pass reduction over a coherent run's access words, and the
// driver that chains generator -> gg_coherent_run -> reduction on a context.
//
// A tile's stream is cut into chunks of kChunk instructions, one wave each:
// drand48_r is an affine map mod 2^48, so the state at any position is reached
// in O(log k) steps (lcg_pow).  A count pass gives every chunk its six type
// counts; a scan on the host turns them into the chunk's record offset, its
// ranks in the tile's two address streams, its private-access count and the
// gap carried in; the fill pass writes the records.
#include <math.h>
#include <stdlib.h>

#include <algorithm>

#include "gg_internal.h"
#include "gg_noc_synth_dev.h"              // wave_sum / wave_max and the reduction's launch shape

namespace {

constexpr uint64_t kLcgA = 0x5DEECE66Dull, kLcgC = 0xBull, kMask48 = (1ull << 48) - 1;   // drand48_r
constexpr uint32_t kChunkRounds = 16;                        // 64-instruction rounds of a chunk
constexpr uint32_t kChunk = kChunkRounds * GG_WAVE;          // 1024 instructions: 10 chunks a tile at input.64
constexpr int kMemWaves = 4;                                 // chunks (waves) per workgroup
constexpr uint32_t kMaxList = 32768;                         // synthetic_memory.cc:375, :385
constexpr int kMlsSums = 10;                                 // GG_MLS_RECORDS .. GG_MLS_MAX_LATENCY_PS
constexpr unsigned long long kNoErr = ~0ull;

struct lcg_jump { uint64_t a, c; };                          // X -> a X + c, k steps at once

// (A_k, C_k): k steps of X' = a X + c composed by squaring.  The arithmetic is
// mod 2^64 and 2^48 divides it, so masking at the end is enough.
__host__ __device__ inline lcg_jump lcg_pow(uint64_t k)
{
  uint64_t A = 1, C = 0, sa = kLcgA, sc = kLcgC;
  while (k) {
    if (k & 1) { A = A * sa; C = C * sa + sc; }
    sc = (sa + 1) * sc;
    sa = sa * sa;
    k >>= 1;
  }
  return {A & kMask48, C & kMask48};
}
__host__ __device__ inline uint64_t lcg_apply(lcg_jump j, uint64_t x) { return (j.a * x + j.c) & kMask48; }
// srand48_r keeps the low 32 bits of its seed
__host__ __device__ inline uint64_t lcg_seed(uint64_t seed) { return ((seed & 0xFFFFFFFFull) << 16) | 0x330Eull; }

struct chunk_start {
  uint64_t rec;                            // first record of the chunk
  uint32_t ro, rw;                         // draws of the tile's read-only / read-write stream before it
  uint32_t priv;                           // private accesses of the tile before it
  uint32_t carry;                          // NON_MEMORY instructions since the tile's last access
};
enum { kCntAny = 6, kCntTrail = 7, kCntWords = 8 };          // a chunk's count words: six types, has an access, trailing NON_MEMORY

struct mem_plan {
  uint64_t N, seed_base, cap;
  uint64_t thr[GG_NUM_MEM_INS_TYPES];      // least X whose (float)(X 2^-48) >= cum[i] (2^48: none)
  uint32_t T, chunks;                      // chunks per tile
  uint32_t log_line, log_shared, num_private;
  const uint32_t* off;                     // [2][T + 1]: the tile's read-only, then read-write list in `lists`
  const uint64_t* lists;
  uint32_t* counts;                        // [T * chunks][kCntWords], the count pass's result
  unsigned long long* err;                 // lowest (tile << 32 | instruction) whose draw names no type
  const chunk_start* starts;               // [T * chunks], the scan's result
  uint64_t* addr;
  uint32_t* meta;
};

__device__ __forceinline__ uint64_t readlane64(uint64_t v, uint32_t l)
{
  const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)v, (int)l);
  const uint32_t hi = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(v >> 32), (int)l);
  return ((uint64_t)hi << 32) | lo;
}

// Float rounding is monotone, so the first i with (float)u < cum[i] is the
// number of thresholds at or below X; GG_NUM_MEM_INS_TYPES: none (the reference asserts).
__device__ __forceinline__ uint32_t ins_type(const mem_plan& P, uint64_t X)
{
  uint32_t ty = 0;
#pragma unroll
  for (int i = 0; i < GG_NUM_MEM_INS_TYPES; ++i) ty += X >= P.thr[i] ? 1u : 0u;
  return ty;
}

// What both passes share: the wave's chunk, the lane's jump constants and the
// type stream's state at the chunk's first instruction.
struct chunk_ctx {
  uint32_t lane, w, t;
  uint64_t first, end, X0, Xb;
  lcg_jump J;                              // lane l: l + 1 steps
  uint32_t ro_n, rw_n;
};
__device__ __forceinline__ bool chunk_begin(const mem_plan& P, chunk_ctx& c)
{
  c.lane = threadIdx.x & (GG_WAVE - 1);
  c.w = __builtin_amdgcn_readfirstlane(blockIdx.x * kMemWaves + (threadIdx.x >> 6));
  if (c.w >= P.T * P.chunks) return false;
  c.t = c.w / P.chunks;
  c.first = (uint64_t)(c.w % P.chunks) * kChunk;
  c.end = c.first + kChunk < P.N ? c.first + kChunk : P.N;
  c.J = lcg_pow(c.lane + 1);
  c.X0 = lcg_seed(P.seed_base + c.t);
  c.Xb = lcg_apply(lcg_pow(c.first), c.X0);
  c.ro_n = P.off[c.t + 1] - P.off[c.t];
  c.rw_n = P.off[P.T + 1 + c.t + 1] - P.off[P.T + 1 + c.t];
  return true;
}

// Count pass: one wave per chunk, 64 instructions a round.
__global__ __launch_bounds__(kMemWaves* GG_WAVE) void k_mem_count(mem_plan P)
{
  chunk_ctx c;
  if (!chunk_begin(P, c)) return;
  uint32_t cnt[GG_NUM_MEM_INS_TYPES] = {0, 0, 0, 0, 0, 0};
  uint32_t trail = 0, any = 0;
  for (uint64_t pos = c.first; pos < c.end; pos += GG_WAVE) {
    const uint64_t X = lcg_apply(c.J, c.Xb);
    const bool valid = pos + c.lane < c.end;
    const uint32_t ty = valid ? ins_type(P, X) : GG_NUM_MEM_INS_TYPES + 1;
    if (ty == GG_NUM_MEM_INS_TYPES) atomicMin(P.err, ((unsigned long long)c.t << 32) | (pos + c.lane));
    uint64_t m[GG_NUM_MEM_INS_TYPES];
#pragma unroll
    for (int i = 0; i < GG_NUM_MEM_INS_TYPES; ++i) {
      m[i] = __ballot(ty == (uint32_t)i);
      cnt[i] += (uint32_t)__popcll(m[i]);
    }
    const uint64_t acc = (c.ro_n ? m[1] : 0) | (c.rw_n ? m[2] | m[3] : 0) | m[4] | m[5];
    if (acc) {
      const int hi = 63 - __clzll((long long)acc);
      any = 1;
      trail = (uint32_t)__popcll(m[0] & ~((2ull << hi) - 1));
    } else {
      trail += (uint32_t)__popcll(m[0]);
    }
    c.Xb = readlane64(X, GG_WAVE - 1);
  }
  if (c.lane == 0) {
    uint32_t* o = P.counts + (uint64_t)c.w * kCntWords;
#pragma unroll
    for (int i = 0; i < GG_NUM_MEM_INS_TYPES; ++i) o[i] = cnt[i];
    o[kCntAny] = any;
    o[kCntTrail] = trail;
  }
}

// Fill pass.  The state of the two address streams is the same in every lane:
// a lane's draw is the stream's state advanced by its rank among the round's
// lanes of that stream, with the constants of the lane that holds that jump.
__global__ __launch_bounds__(kMemWaves* GG_WAVE) void k_mem_fill(mem_plan P)
{
  chunk_ctx c;
  if (!chunk_begin(P, c)) return;
  const chunk_start cs = P.starts[c.w];
  uint64_t rec = cs.rec;
  uint32_t carry = cs.carry, priv = cs.priv;
  uint64_t Gro = lcg_apply(lcg_pow(cs.ro), c.X0), Grw = lcg_apply(lcg_pow(cs.rw), c.X0);
  const uint64_t below = (1ull << c.lane) - 1;
  const uint64_t* ro_list = P.lists + P.off[c.t];
  const uint64_t* rw_list = P.lists + P.off[P.T + 1 + c.t];
  const uint64_t priv_base = (1ull << (P.log_shared + P.log_line));
  for (uint64_t pos = c.first; pos < c.end; pos += GG_WAVE) {
    const uint64_t X = lcg_apply(c.J, c.Xb);
    const bool valid = pos + c.lane < c.end;
    const uint32_t ty = valid ? ins_type(P, X) : GG_NUM_MEM_INS_TYPES + 1;
    const uint64_t m0 = __ballot(ty == GG_MI_NON_MEMORY);
    const uint64_t m1 = __ballot(ty == GG_MI_RD_ONLY_SHARED_READ && c.ro_n);
    const uint64_t m23 = __ballot((ty == GG_MI_RD_WR_SHARED_READ || ty == GG_MI_RD_WR_SHARED_WRITE) && c.rw_n);
    const uint64_t m45 = __ballot(ty == GG_MI_PRIVATE_READ || ty == GG_MI_PRIVATE_WRITE);
    const uint64_t acc = m1 | m23 | m45;
    uint64_t a = 0;
    if (m1) {                              // (wave-uniform: every lane takes part in the shuffles)
      const int j = __popcll(m1 & below);
      const lcg_jump Jj = {(uint64_t)__shfl((unsigned long long)c.J.a, j, GG_WAVE),
                           (uint64_t)__shfl((unsigned long long)c.J.c, j, GG_WAVE)};
      const uint64_t G = lcg_apply(Jj, Gro);
      // Random<int>::next: (int)(u * size) in double, as the reference computes it
      uint32_t idx = (uint32_t)(int)((double)G * 0x1p-48 * (double)c.ro_n);
      idx = idx < c.ro_n ? idx : c.ro_n - 1;                 // (u < 1: never taken; keeps the load inside the list)
      if ((m1 >> c.lane) & 1) a = ro_list[idx];
      const uint32_t n = (uint32_t)__popcll(m1);
      Gro = lcg_apply(lcg_jump{readlane64(c.J.a, n - 1), readlane64(c.J.c, n - 1)}, Gro);
    }
    if (m23) {
      const int j = __popcll(m23 & below);
      const lcg_jump Jj = {(uint64_t)__shfl((unsigned long long)c.J.a, j, GG_WAVE),
                           (uint64_t)__shfl((unsigned long long)c.J.c, j, GG_WAVE)};
      const uint64_t G = lcg_apply(Jj, Grw);
      uint32_t idx = (uint32_t)(int)((double)G * 0x1p-48 * (double)c.rw_n);
      idx = idx < c.rw_n ? idx : c.rw_n - 1;
      if ((m23 >> c.lane) & 1) a = rw_list[idx];
      const uint32_t n = (uint32_t)__popcll(m23);
      Grw = lcg_apply(lcg_jump{readlane64(c.J.a, n - 1), readlane64(c.J.c, n - 1)}, Grw);
    }
    if ((m45 >> c.lane) & 1) {
      const uint32_t k = (priv + (uint32_t)__popcll(m45 & below)) & (P.num_private - 1);
      a = priv_base + (((uint64_t)c.t * P.num_private + k) << P.log_line);
    }
    priv += (uint32_t)__popcll(m45);
    if ((acc >> c.lane) & 1) {
      const uint64_t prev = acc & below;
      uint32_t gap;
      if (prev) {
        const int hi = 63 - __clzll((long long)prev);
        gap = (uint32_t)__popcll(m0 & below & ~((2ull << hi) - 1));
      } else {
        gap = carry + (uint32_t)__popcll(m0 & below);
      }
      const uint64_t r = rec + (uint64_t)__popcll(prev);
      if (r < P.cap) {
        const bool wr = ty == GG_MI_RD_WR_SHARED_WRITE || ty == GG_MI_PRIVATE_WRITE;
        P.addr[r] = a;
        P.meta[r] = (gap << 1) | (wr ? GG_META_WRITE : 0u);
      }
    }
    if (acc) {
      const int hi = 63 - __clzll((long long)acc);
      carry = (uint32_t)__popcll(m0 & ~((2ull << hi) - 1));
      rec += (uint64_t)__popcll(acc);
    } else {
      carry += (uint32_t)__popcll(m0);
    }
    c.Xb = readlane64(X, GG_WAVE - 1);
  }
}

// One pass over a run's access words, after k_noc_latency_stats: sums and the
// maximum in registers, the histogram in LDS once per distinct bin of a wave,
// one 64-bit atomic per word and workgroup at the end.
__global__ __launch_bounds__(kRedThreads) void k_mem_access_stats(const uint32_t* __restrict__ meta,
    const uint64_t* __restrict__ out, uint64_t n, unsigned long long* red)
{
  __shared__ uint32_t hist[65];
  __shared__ uint64_t part[kRedWaves][kMlsSums];
  const uint32_t lane = threadIdx.x & (GG_WAVE - 1);
  const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  if (threadIdx.x < 65) hist[threadIdx.x] = 0;
  __syncthreads();
  uint64_t acc[kMlsSums] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
  const uint64_t stride = (uint64_t)gridDim.x * kRedThreads;
  for (uint64_t base = (uint64_t)blockIdx.x * kRedThreads + wave * GG_WAVE; base < n; base += stride) {
    const uint64_t i = base + lane;
    bool counted = false;
    uint32_t bin = 0;
    if (i < n) {
      const uint32_t m = meta[i];
      if (m != GG_META_BARRIER) {
        const uint64_t wd = out[i], lat = wd >> 2;
        const uint32_t lvl = (uint32_t)(wd & 3);
        counted = true;
        bin = lat ? 64u - (uint32_t)__clzll((long long)lat) : 0u;
        acc[GG_MLS_RECORDS] += 1;
        acc[(m & GG_META_WRITE) ? GG_MLS_WRITES : GG_MLS_READS] += 1;
        if (lvl == GG_LVL_L1) { acc[GG_MLS_L1_HITS] += 1; acc[GG_MLS_L1_LATENCY_PS] += lat; }
        if (lvl == GG_LVL_L2) { acc[GG_MLS_L2_HITS] += 1; acc[GG_MLS_L2_LATENCY_PS] += lat; }
        if (lvl == GG_LVL_DIR) { acc[GG_MLS_L2_MISSES] += 1; acc[GG_MLS_L2_MISS_LATENCY_PS] += lat; }
        acc[GG_MLS_MAX_LATENCY_PS] = lat > acc[GG_MLS_MAX_LATENCY_PS] ? lat : acc[GG_MLS_MAX_LATENCY_PS];
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
#pragma unroll
  for (int k = 0; k < kMlsSums; ++k) {
    const uint64_t v = k == GG_MLS_MAX_LATENCY_PS ? wave_max(acc[k]) : wave_sum(acc[k]);
    if (lane == 0) part[wave][k] = v;
  }
  __syncthreads();
  if (threadIdx.x < kMlsSums) {
    const int k = (int)threadIdx.x;
    const bool is_max = k == GG_MLS_MAX_LATENCY_PS;
    uint64_t v = part[0][k];
    for (int w = 1; w < kRedWaves; ++w) v = is_max ? (part[w][k] > v ? part[w][k] : v) : v + part[w][k];
    if (v) {
      if (is_max) atomicMax(&red[k], (unsigned long long)v);
      else atomicAdd(&red[k], (unsigned long long)v);
    }
  }
  if (threadIdx.x >= GG_WAVE && threadIdx.x < GG_WAVE + 65 && hist[threadIdx.x - GG_WAVE])
    atomicAdd(&red[GG_MLS_HIST + threadIdx.x - GG_WAVE], (unsigned long long)hist[threadIdx.x - GG_WAVE]);
}

bool is_pow2(uint64_t x) { return x && !(x & (x - 1)); }
uint32_t log2u(uint64_t x) { uint32_t l = 0; while (x >> (l + 1)) ++l; return l; }

// The least X in [0, 2^48] whose (float)(X 2^-48) >= c (2^48: no draw reaches c).
uint64_t type_threshold(float c)
{
  uint64_t lo = 0, hi = 1ull << 48;
  while (lo < hi) {
    const uint64_t mid = lo + (hi - lo) / 2;
    if ((float)((double)mid * 0x1p-48) >= c) hi = mid; else lo = mid + 1;
  }
  return lo;
}

// What a plan leaves on the host.
struct mem_host {
  std::vector<uint32_t> off;               // [2][T + 1]
  std::vector<uint64_t> lists;
  std::vector<uint64_t> tile_offsets, tails, type_counts;
  std::vector<chunk_start> starts;
};
// Device scratch of the two passes.
struct mem_bufs {
  gg_dbuf<uint32_t> off, counts;
  gg_dbuf<uint64_t> lists;
  gg_dbuf<chunk_start> starts;
  gg_dbuf<unsigned long long> err;
};

// The checks that need no device, the thresholds and the address map.
gg_status mem_prepare(const gg_mem_traffic_params* p, uint32_t T, uint32_t line, mem_plan* P, mem_host* H)
{
  const char* who = "gg_gen_memory_traffic";
  if (!p) return gg_fail(GG_ERR_INVALID, "%s: params NULL", who);
  if (T == 0) return gg_fail(GG_ERR_INVALID, "%s: no tiles", who);
  if (p->num_threads && p->num_threads != T)
    return gg_fail(GG_ERR_INVALID, "%s: num_threads %u on %u tiles", who, p->num_threads, T);
  if (!is_pow2(line)) return gg_fail(GG_ERR_INVALID, "%s: line of %u bytes is no power of two", who, line);
  if (!is_pow2(p->num_shared_addresses))
    return gg_fail(GG_ERR_INVALID, "%s: num_shared_addresses %u is no power of two", who, p->num_shared_addresses);
  if (p->num_private_addresses && !is_pow2(p->num_private_addresses))
    return gg_fail(GG_ERR_INVALID, "%s: num_private_addresses %u is no power of two", who, p->num_private_addresses);
  if (p->degree_of_sharing > T)
    return gg_fail(GG_ERR_INVALID, "%s: degree_of_sharing %u beyond %u tiles", who, p->degree_of_sharing, T);
  for (int i = 0; i < GG_NUM_MEM_INS_TYPES; ++i)
    if (!(p->probability[i] >= 0.0f && p->probability[i] <= 1.0f))
      return gg_fail(GG_ERR_INVALID, "%s: probability[%d] = %g outside [0, 1]", who, i, (double)p->probability[i]);
  if (!p->num_private_addresses && p->probability[GG_MI_PRIVATE_READ] + p->probability[GG_MI_PRIVATE_WRITE] > 0.0f)
    return gg_fail(GG_ERR_INVALID, "%s: private accesses with num_private_addresses 0", who);
  if (p->instructions_per_tile == 0) return gg_fail(GG_ERR_INVALID, "%s: no instructions per tile", who);
  const uint32_t log_line = log2u(line), log_shared = log2u(p->num_shared_addresses);
  if (log_shared + log_line > 30)
    return gg_fail(GG_ERR_RANGE, "%s: %u shared lines of %u bytes: the private base 1 << %u is beyond an int", who,
                   p->num_shared_addresses, line, log_shared + log_line);
  if ((uint64_t)T * p->num_private_addresses >= (1ull << 31))
    return gg_fail(GG_ERR_RANGE, "%s: %u tiles x %u private lines is beyond 2^31 - 1", who, T, p->num_private_addresses);
  if (p->instructions_per_tile >= (1ull << 31))
    return gg_fail(GG_ERR_RANGE, "%s: %llu instructions per tile is beyond 2^31 - 1", who,
                   (unsigned long long)p->instructions_per_tile);
  const uint64_t entries = (uint64_t)p->num_shared_addresses * p->degree_of_sharing;
  if (entries >= (1ull << 31))
    return gg_fail(GG_ERR_RANGE, "%s: an address map of %llu entries is beyond 2^31 - 1", who, (unsigned long long)entries);

  // synthetic_memory.cc:266-272, float arithmetic in the reference's order
  const float* pr = p->probability;
  const float den = pr[1] + pr[2] + pr[3];
  const float frac_ro = den > 0.0f ? pr[1] / den : 0.0f;
  float cum[GG_NUM_MEM_INS_TYPES];
  cum[0] = pr[0];
  for (int i = 1; i < GG_NUM_MEM_INS_TYPES; ++i) cum[i] = pr[i] + cum[i - 1];
  for (int i = 0; i < GG_NUM_MEM_INS_TYPES; ++i) P->thr[i] = type_threshold(cum[i]);
  P->N = p->instructions_per_tile;
  P->seed_base = p->seed_base;
  P->T = T;
  P->chunks = (uint32_t)((P->N + kChunk - 1) / kChunk);
  P->log_line = log_line;
  P->log_shared = log_shared;
  P->num_private = p->num_private_addresses;

  // computeSharedAddressToThreadMapping (:314-334) on a random_r state of its own
  // (128 bytes: the TYPE_3 generator that srandom seeds)
  char statebuf[128] = {0};
  struct random_data rd = {};
  initstate_r(p->map_seed, statebuf, sizeof(statebuf), &rd);
  const int32_t ro_lines = (int32_t)(frac_ro * (float)(int32_t)p->num_shared_addresses);
  std::vector<uint32_t> tid(entries);
  std::vector<uint32_t>& off = H->off;
  off.assign(2 * ((size_t)T + 1), 0);
  uint64_t e = 0;
  for (uint32_t i = 0; i < p->num_shared_addresses; ++i) {
    const bool ro = (int32_t)i < ro_lines;
    for (uint32_t j = 0; j < p->degree_of_sharing; ++j, ++e) {
      int32_t r = 0;
      random_r(&rd, &r);
      const float q = ((float)r) / (float)RAND_MAX;
      const int32_t t = (int32_t)(q * (float)(int32_t)T);
      if (t < 0 || (uint32_t)t >= T)
        return gg_fail(GG_ERR_STATE, "%s: map draw %llu (line %u) names tile %d of %u (the reference indexes out of range)",
                       who, (unsigned long long)e, i, t, T);
      tid[e] = (uint32_t)t;
      ++off[(ro ? 0 : T + 1) + (size_t)t + 1];
    }
  }
  // CSR: read-only lists of all tiles, then read-write lists; push order kept
  uint32_t run = 0;
  for (size_t k = 0; k < off.size(); ++k) {
    if (k == (size_t)T + 1) { off[k] = run; continue; }      // (the read-write block's first offset)
    if (k == 0) continue;
    run += off[k];
    off[k] = run;
  }
  H->lists.assign(entries ? entries : 1, 0);
  std::vector<uint32_t> at(off);
  e = 0;
  for (uint32_t i = 0; i < p->num_shared_addresses; ++i) {
    const bool ro = (int32_t)i < ro_lines;
    for (uint32_t j = 0; j < p->degree_of_sharing; ++j, ++e)
      H->lists[at[(ro ? 0 : T + 1) + (size_t)tid[e]]++] = (uint64_t)i << log_line;
  }
  return GG_OK;
}

// Upload, count pass, scan.  Synchronizes the stream.
gg_status mem_plan_launch(mem_plan& P, mem_host& H, mem_bufs& B, hipStream_t s)
{
  const char* who = "gg_gen_memory_traffic";
  const uint32_t T = P.T;
  const uint64_t W = (uint64_t)T * P.chunks;
  if (gg_status st = B.off.reserve(H.off.size())) return st;
  if (gg_status st = B.lists.reserve(H.lists.size())) return st;
  if (gg_status st = B.counts.reserve(W * kCntWords)) return st;
  if (gg_status st = B.starts.reserve(W)) return st;
  if (gg_status st = B.err.reserve(1)) return st;
  GG_HIP(hipMemcpyAsync(B.off, H.off.data(), sizeof(uint32_t) * H.off.size(), hipMemcpyHostToDevice, s));
  GG_HIP(hipMemcpyAsync(B.lists, H.lists.data(), sizeof(uint64_t) * H.lists.size(), hipMemcpyHostToDevice, s));
  GG_HIP(hipMemsetAsync(B.err, 0xFF, sizeof(unsigned long long), s));
  P.off = B.off; P.lists = B.lists; P.counts = B.counts; P.err = B.err; P.starts = B.starts;
  P.addr = nullptr; P.meta = nullptr; P.cap = 0;
  const uint32_t blocks = (uint32_t)((W + kMemWaves - 1) / kMemWaves);
  hipLaunchKernelGGL(k_mem_count, dim3(blocks), dim3(kMemWaves * GG_WAVE), 0, s, P);
  GG_HIP(hipGetLastError());
  std::vector<uint32_t> cnt(W * kCntWords);
  unsigned long long err = kNoErr;
  GG_HIP(hipMemcpyAsync(cnt.data(), B.counts, sizeof(uint32_t) * cnt.size(), hipMemcpyDeviceToHost, s));
  GG_HIP(hipMemcpyAsync(&err, B.err, sizeof(err), hipMemcpyDeviceToHost, s));
  GG_HIP(hipStreamSynchronize(s));
  if (err != kNoErr)
    return gg_fail(GG_ERR_STATE, "%s: tile %llu instruction %llu: the draw is at or above the last cumulative "
                   "probability (the reference asserts)", who, err >> 32, err & 0xFFFFFFFFull);
  // the scan: per tile over its chunks
  H.tile_offsets.assign((size_t)T + 1, 0);
  H.tails.assign(T, 0);
  H.type_counts.assign((size_t)T * GG_NUM_MEM_INS_TYPES, 0);
  H.starts.resize(W);
  uint64_t rec = 0;
  for (uint32_t t = 0; t < T; ++t) {
    const uint32_t ro_n = H.off[t + 1] - H.off[t], rw_n = H.off[T + 1 + t + 1] - H.off[T + 1 + t];
    uint32_t ro = 0, rw = 0, priv = 0, carry = 0;
    uint64_t* tc = &H.type_counts[(size_t)t * GG_NUM_MEM_INS_TYPES];
    for (uint32_t c = 0; c < P.chunks; ++c) {
      const uint64_t w = (uint64_t)t * P.chunks + c;
      const uint32_t* k = &cnt[w * kCntWords];
      H.starts[w] = chunk_start{rec, ro, rw, priv, carry};
      for (int i = 0; i < GG_NUM_MEM_INS_TYPES; ++i) tc[i] += k[i];
      if (ro_n) { ro += k[1]; rec += k[1]; }
      if (rw_n) { rw += k[2] + k[3]; rec += k[2] + k[3]; }
      priv += k[4] + k[5];
      rec += k[4] + k[5];
      carry = k[kCntAny] ? k[kCntTrail] : carry + k[0];
    }
    if ((tc[1] && ro_n > kMaxList) || ((tc[2] || tc[3]) && rw_n > kMaxList))
      return gg_fail(GG_ERR_STATE, "%s: tile %u draws from a list of %u entries, more than 32768 (the reference asserts)",
                     who, t, (tc[1] && ro_n > kMaxList) ? ro_n : rw_n);
    if (tc[0] >= (1ull << 30))
      return gg_fail(GG_ERR_RANGE, "%s: tile %u has %llu NON_MEMORY instructions: a gap may not fit 30 bits", who, t,
                     (unsigned long long)tc[0]);
    H.tails[t] = carry;
    H.tile_offsets[t + 1] = rec;
  }
  return GG_OK;
}

// Fill pass after mem_plan_launch.  Synchronizes the stream.
gg_status mem_fill_launch(mem_plan& P, const mem_host& H, mem_bufs& B, uint64_t* addr, uint32_t* meta, uint64_t cap,
                          uint64_t* tail_dev, uint64_t* types_dev, hipStream_t s)
{
  const uint64_t W = (uint64_t)P.T * P.chunks, n = H.tile_offsets[P.T];
  if (n > cap)
    return gg_fail(GG_ERR_INVALID, "gg_gen_memory_traffic: %llu records, room for %llu", (unsigned long long)n,
                   (unsigned long long)cap);
  GG_HIP(hipMemcpyAsync(B.starts, H.starts.data(), sizeof(chunk_start) * W, hipMemcpyHostToDevice, s));
  P.addr = addr; P.meta = meta; P.cap = n;
  if (n) {
    hipLaunchKernelGGL(k_mem_fill, dim3((uint32_t)((W + kMemWaves - 1) / kMemWaves)), dim3(kMemWaves * GG_WAVE), 0, s, P);
    GG_HIP(hipGetLastError());
  }
  if (tail_dev) GG_HIP(hipMemcpyAsync(tail_dev, H.tails.data(), sizeof(uint64_t) * P.T, hipMemcpyHostToDevice, s));
  if (types_dev)
    GG_HIP(hipMemcpyAsync(types_dev, H.type_counts.data(), sizeof(uint64_t) * H.type_counts.size(), hipMemcpyHostToDevice, s));
  GG_HIP(hipStreamSynchronize(s));
  return GG_OK;
}

// red: GG_NUM_MLS device words.  Synchronizes the stream.
gg_status mem_stats_launch(const uint32_t* meta, const uint64_t* out, uint64_t n, unsigned long long* red,
                           uint64_t* stats, hipStream_t s)
{
  GG_HIP(hipMemsetAsync(red, 0, sizeof(uint64_t) * GG_NUM_MLS, s));
  if (n) {
    hipLaunchKernelGGL(k_mem_access_stats, dim3(noc_stats_blocks(n)), dim3(kRedThreads), 0, s, meta, out, n, red);
    GG_HIP(hipGetLastError());
  }
  GG_HIP(hipMemcpyAsync(stats, red, sizeof(uint64_t) * GG_NUM_MLS, hipMemcpyDeviceToHost, s));
  GG_HIP(hipStreamSynchronize(s));
  return GG_OK;
}

}  // namespace

// Scratch of gg_mem_synthetic_run, owned by the context (gg_destroy frees it).
struct gg_memsynth_state {
  mem_bufs bufs;
  mem_host host;
  gg_dbuf<uint64_t> addr, out, tail, types;
  gg_dbuf<uint32_t> meta;
  gg_dbuf<unsigned long long> red;
  uint64_t n = 0;
  bool valid = false;
};

void gg_memsynth_free(gg_ctx* ctx)
{
  delete ctx->memsynth;
  ctx->memsynth = nullptr;
}

extern "C" {

void gg_mem_traffic_params_default(gg_mem_traffic_params* p)
{
  if (!p) return;
  *p = gg_mem_traffic_params{};
  p->num_threads = 64;                     // inputs/input.64
  p->degree_of_sharing = 1;
  p->num_shared_addresses = 1024;
  p->num_private_addresses = 256;
  p->instructions_per_tile = 10000;
  const float pr[GG_NUM_MEM_INS_TYPES] = {0.7f, 0.025f, 0.060f, 0.015f, 0.14f, 0.06f};
  for (int i = 0; i < GG_NUM_MEM_INS_TYPES; ++i) p->probability[i] = pr[i];
  p->seed_base = 0;
  p->map_seed = 1;
}

gg_status gg_gen_memory_traffic(const gg_mem_traffic_params* p, uint32_t num_tiles, uint32_t line_bytes,
                                uint64_t* tile_offsets, uint64_t* num_records, uint64_t* addr_dev, uint32_t* meta_dev,
                                uint64_t capacity, uint64_t* tail_cycles_dev, uint64_t* type_counts_dev, void* stream)
{
  if (!addr_dev != !meta_dev)
    return gg_fail(GG_ERR_INVALID, "gg_gen_memory_traffic: addr_dev and meta_dev are both NULL (plan) or both set (fill)");
  mem_plan P{};
  mem_host H;
  if (gg_status st = mem_prepare(p, num_tiles, line_bytes, &P, &H)) return st;
  mem_bufs B;                              // call-local
  hipStream_t s = (hipStream_t)stream;
  if (gg_status st = mem_plan_launch(P, H, B, s)) return st;
  if (tile_offsets) std::copy(H.tile_offsets.begin(), H.tile_offsets.end(), tile_offsets);
  if (num_records) *num_records = H.tile_offsets[num_tiles];
  if (!addr_dev) return GG_OK;
  return mem_fill_launch(P, H, B, addr_dev, meta_dev, capacity, tail_cycles_dev, type_counts_dev, s);
}

gg_status gg_mem_latency_stats(const gg_trace* trace, const uint64_t* access_out_dev, uint64_t* stats, void* stream)
{
  if (!trace || !stats) return gg_fail(GG_ERR_INVALID, "gg_mem_latency_stats: NULL argument");
  if (trace->num_records && (!trace->meta_dev || !access_out_dev))
    return gg_fail(GG_ERR_INVALID, "gg_mem_latency_stats: NULL device array");
  gg_dbuf<unsigned long long> red;         // call-local
  if (gg_status st = red.reserve(GG_NUM_MLS)) return st;
  return mem_stats_launch(trace->meta_dev, access_out_dev, trace->num_records, red, stats, (hipStream_t)stream);
}

gg_status gg_mem_synthetic_run(gg_ctx* ctx, const gg_mem_traffic_params* p, uint64_t* stats, void* stream)
{
  GG_NOT_ATAC(ctx, "gg_mem_synthetic_run");
  if (!ctx || !p || !stats) return gg_fail(GG_ERR_INVALID, "gg_mem_synthetic_run: NULL argument");
  mem_plan P{};
  if (!ctx->memsynth) ctx->memsynth = new gg_memsynth_state();
  gg_memsynth_state& S = *ctx->memsynth;
  S.valid = false;
  const uint32_t T = ctx->cfg.num_tiles;
  if (gg_status st = mem_prepare(p, T, ctx->cfg.line_size, &P, &S.host)) return st;
  hipSetDevice(ctx->device);
  hipStream_t s = (hipStream_t)stream;
  if (gg_status st = mem_plan_launch(P, S.host, S.bufs, s)) return st;
  const uint64_t n = S.host.tile_offsets[T];
  const uint64_t room = n ? n : 1;
  if (gg_status st = gg_reserve_all(room, room, S.addr, S.out)) return st;
  if (gg_status st = S.meta.reserve(room)) return st;
  if (gg_status st = S.tail.reserve(T)) return st;
  if (gg_status st = S.types.reserve((uint64_t)T * GG_NUM_MEM_INS_TYPES)) return st;
  if (gg_status st = S.red.reserve(GG_NUM_MLS)) return st;
  if (gg_status st = mem_fill_launch(P, S.host, S.bufs, S.addr, S.meta, n, S.tail, S.types, s)) return st;
  S.n = n;
  const gg_trace tr{S.addr, S.meta, S.host.tile_offsets.data(), n};
  if (gg_status st = gg_coherent_run(ctx, &tr, S.out, stream)) return st;
  if (gg_status st = mem_stats_launch(S.meta, S.out, n, S.red, stats, s)) return st;
  std::vector<uint64_t> ts((size_t)T * GG_NUM_TILE_STATS);
  if (gg_status st = gg_coherent_get_stats(ctx, ts.data(), nullptr, nullptr)) return st;
  const uint64_t cycle_ps = (uint64_t)ceil(1000.0 / ctx->cfg.frequency_ghz);    // Latency(1, f) (time_types.h:81-109)
  uint64_t max_clock = 0;
  for (uint32_t t = 0; t < T; ++t) {
    max_clock = std::max(max_clock, ts[(size_t)t * GG_NUM_TILE_STATS + GG_CT_CLOCK_PS] + S.host.tails[t] * cycle_ps);
    for (int i = 0; i < GG_NUM_MEM_INS_TYPES; ++i)
      stats[GG_MLS_TYPE_COUNTS + i] += S.host.type_counts[(size_t)t * GG_NUM_MEM_INS_TYPES + i];
  }
  stats[GG_MLS_MAX_TILE_CLOCK_PS] = max_clock;
  S.valid = true;
  return GG_OK;
}

gg_status gg_mem_synthetic_get(gg_ctx* ctx, gg_trace* trace, const uint64_t** access_out_dev,
                               const uint64_t** tail_cycles_dev, const uint64_t** type_counts_dev)
{
  if (!ctx) return gg_fail(GG_ERR_INVALID, "gg_mem_synthetic_get: ctx NULL");
  if (!ctx->memsynth || !ctx->memsynth->valid)
    return gg_fail(GG_ERR_INVALID, "gg_mem_synthetic_get: no finished gg_mem_synthetic_run on this context");
  const gg_memsynth_state& S = *ctx->memsynth;
  if (trace) *trace = gg_trace{S.addr, S.meta, S.host.tile_offsets.data(), S.n};
  if (access_out_dev) *access_out_dev = S.out;
  if (tail_cycles_dev) *tail_cycles_dev = S.tail;
  if (type_counts_dev) *type_counts_dev = S.types;
  return GG_OK;
}

gg_status gg_mem_synthetic_copy(gg_ctx* ctx, uint64_t* addr_dev, uint32_t* meta_dev, uint64_t* access_out_dev,
                                uint64_t* tail_cycles_dev, uint64_t* type_counts_dev, void* stream)
{
  if (!ctx) return gg_fail(GG_ERR_INVALID, "gg_mem_synthetic_copy: ctx NULL");
  if (!ctx->memsynth || !ctx->memsynth->valid)
    return gg_fail(GG_ERR_INVALID, "gg_mem_synthetic_copy: no finished gg_mem_synthetic_run on this context");
  const gg_memsynth_state& S = *ctx->memsynth;
  const uint32_t T = ctx->cfg.num_tiles;
  hipSetDevice(ctx->device);
  hipStream_t s = (hipStream_t)stream;
  if (addr_dev && S.n) GG_HIP(hipMemcpyAsync(addr_dev, S.addr, sizeof(uint64_t) * S.n, hipMemcpyDeviceToDevice, s));
  if (meta_dev && S.n) GG_HIP(hipMemcpyAsync(meta_dev, S.meta, sizeof(uint32_t) * S.n, hipMemcpyDeviceToDevice, s));
  if (access_out_dev && S.n)
    GG_HIP(hipMemcpyAsync(access_out_dev, S.out, sizeof(uint64_t) * S.n, hipMemcpyDeviceToDevice, s));
  if (tail_cycles_dev) GG_HIP(hipMemcpyAsync(tail_cycles_dev, S.tail, sizeof(uint64_t) * T, hipMemcpyDeviceToDevice, s));
  if (type_counts_dev)
    GG_HIP(hipMemcpyAsync(type_counts_dev, S.types, sizeof(uint64_t) * T * GG_NUM_MEM_INS_TYPES, hipMemcpyDeviceToDevice, s));
  GG_HIP(hipStreamSynchronize(s));
  return GG_OK;
}

}  // extern "C"
