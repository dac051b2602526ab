// gg_noc_synth.hip — synthetic network traffic on the device:
// the open-loop packet generator of the reference's NoC benchmark
// (tests/benchmarks/synthetic_network/synthetic_network.cc:140-359), the
// one-pass latency reduction over a routed batch, and the driver that chains
// generator -> gg_noc_route_batch -> reduction on a context.
#include <math.h>

#include "gg_internal.h"

namespace {

constexpr uint64_t kMix = 0x9E3779B97F4A7C15ull;
constexpr uint64_t kStopCycle = (1ull << 32) - 64;       // a tile gives up here (never reached inside the host's bounds)
constexpr double kMaxExpectedCycles = 268435456.0;       // 2^28: packets_per_tile / offered_load
constexpr uint32_t kMaxTableTiles = 1u << 20;            // uniform_random keeps a 2T-entry table
constexpr int kGenWaves = 4;                             // tiles (waves) per generator workgroup
constexpr int kRedThreads = 256, kRedWaves = kRedThreads / GG_WAVE;
constexpr uint32_t kRedMaxBlocks = 1024;
constexpr int kRedSums = 7;                              // GG_NLS_PACKETS .. GG_NLS_LAST_ARRIVAL_PS

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

struct synth_plan {
  uint64_t* time;
  uint64_t* last_cycle;      // [tiles] or nullptr
  uint32_t* src;
  uint32_t* dst;
  uint32_t* len;
  uint32_t* aux;             // [0] stop flag, [2 ..] the 2T-entry orbit table (uniform_random)
  uint64_t N, seed, thr, cycle_ps;
  uint32_t T, w, h, pattern, bits;
};

// One wave per tile, 64 cycles a round: lane l decides cycle base + l, the
// ballot of the decisions gives every sending lane its packet ordinal.  The
// loop state (base, count) is the same in every lane.
__global__ __launch_bounds__(kGenWaves* GG_WAVE) void k_synth_generate(synth_plan P)
{
  const uint32_t lane = threadIdx.x & (GG_WAVE - 1);
  const uint32_t t = __builtin_amdgcn_readfirstlane(blockIdx.x * kGenWaves + (threadIdx.x >> 6));
  if (t >= P.T) return;
  const uint64_t tile_seed = splitmix64_at(P.seed, t);
  const uint32_t fixed = P.pattern == GG_TP_UNIFORM_RANDOM ? 0u : fixed_destination(P.pattern, t, P.T, P.w, P.h);
  const uint32_t* orbit = P.aux + 2;
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
// workgroup's totals go to `red` with one 64-bit atomic per word.
__global__ __launch_bounds__(kRedThreads) void k_noc_latency_stats(const uint32_t* __restrict__ src,
    const uint32_t* __restrict__ dst, const uint64_t* __restrict__ time, const uint64_t* __restrict__ arr,
    const uint64_t* __restrict__ zl, const uint64_t* __restrict__ ct, uint64_t n, unsigned long long* red)
{
  __shared__ uint32_t hist[65];
  __shared__ uint64_t part[kRedWaves][kRedSums];
  const uint32_t lane = threadIdx.x & (GG_WAVE - 1);
  const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  if (threadIdx.x < 65) hist[threadIdx.x] = 0;
  __syncthreads();
  uint64_t acc[kRedSums] = {0, 0, 0, 0, 0, 0, 0};
  const uint64_t stride = (uint64_t)gridDim.x * kRedThreads;
  for (uint64_t base = (uint64_t)blockIdx.x * kRedThreads + wave * GG_WAVE; base < n; base += stride) {
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

bool is_pow2(uint64_t x) { return x && !(x & (x - 1)); }

// The checks of gg_gen_network_traffic that need no device, and the launch
// constants.  orbit: filled for uniform_random (2T entries).
gg_status synth_prepare(const gg_traffic_params* p, uint32_t T, double f, synth_plan* P, std::vector<uint32_t>* orbit)
{
  if (!p) return gg_fail(GG_ERR_INVALID, "gg_gen_network_traffic: params NULL");
  if (T == 0 || !(f > 0)) return gg_fail(GG_ERR_INVALID, "gg_gen_network_traffic: %u tiles at %g GHz", T, f);
  if (p->pattern >= GG_NUM_TRAFFIC_PATTERNS)
    return gg_fail(GG_ERR_INVALID, "gg_gen_network_traffic: unknown traffic pattern %u", p->pattern);
  if (!(p->offered_load > 0.0 && p->offered_load <= 1.0))
    return gg_fail(GG_ERR_INVALID, "gg_gen_network_traffic: offered load %g outside (0, 1]", p->offered_load);
  if (p->packets_per_tile == 0) return gg_fail(GG_ERR_INVALID, "gg_gen_network_traffic: no packets per tile");
  if (p->packet_bytes > (1u << 28))
    return gg_fail(GG_ERR_INVALID, "gg_gen_network_traffic: packet of %u bytes", p->packet_bytes);
  // computeEMeshTopologyParams (synthetic_network.cc:343-348) asserts a full mesh
  const uint32_t w = (uint32_t)floor(sqrt((double)T)), h = (uint32_t)ceil((double)T / w);
  if ((uint64_t)w * h != T)
    return gg_fail(GG_ERR_INVALID, "gg_gen_network_traffic: %u tiles do not fill a %u x %u mesh", T, w, h);
  if ((p->pattern == GG_TP_BIT_COMPLEMENT || p->pattern == GG_TP_SHUFFLE) && !is_pow2(T))
    return gg_fail(GG_ERR_INVALID, "gg_gen_network_traffic: pattern %u needs a power-of-two tile count, not %u",
                   p->pattern, T);
  if (p->pattern == GG_TP_UNIFORM_RANDOM) {
    if (T > kMaxTableTiles) return gg_fail(GG_ERR_UNSUPPORTED, "gg_gen_network_traffic: uniform_random beyond 2^20 tiles");
    // send_matrix[i][j] = orbit[i + j] (synthetic_network.cc:238-252).  Row i and
    // column i are both the window orbit[i .. i + T): all are permutations iff
    // the first is and the orbit repeats with period T (:255-279 asserts it).
    orbit->resize(2 * (size_t)T);
    (*orbit)[0] = T / 2;
    for (size_t k = 1; k < orbit->size(); ++k) (*orbit)[k] = (uint32_t)((13ull * (*orbit)[k - 1] + 5) % T);
    std::vector<char> seen(T, 0);
    bool ok = true;
    for (uint32_t k = 0; k < T && ok; ++k) {
      ok = !seen[(*orbit)[k]] && (*orbit)[k + T] == (*orbit)[k];
      seen[(*orbit)[k]] = 1;
    }
    if (!ok)
      return gg_fail(GG_ERR_INVALID, "gg_gen_network_traffic: uniform_random's destination matrix is no set of "
                     "permutations for %u tiles (the reference asserts)", T);
  }
  if ((uint64_t)T * p->packets_per_tile >= (1ull << 32) || p->packets_per_tile >= (1ull << 32))
    return gg_fail(GG_ERR_RANGE, "gg_gen_network_traffic: %u tiles x %llu packets is beyond a batch of 2^32 - 1", T,
                   (unsigned long long)p->packets_per_tile);
  if ((double)p->packets_per_tile / p->offered_load > kMaxExpectedCycles)
    return gg_fail(GG_ERR_RANGE, "gg_gen_network_traffic: %llu packets at load %g need more than 2^28 cycles",
                   (unsigned long long)p->packets_per_tile, p->offered_load);
  P->N = p->packets_per_tile;
  P->seed = p->seed;
  P->thr = (uint64_t)ceil(p->offered_load * 9007199254740992.0);        // 2^53: u < load for the 53-bit u
  P->cycle_ps = (uint64_t)ceil(1000.0 / f);                              // Latency(1, f) (time_types.h:81-109)
  P->T = T; P->w = w; P->h = h;
  P->pattern = p->pattern;
  P->bits = (GG_NETPACKET_BYTES + p->packet_bytes) * 8u;                 // network_model.cc:196-199
  return GG_OK;
}

// aux: room for 2 + 2T words.  Synchronizes the stream.
gg_status synth_launch(synth_plan& P, const std::vector<uint32_t>& orbit, hipStream_t s)
{
  GG_HIP(hipMemsetAsync(P.aux, 0, 2 * sizeof(uint32_t), s));
  if (!orbit.empty())
    GG_HIP(hipMemcpyAsync(P.aux + 2, orbit.data(), sizeof(uint32_t) * orbit.size(), hipMemcpyHostToDevice, s));
  hipLaunchKernelGGL(k_synth_generate, dim3((P.T + kGenWaves - 1) / kGenWaves), dim3(kGenWaves * GG_WAVE), 0, s, P);
  GG_HIP(hipGetLastError());
  uint32_t stopped = 0;
  GG_HIP(hipMemcpyAsync(&stopped, P.aux, sizeof(stopped), hipMemcpyDeviceToHost, s));
  GG_HIP(hipStreamSynchronize(s));
  if (stopped)
    return gg_fail(GG_ERR_RANGE, "gg_gen_network_traffic: a tile reached cycle 2^32 - 64 before its last packet");
  return GG_OK;
}

// red: GG_NUM_NLS device words.  Synchronizes the stream.
gg_status stats_launch(const gg_packets* pk, const gg_packet_out* out, unsigned long long* red, uint64_t* stats,
                       hipStream_t s)
{
  GG_HIP(hipMemsetAsync(red, 0, sizeof(uint64_t) * GG_NUM_NLS, s));
  const uint64_t n = pk->num_packets;
  if (n) {
    const uint64_t blocks = (n + kRedThreads - 1) / kRedThreads;
    hipLaunchKernelGGL(k_noc_latency_stats, dim3((uint32_t)(blocks < kRedMaxBlocks ? blocks : kRedMaxBlocks)),
                       dim3(kRedThreads), 0, s, pk->src_dev, pk->dst_dev, pk->time_ps_dev, out->arrival_ps_dev,
                       out->zero_load_ps_dev, out->contention_ps_dev, n, red);
    GG_HIP(hipGetLastError());
  }
  GG_HIP(hipMemcpyAsync(stats, red, sizeof(uint64_t) * GG_NUM_NLS, hipMemcpyDeviceToHost, s));
  GG_HIP(hipStreamSynchronize(s));
  return GG_OK;
}

gg_status stats_check(const gg_packets* pk, const gg_packet_out* out, const uint64_t* stats)
{
  if (!pk || !out || !stats) return gg_fail(GG_ERR_INVALID, "gg_noc_latency_stats: NULL argument");
  if (pk->num_packets >= (1ull << 32))
    return gg_fail(GG_ERR_RANGE, "gg_noc_latency_stats: %llu packets is beyond a batch of 2^32 - 1",
                   (unsigned long long)pk->num_packets);
  if (pk->num_packets && (!pk->src_dev || !pk->dst_dev || !pk->time_ps_dev || !out->arrival_ps_dev ||
                          !out->zero_load_ps_dev || !out->contention_ps_dev))
    return gg_fail(GG_ERR_INVALID, "gg_noc_latency_stats: NULL packet array");
  return GG_OK;
}

}  // namespace

// Scratch of gg_noc_synthetic_run, owned by the context (gg_destroy frees it).
struct gg_synth_state {
  gg_dbuf<uint32_t> src, dst, len;
  gg_dbuf<uint64_t> time, arr, zl, ct;
  gg_dbuf<uint32_t> aux;
  gg_dbuf<unsigned long long> red;
};

void gg_synth_free(gg_ctx* ctx)
{
  delete ctx->synth;
  ctx->synth = nullptr;
}

extern "C" {

void gg_traffic_params_default(gg_traffic_params* p)
{
  if (!p) return;
  p->pattern = GG_TP_UNIFORM_RANDOM;       // synthetic_network.cc's defaults
  p->packet_bytes = 8;
  p->offered_load = 0.1;
  p->packets_per_tile = 10000;
  p->seed = 0;
}

gg_status gg_gen_network_traffic(const gg_traffic_params* p, uint32_t num_tiles, double frequency_ghz,
                                 uint32_t* src_dev, uint32_t* dst_dev, uint32_t* length_bits_dev,
                                 uint64_t* time_ps_dev, uint64_t* last_cycle_dev, void* stream)
{
  if (!p || !src_dev || !dst_dev || !length_bits_dev || !time_ps_dev)
    return gg_fail(GG_ERR_INVALID, "gg_gen_network_traffic: NULL argument");
  synth_plan P{};
  std::vector<uint32_t> orbit;
  if (gg_status st = synth_prepare(p, num_tiles, frequency_ghz, &P, &orbit)) return st;
  gg_dbuf<uint32_t> aux;                   // call-local
  if (gg_status st = aux.reserve(2 + orbit.size())) return st;
  P.src = src_dev; P.dst = dst_dev; P.len = length_bits_dev; P.time = time_ps_dev;
  P.last_cycle = last_cycle_dev;
  P.aux = aux;
  return synth_launch(P, orbit, (hipStream_t)stream);
}

gg_status gg_noc_latency_stats(const gg_packets* pk, const gg_packet_out* out, uint64_t* stats, void* stream)
{
  if (gg_status st = stats_check(pk, out, stats)) return st;
  gg_dbuf<unsigned long long> red;         // call-local
  if (gg_status st = red.reserve(GG_NUM_NLS)) return st;
  return stats_launch(pk, out, red, stats, (hipStream_t)stream);
}

gg_status gg_noc_synthetic_run(gg_ctx* ctx, const gg_traffic_params* p, uint64_t* stats, void* stream)
{
  if (!ctx || !p || !stats) return gg_fail(GG_ERR_INVALID, "gg_noc_synthetic_run: NULL argument");
  synth_plan P{};
  std::vector<uint32_t> orbit;
  if (gg_status st = synth_prepare(p, ctx->cfg.num_tiles, ctx->cfg.frequency_ghz, &P, &orbit)) return st;
  hipSetDevice(ctx->device);
  hipStream_t s = (hipStream_t)stream;
  if (!ctx->synth) ctx->synth = new gg_synth_state();
  gg_synth_state& S = *ctx->synth;
  const uint64_t n = (uint64_t)P.T * P.N;
  if (gg_status st = gg_reserve_all(n, n, S.src, S.dst, S.len)) return st;
  if (gg_status st = gg_reserve_all(n, n, S.time, S.arr, S.zl, S.ct)) return st;
  if (gg_status st = S.aux.reserve(2 + 2 * (uint64_t)P.T)) return st;
  if (gg_status st = S.red.reserve(GG_NUM_NLS)) return st;
  P.src = S.src; P.dst = S.dst; P.len = S.len; P.time = S.time;
  P.last_cycle = nullptr;
  P.aux = S.aux;
  if (gg_status st = synth_launch(P, orbit, s)) return st;
  const gg_packets pk{S.src, S.dst, S.len, S.time, n};
  const gg_packet_out out{S.arr, S.zl, S.ct};
  if (gg_status st = gg_noc_route_batch(ctx, &pk, &out, stream)) return st;
  return stats_launch(&pk, &out, S.red, stats, s);
}

}  // extern "C"
