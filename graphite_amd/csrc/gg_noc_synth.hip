// gg_noc_synth.hip — synthetic network traffic on the device:
// the open-loop packet generator of the reference's NoC benchmark
// (tests/benchmarks/synthetic_network/synthetic_network.cc:140-359), the
// one-pass latency reduction over a routed batch, and the driver that chains
// generator -> gg_noc_route_batch -> reduction on a context.
#include <math.h>

#include "gg_internal.h"
#include "gg_noc_synth_dev.h"

namespace {

constexpr double kMaxExpectedCycles = 268435456.0;       // 2^28: packets_per_tile / offered_load
constexpr uint32_t kMaxTableTiles = 1u << 20;            // uniform_random keeps a 2T-entry table

// The kernels: the bodies of gg_noc_synth_dev.h on this launch's arguments.
__global__ __launch_bounds__(kGenWaves* GG_WAVE) void k_synth_generate(synth_plan P)
{
  synth_generate_body(P, P.aux + 2, blockIdx.x);
}
__global__ __launch_bounds__(kRedThreads) void k_noc_latency_stats(const uint32_t* __restrict__ src,
    const uint32_t* __restrict__ dst, const uint64_t* __restrict__ time, const uint64_t* __restrict__ arr,
    const uint64_t* __restrict__ zl, const uint64_t* __restrict__ ct, uint64_t n, unsigned long long* red)
{
  noc_latency_stats_body(src, dst, time, arr, zl, ct, n, red, blockIdx.x, gridDim.x);
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
    hipLaunchKernelGGL(k_noc_latency_stats, dim3(noc_stats_blocks(n)), dim3(kRedThreads), 0, s, pk->src_dev, pk->dst_dev, pk->time_ps_dev, out->arrival_ps_dev,
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
  gg_dbuf<uint8_t> many_tab;               // gg_noc_synthetic_run_many with this context first: its table
};

void gg_synth_free(gg_ctx* ctx)
{
  delete ctx->synth;
  ctx->synth = nullptr;
}

// ---- gg_noc_synthetic_run_many (gg_noc_many.hip): this context as one instance
gg_status gg_synth_many_prepare(gg_ctx* ctx, const gg_traffic_params* p, gg_synth_view* v, std::vector<uint32_t>* orbit)
{
  synth_plan P{};
  if (gg_status st = synth_prepare(p, ctx->cfg.num_tiles, ctx->cfg.frequency_ghz, &P, orbit)) return st;
  if (!ctx->synth) ctx->synth = new gg_synth_state();
  gg_synth_state& S = *ctx->synth;
  const uint64_t n = (uint64_t)P.T * P.N;
  if (gg_status st = gg_reserve_all(n, n, S.src, S.dst, S.len)) return st;
  if (gg_status st = gg_reserve_all(n, n, S.time, S.arr, S.zl, S.ct)) return st;
  P.src = S.src; P.dst = S.dst; P.len = S.len; P.time = S.time;
  v->P = P; v->arr = S.arr; v->zl = S.zl; v->ct = S.ct;
  return GG_OK;
}

gg_status gg_synth_many_table(gg_ctx* ctx, uint64_t bytes, void** dev)
{
  if (!ctx->synth) ctx->synth = new gg_synth_state();
  if (gg_status st = ctx->synth->many_tab.reserve(bytes)) return st;
  *dev = ctx->synth->many_tab.get();
  return GG_OK;
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
