// gg_noc_many.hip — many NoC batches side by side:
// gg_noc_route_batch_many and gg_noc_synthetic_run_many.  A load-latency
// sweep is a set of independent batches on independent contexts; one batch on
// a small mesh fills a few workgroups and costs two dozen enqueues.  Here the
// instances share every launch: the grid's y index picks the instance, its x
// index is the block the single launch would have had, and the kernels are the
// bodies of gg_noc.hip's first part / gg_noc_synth_dev.h on the instance's
// record instead of on launch arguments.  Each instance works on the state and
// the scratch of its own context, so nothing is shared but the launches.
#define GG_NOC_DEVICE_ONLY 1
#include "gg_noc.hip"
#include "gg_noc_synth_dev.h"
#include "gg_noc_many.h"

#include <string.h>

#include <algorithm>
#include <utility>

namespace {
using namespace gg;

// The record table is written by the host before the first launch and constant
// for every kernel, so it is read through the constant address space: the
// fields stay scalar loads (gg_coh_many.h's launch_const and DESIGN.md §4f have
// the story of what flat vector loads of such pointers cost).
template <class T> __device__ __forceinline__ const T* launch_const(const T* p)
{
  typedef const T __attribute__((address_space(4))) * CT;
  return (const T*)(CT)(uintptr_t)p;          // (through an integer: a plain cast chain is folded away)
}
// a synthetic instance whose generator stopped early routes nothing (uniform per block)
__device__ __forceinline__ bool stop_word(const uint32_t* w) { return __builtin_amdgcn_readfirstlane((int)*w) != 0; }
__device__ __forceinline__ bool rec_stopped(const NocManyRec& R) { return R.stop && stop_word(R.stop); }

// Every wrapper: the record at blockIdx.y, then a return that is uniform per
// block for blocks beyond the instance's own grid, before the body touches
// anything or meets a barrier.
constexpr uint32_t kPkThreads = 256;
__global__ __launch_bounds__(kPkThreads) void k_many_init(const NocManyRec* recs)
{
  const NocManyRec& R = *launch_const(recs + blockIdx.y);
  if ((uint64_t)blockIdx.x * kPkThreads >= R.n || rec_stopped(R)) return;
  init_pkts_body(R.src, R.t0, R.n, nullptr, R.S, (uint64_t)blockIdx.x * kPkThreads + threadIdx.x);
}
__global__ __launch_bounds__(kPkThreads) void k_many_zero_counts(const NocManyRec* recs, uint32_t words)
{
  const NocManyRec& R = *launch_const(recs + blockIdx.y);
  const uint32_t i = blockIdx.x * kPkThreads + threadIdx.x;
  if (i < words) R.counts[i] = 0;
}
__global__ __launch_bounds__(kPkThreads) void k_many_keys(const NocManyRec* recs, int stage)
{
  const NocManyRec& R = *launch_const(recs + blockIdx.y);
  if ((uint64_t)blockIdx.x * kPkThreads >= R.n || rec_stopped(R)) return;
  keys_body(R.D.P, stage, R.src, R.dst, R.n, nullptr, R.keys, R.counts, R.D.err,
            (uint64_t)blockIdx.x * kPkThreads + threadIdx.x);
}
__global__ __launch_bounds__(1024) void k_many_scan(const NocManyRec* recs, uint32_t nb)
{
  const NocManyRec& R = *launch_const(recs + blockIdx.y);
  scan_counts_body(R.counts, nb, R.off, R.cursor);
}
__global__ __launch_bounds__(kPkThreads) void k_many_bucket(const NocManyRec* recs)
{
  const NocManyRec& R = *launch_const(recs + blockIdx.y);
  if ((uint64_t)blockIdx.x * kPkThreads >= R.n || rec_stopped(R)) return;
  bucket_body(R.keys, R.n, nullptr, R.off, R.cursor, R.ids, (uint64_t)blockIdx.x * kPkThreads + threadIdx.x);
}
// the stage kernels: the grids of all instances are alike (launch-compatible contexts share w and h)
template <bool SELF>
__global__ __launch_bounds__(64 * kPortWaves) void k_many_port(const NocManyRec* recs)
{
  const NocManyRec& R = *launch_const(recs + blockIdx.y);
  if (rec_stopped(R)) return;
  port_sweep<SELF>(R.D, R.len, R.off, R.ids, R.heap, R.S, blockIdx.x);
}
__global__ __launch_bounds__(64 * kPipeWaves) void k_many_pipe(const NocManyRec* recs, int stage)
{
  const NocManyRec& R = *launch_const(recs + blockIdx.y);
  if (rec_stopped(R)) return;
  chain_pipe(R.D, stage, R.dst, R.len, R.off, R.ids, R.heap, R.S, R.pscr, R.pstride, R.pk_max, nullptr, blockIdx.x);
}
__global__ __launch_bounds__(kSweepThreads) void k_many_sweep(const NocManyRec* recs, int stage)
{
  const NocManyRec& R = *launch_const(recs + blockIdx.y);
  if (rec_stopped(R)) return;
  chain_sweep(R.D, stage, R.dst, R.len, R.off, R.ids, R.heap, R.S, nullptr, blockIdx.x);
}
__global__ __launch_bounds__(64) void k_many_chain(const NocManyRec* recs, int stage, uint32_t nchains)
{
  const NocManyRec& R = *launch_const(recs + blockIdx.y);
  if (rec_stopped(R)) return;
  chain_hbm(R.D, stage, R.dst, R.len, R.off, R.ids, R.heap, R.S, nchains, blockIdx.x * 64 + threadIdx.x);
}
__global__ __launch_bounds__(kPkThreads) void k_many_hop_counter(const NocManyRec* recs)
{
  const NocManyRec& R = *launch_const(recs + blockIdx.y);
  if ((uint64_t)blockIdx.x * kPkThreads >= R.n || rec_stopped(R)) return;
  hop_counter_body(R.D.P, R.src, R.dst, R.len, R.t0, R.n, R.arrival, R.zero_load, R.contention, R.D.ctr,
                   (uint64_t)blockIdx.x * kPkThreads + threadIdx.x);
}
// the three result arrays of a hop-by-hop instance, from its context's packet state (gg_noc_run's copies)
__global__ __launch_bounds__(kPkThreads) void k_many_out(const NocManyRec* recs)
{
  const NocManyRec& R = *launch_const(recs + blockIdx.y);
  if ((uint64_t)blockIdx.x * kPkThreads >= R.n || rec_stopped(R)) return;
  const uint64_t k = (uint64_t)blockIdx.x * kPkThreads + threadIdx.x;
  if (k >= R.n) return;
  R.arrival[k] = R.S.t[k]; R.zero_load[k] = R.S.zl[k]; R.contention[k] = R.S.ct[k];
}

// ---- synthetic traffic: generator and reduction over (instance, tile | block)
constexpr uint32_t kResWords = GG_NUM_NLS + 1;   // an instance's result: the 73 words, then the generator's stop word
struct SynthManyRec {
  synth_plan P;                  // P.aux: the stop word
  const uint32_t* orbit;         // uniform_random's table, one for the set (a function of the tile count)
  unsigned long long* red;
  const uint64_t* arr; const uint64_t* zl; const uint64_t* ct;
  uint64_t n;
  uint32_t red_blocks;
};
__global__ __launch_bounds__(kGenWaves* GG_WAVE) void k_many_generate(const SynthManyRec* recs)
{
  const SynthManyRec& R = *launch_const(recs + blockIdx.y);
  synth_generate_body(R.P, R.orbit, blockIdx.x);
}
__global__ __launch_bounds__(kRedThreads) void k_many_stats(const SynthManyRec* recs)
{
  const SynthManyRec& R = *launch_const(recs + blockIdx.y);
  if (blockIdx.x >= R.red_blocks || stop_word(R.P.aux)) return;
  noc_latency_stats_body(R.P.src, R.P.dst, R.P.time, R.arr, R.zl, R.ct, R.n, R.red, blockIdx.x, R.red_blocks);
}

// ---------------------------------------------------------------------------
// host
// ---------------------------------------------------------------------------
// What fixes the shape of an ensemble launch must be alike in every context;
// it is read from the derived NoC parameters, not from config fields.
const char* many_mismatch(gg_ctx* a, gg_ctx* b)
{
  if (a->device != b->device) return "device";
  if (a->cfg.num_tiles != b->cfg.num_tiles) return "num_tiles";
  if (a->cfg.net_model != b->cfg.net_model) return "net_model";
  if (a->cfg.net_model == GG_NET_EMESH_HOP_BY_HOP)
    for (int stage = 1; stage <= 2; ++stage)
      if (gg_noc_form(a, stage) != gg_noc_form(b, stage))
        return stage == 1 ? "the X stage's kernel form (slab pipeline, position sweep or queues in HBM)"
                          : "the Y stage's kernel form (slab pipeline, position sweep or queues in HBM)";
  return nullptr;
}

// The set-level rules, before any launch and any change of state.
gg_status many_validate(const char* what, gg_ctx* const* ctxs, uint32_t n, bool arrays_ok)
{
  if (n == 0) return gg_fail(GG_ERR_INVALID, "%s: n == 0", what);
  if (n > GG_MANY_MAX) return gg_fail(GG_ERR_INVALID, "%s: n = %u above GG_MANY_MAX = %u", what, n, (unsigned)GG_MANY_MAX);
  if (!ctxs || !arrays_ok) return gg_fail(GG_ERR_INVALID, "%s: NULL argument", what);
  std::vector<std::pair<const gg_ctx*, uint32_t>> seen(n);
  for (uint32_t i = 0; i < n; ++i) {
    if (!ctxs[i]) return gg_fail(GG_ERR_INVALID, "%s: context %u is NULL", what, i);
    seen[i] = {ctxs[i], i};
  }
  std::sort(seen.begin(), seen.end());
  uint32_t dup = ~0u, of = 0;
  for (uint32_t i = 1; i < n; ++i)
    if (seen[i].first == seen[i - 1].first && seen[i].second < dup) { dup = seen[i].second; of = seen[i - 1].second; }
  if (dup != ~0u) return gg_fail(GG_ERR_INVALID, "%s: context %u is context %u again", what, dup, of);
  for (uint32_t i = 0; i < n; ++i)
    if (ctxs[i]->cfg.net_model == GG_NET_ATAC)
      return gg_fail(GG_ERR_UNSUPPORTED, "%s: context %u has the ATAC network model (net_model): its hub and "
                     "receive-net kernels have no ensemble form, route it with gg_noc_route_batch", what, i);
  for (uint32_t i = 1; i < n; ++i)
    if (const char* f = many_mismatch(ctxs[0], ctxs[i]))
      return gg_fail(GG_ERR_INVALID, "%s: context %u differs from context 0 in %s", what, i, f);
  return GG_OK;
}

gg_status hip_status(hipError_t e, const char* what) { return e == hipSuccess ? GG_OK : gg_hip_check(e, what); }

// The instances i with stv[i] == GG_OK and a non-empty batch, in one set of
// launches on s.  stv[i] becomes what gg_noc_route_batch(ctxs[i], &pks[i],
// &outs[i]) would return; stops (NULL, or per instance NULL or a device word):
// NocManyRec::stop.  The set has passed many_validate.
void many_route(gg_ctx* const* ctxs, uint32_t n, const gg_packets* pks, const gg_packet_out* outs,
                const uint32_t* const* stops, std::vector<gg_status>& stv, hipStream_t s)
{
  std::vector<uint32_t> live;
  std::vector<NocManyRec> recs;
  uint64_t n_max = 0;
  for (uint32_t i = 0; i < n; ++i) {
    if (stv[i] != GG_OK || pks[i].num_packets == 0) continue;
    gg_noc_view v;
    if (gg_status st = gg_noc_many_prepare(ctxs[i], &pks[i], &outs[i], &v)) { stv[i] = st; continue; }
    NocManyRec R{};
    R.D = NocDev{v.P, v.q, v.nd, v.ctr, ctxs[i]->err_dev};
    R.S = PktState{v.t, v.zl, v.ct, v.cur, nullptr, nullptr};
    R.src = pks[i].src_dev; R.dst = pks[i].dst_dev; R.len = pks[i].length_bits_dev; R.t0 = pks[i].time_ps_dev;
    R.n = pks[i].num_packets;
    R.arrival = outs[i].arrival_ps_dev; R.zero_load = outs[i].zero_load_ps_dev; R.contention = outs[i].contention_ps_dev;
    R.off = v.off; R.ids = v.ids; R.keys = v.keys; R.counts = v.counts; R.cursor = v.cursor;
    R.heap = static_cast<Ev*>(v.heap);
    R.pscr = static_cast<SK*>(v.pscr); R.pstride = v.pstride; R.pk_max = v.pk_max;
    R.stop = stops ? stops[i] : nullptr;
    live.push_back(i);
    recs.push_back(R);
    n_max = std::max(n_max, R.n);
  }
  if (live.empty()) return;
  const uint32_t m = (uint32_t)live.size();
  gg_ctx* c0 = ctxs[0];
  auto fail_all = [&](gg_status st) { for (uint32_t i : live) stv[i] = st; };
  void* tab = nullptr;
  if (gg_status st = gg_noc_many_table(c0, sizeof(NocManyRec) * (uint64_t)n, &tab)) { fail_all(st); return; }
  const NocManyRec* rd = static_cast<const NocManyRec*>(tab);
  const NocParams P = recs[0].D.P;                 // the shape: tiles, w, h, model and forms are the set's
  gg_status st = GG_OK;
#define MANY_HIP(x) do { if (st == GG_OK) st = hip_status((x), #x); } while (0)
  if (P.net_model == GG_NET_EMESH_HOP_BY_HOP) {
    MANY_HIP(hipFuncSetAttribute((const void*)k_many_sweep, hipFuncAttributeMaxDynamicSharedMemorySize, (int)kStageLdsMax));
    MANY_HIP(hipFuncSetAttribute((const void*)k_many_pipe, hipFuncAttributeMaxDynamicSharedMemorySize, (int)kStageLdsMax));
    MANY_HIP(hipFuncSetAttribute((const void*)k_many_port<false>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)kPortLds));
    MANY_HIP(hipFuncSetAttribute((const void*)k_many_port<true>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)kPortLds));
  }
  // (a pageable source: the copy has left recs when the call returns)
  MANY_HIP(hipMemcpyAsync(tab, recs.data(), sizeof(NocManyRec) * m, hipMemcpyHostToDevice, s));
  if (st != GG_OK) { fail_all(st); return; }
  for (uint32_t i : live) ctxs[i]->last_stream = s;
  gg_timer_begin(c0, "noc_route_many", s);
  const dim3 pg((uint32_t)((n_max + kPkThreads - 1) / kPkThreads), m);   // packets of the largest instance
  if (P.net_model != GG_NET_EMESH_HOP_BY_HOP) {
    hipLaunchKernelGGL(k_many_hop_counter, pg, dim3(kPkThreads), 0, s, rd);
  } else {
    hipLaunchKernelGGL(k_many_init, pg, dim3(kPkThreads), 0, s, rd);
    for (int stage = 0; stage < 4; ++stage) {
      const uint32_t nb = (stage == 0 || stage == 3) ? P.tiles : (stage == 1 ? 2 * P.h : 2 * P.w);
      hipLaunchKernelGGL(k_many_zero_counts, dim3((nb + 1 + kPkThreads - 1) / kPkThreads, m), dim3(kPkThreads), 0, s, rd, nb + 1);
      hipLaunchKernelGGL(k_many_keys, pg, dim3(kPkThreads), 0, s, rd, stage);
      hipLaunchKernelGGL(k_many_scan, dim3(1, m), dim3(1024), 0, s, rd, nb);
      hipLaunchKernelGGL(k_many_bucket, pg, dim3(kPkThreads), 0, s, rd);
      const int form = noc_stage_form(P, stage);
      if (stage == 0 || stage == 3) {
        const dim3 g((P.tiles + kPortWaves - 1) / kPortWaves, m);
        if (stage == 0) hipLaunchKernelGGL(k_many_port<false>, g, dim3(64 * kPortWaves), kPortLds, s, rd);
        else hipLaunchKernelGGL(k_many_port<true>, g, dim3(64 * kPortWaves), kPortLds, s, rd);
      } else if (form == NOC_FORM_PIPE) {
        hipLaunchKernelGGL(k_many_pipe, dim3(nb, m), dim3(64 * kPipeWaves), kStageLdsMax, s, rd, stage - 1);
      } else if (form == NOC_FORM_SWEEP) {
        hipLaunchKernelGGL(k_many_sweep, dim3(nb, m), dim3(kSweepThreads), kStageLdsMax, s, rd, stage - 1);
      } else {
        hipLaunchKernelGGL(k_many_chain, dim3((nb + 63) / 64, m), dim3(64), 0, s, rd, stage - 1, nb);
      }
      MANY_HIP(hipGetLastError());
    }
    hipLaunchKernelGGL(k_many_out, pg, dim3(kPkThreads), 0, s, rd);
  }
  MANY_HIP(hipGetLastError());
#undef MANY_HIP
  gg_timer_end(c0, "noc_route_many", s);
  if (st != GG_OK) fail_all(st);
}

gg_status first_status(const std::vector<gg_status>& stv, gg_status* statuses)
{
  gg_status first = GG_OK;
  for (size_t i = 0; i < stv.size(); ++i) {
    if (statuses) statuses[i] = stv[i];
    if (first == GG_OK) first = stv[i];
  }
  return first;
}

}  // namespace

extern "C" {

gg_status gg_noc_route_batch_many(gg_ctx* const* ctxs, uint32_t n, const gg_packets* pks, const gg_packet_out* outs,
                                  gg_status* statuses, void* stream)
{
  if (gg_status st = many_validate("gg_noc_route_batch_many", ctxs, n, pks && outs)) return st;
  hipSetDevice(ctxs[0]->device);
  std::vector<gg_status> stv(n, GG_OK);
  many_route(ctxs, n, pks, outs, nullptr, stv, (hipStream_t)stream);
  return first_status(stv, statuses);
}

gg_status gg_noc_synthetic_run_many(gg_ctx* const* ctxs, uint32_t n, const gg_traffic_params* params, uint64_t* stats,
                                    gg_status* statuses, void* stream)
{
  const char* what = "gg_noc_synthetic_run_many";
  if (gg_status st = many_validate(what, ctxs, n, params && stats)) return st;
  hipSetDevice(ctxs[0]->device);
  hipStream_t s = (hipStream_t)stream;
  std::vector<gg_status> stv(n, GG_OK);
  // every instance's parameters and arrays first: a failure is that instance's, before any launch
  std::vector<gg_synth_view> views(n);
  std::vector<uint32_t> orbit;
  std::vector<uint32_t> live;
  for (uint32_t i = 0; i < n; ++i) {
    std::vector<uint32_t> o;
    stv[i] = gg_synth_many_prepare(ctxs[i], &params[i], &views[i], &o);
    if (stv[i] != GG_OK) continue;
    if (orbit.empty() && !o.empty()) orbit.swap(o);
    live.push_back(i);
  }
  if (live.empty()) return first_status(stv, statuses);
  const uint32_t m = (uint32_t)live.size();
  auto fail_all = [&](gg_status st) { for (uint32_t i : live) if (stv[i] == GG_OK) stv[i] = st; return first_status(stv, statuses); };
  // the set's table on the first context: [n] records | the orbit | [n] results
  const uint64_t rec_bytes = sizeof(SynthManyRec) * (uint64_t)n;
  const uint64_t orb_bytes = (sizeof(uint32_t) * 2ull * ctxs[0]->cfg.num_tiles + 7) & ~7ull;
  const uint64_t res_bytes = sizeof(uint64_t) * kResWords * (uint64_t)n;
  void* tab = nullptr;
  if (gg_status st = gg_synth_many_table(ctxs[0], rec_bytes + orb_bytes + res_bytes, &tab)) return fail_all(st);
  uint8_t* const tb = static_cast<uint8_t*>(tab);
  const uint32_t* orbit_d = reinterpret_cast<const uint32_t*>(tb + rec_bytes);
  uint64_t* res_d = reinterpret_cast<uint64_t*>(tb + rec_bytes + orb_bytes);
  std::vector<uint8_t> up(rec_bytes + orb_bytes, 0);
  SynthManyRec* recs = reinterpret_cast<SynthManyRec*>(up.data());
  std::vector<gg_packets> pks(n, gg_packets{});
  std::vector<gg_packet_out> outs(n, gg_packet_out{});
  std::vector<const uint32_t*> stops(n, nullptr);
  uint32_t red_max = 1;
  for (uint32_t j = 0; j < m; ++j) {
    const uint32_t i = live[j];
    const gg_synth_view& v = views[i];
    SynthManyRec& R = recs[j];
    R.P = v.P;
    R.P.last_cycle = nullptr;
    R.P.aux = reinterpret_cast<uint32_t*>(res_d + (size_t)j * kResWords + GG_NUM_NLS);
    R.orbit = orbit_d;
    R.red = reinterpret_cast<unsigned long long*>(res_d + (size_t)j * kResWords);
    R.arr = v.arr; R.zl = v.zl; R.ct = v.ct;
    R.n = (uint64_t)v.P.T * v.P.N;
    R.red_blocks = noc_stats_blocks(R.n);
    red_max = std::max(red_max, R.red_blocks);
    pks[i] = gg_packets{v.P.src, v.P.dst, v.P.len, v.P.time, R.n};
    outs[i] = gg_packet_out{v.arr, v.zl, v.ct};
    stops[i] = R.P.aux;
  }
  if (!orbit.empty()) memcpy(up.data() + rec_bytes, orbit.data(), sizeof(uint32_t) * orbit.size());
  gg_status st = hip_status(hipMemcpyAsync(tab, up.data(), up.size(), hipMemcpyHostToDevice, s), "hipMemcpyAsync(instance table)");
  if (st == GG_OK) st = hip_status(hipMemsetAsync(res_d, 0, sizeof(uint64_t) * kResWords * m, s), "hipMemsetAsync(results)");
  if (st != GG_OK) return fail_all(st);
  const SynthManyRec* rd = static_cast<const SynthManyRec*>(tab);
  hipLaunchKernelGGL(k_many_generate, dim3((ctxs[0]->cfg.num_tiles + kGenWaves - 1) / kGenWaves, m), dim3(kGenWaves * GG_WAVE),
                     0, s, rd);
  if ((st = hip_status(hipGetLastError(), "k_many_generate")) != GG_OK) return fail_all(st);
  many_route(ctxs, n, pks.data(), outs.data(), stops.data(), stv, s);
  hipLaunchKernelGGL(k_many_stats, dim3(red_max, m), dim3(kRedThreads), 0, s, rd);
  std::vector<uint64_t> res((size_t)kResWords * m);
  st = hip_status(hipGetLastError(), "k_many_stats");
  if (st == GG_OK) st = hip_status(hipMemcpyAsync(res.data(), res_d, sizeof(uint64_t) * res.size(), hipMemcpyDeviceToHost, s),
                                   "hipMemcpyAsync(results)");
  if (st == GG_OK) st = hip_status(hipStreamSynchronize(s), "hipStreamSynchronize");
  if (st != GG_OK) return fail_all(st);
  for (uint32_t j = 0; j < m; ++j) {
    const uint32_t i = live[j];
    if (stv[i] != GG_OK) continue;                  // its routing failed on the host: no stats
    const uint64_t* r = res.data() + (size_t)j * kResWords;
    if ((uint32_t)r[GG_NUM_NLS]) {
      stv[i] = gg_fail(GG_ERR_RANGE, "%s: instance %u: a tile reached cycle 2^32 - 64 before its last packet", what, i);
      continue;
    }
    memcpy(stats + (size_t)i * GG_NUM_NLS, r, sizeof(uint64_t) * GG_NUM_NLS);
  }
  return first_status(stv, statuses);
}

}  // extern "C"
