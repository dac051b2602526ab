// gg_stats.hip — the [statistics_trace] time series of a coherent run
// (include/graphite_gpu.h, gg_stats_trace_*): a scan kernel
// over state that is already in HBM — the caches' meta bytes by state, the
// directories' entries by sharer count, the tiles' flit counters — appended
// as one sample to a device buffer.  gg_coherent_run launches it after the
// launches of every slot; it returns at once unless the slot ended a quantum
// with a sample due (the quantum state tells: quantum_end / quantum_end_walk
// leave QS_START = slot + 1), so a sample costs no host round trip and the
// step and walker kernels are untouched.
#include "gg_stats.h"
#include "gg_coh_many.h"

#include <cstring>
#include <sstream>

#include "../host/graphite_host.hpp"

namespace ggc {

enum { SH_COUNT = 0, SH_PREV_SENT, SH_PREV_BCAST, SH_PREV_RECV, SH_ARRIVED, SH_N = 8 };
constexpr uint64_t kSlotTime = ~0ull;    // k_stats_scan's barrier_ns of a device-loop slot launch

struct StatsDev {
  unsigned long long* hdr;               // [SH_N]: samples taken, the flit sums at the previous sample, arrivals
  unsigned long long* samples;           // [max_samples][stride]: GG_STF_* fields, then sharer_hist[0 .. T]
  uint64_t max_samples, interval_ns, quantum_ns;
  uint32_t stride, statistics;
};

// meta bytes by state (bits 0-1: ST_I 0, ST_S 1, ST_M 2, ST_O 3), four per word
__device__ __forceinline__ void count_word(uint32_t w, uint32_t& ex, uint32_t& sh)
{
  const uint32_t lo = w & 0x01010101u, hi = (w >> 1) & 0x01010101u;
  ex += __popc(hi & ~lo);                // MODIFIED
  sh += __popc(lo);                      // SHARED + OWNED
}
// n meta bytes at m (16-byte aligned when n is a multiple of 16: the arrays
// are hipMalloc'ed and a tile's slice is n bytes): 16-B loads, coalesced
__device__ __forceinline__ void count_meta(const GG_DP uint8_t* m, size_t n, uint32_t tid, uint32_t nt, uint32_t& ex,
                                           uint32_t& sh)
{
  if ((n & 15) == 0) {
    const GG_DP uint4* v = reinterpret_cast<const GG_DP uint4*>(m);
    for (size_t i = tid; i < n / 16; i += nt) {
      const uint4 w = v[i];
      count_word(w.x, ex, sh); count_word(w.y, ex, sh); count_word(w.z, ex, sh); count_word(w.w, ex, sh);
    }
  } else {
    for (size_t i = tid; i < n; i += nt) count_word(m[i], ex, sh);
  }
}
// directory entries [0, n) at d by sharer count into the LDS histogram: a
// valid entry with sharers (a never-used slot is {INV_ADDR, -1, UNCACHED, 0},
// a slot refilled by a replacement starts with 0 sharers).  One 16-B load per
// entry; the sharer words are not read.
__device__ __forceinline__ void count_entries(const GG_DP DEnt* d, uint32_t n, uint32_t T, uint32_t tid, uint32_t nt,
                                              uint32_t* hist, const CS& S)
{
  const GG_DP uint4* v = reinterpret_cast<const GG_DP uint4*>(d);
  // (one entry per thread and iteration; eight loads in flight per thread
  // were measured slower: profiles/r09/README.md, "Variants tried")
  for (uint32_t i = tid; i < n; i += nt) {
    const uint4 e = v[i];                // {addr lo, addr hi, owner, dstate | nsh << 16}
    const uint32_t nsh = e.w >> 16;
    if (nsh == 0 || (e.x & e.y) == 0xFFFFFFFFu) continue;
    if (nsh <= T) atomicAdd(&hist[nsh], 1u);
    else atomicOr(S.err, GG_DERR_SHARERS);
  }
}

// One workgroup per owned tile.  barrier_ns = kSlotTime: the launch of slot L
// of the device-driven loop (a sample only if the slot ended a quantum and a
// multiple of the interval lies among the barrier times it passes); else one
// sample at that time.  The sample's words are zero beforehand (gg_stats_begin).
// The body of k_stats_scan and k_stats_scan_many (as step_body / walk_body,
// gg_coh_many.h): gridDim.x is the instance's own tile count in both.
// nt = blockDim.x, read by the kernel itself (only there is it the launch's one word).
__device__ __forceinline__ void stats_scan_body(const CP& P, const CS& S, const StatsDev& D, uint32_t L, uint64_t barrier_ns,
                                                uint32_t nt)
{
  extern __shared__ uint32_t hist[];     // [T + 1] (cache_line_replication)
  __shared__ uint32_t cnt[4];            // L1 exclusive, L1 shared, L2 exclusive, L2 shared
  __shared__ unsigned long long fl[3];   // flits sent, broadcast, received of this workgroup's share of the tiles
  const uint32_t tid = threadIdx.x, lt = blockIdx.x;
  uint64_t time_ns = barrier_ns, repeat = 1;
  if (barrier_ns == kSlotTime) {
    if (S.qs[QS_START] != (uint64_t)L + 1) return;         // no quantum ended in this slot
    // quantum q ended, the run continues at quantum nq (qend_pick): the lax
    // barrier passes (q + 1) * Q ... nq * Q; the last quantum only its own
    const uint64_t q = S.ri[GG_RI_FINAL_QUANTUM], nq = (S.qs[QS_DONE] & 3) ? q + 1 : S.qs[QS_Q];   // (a pause is no end)
    const uint64_t lo = (q + 1) * D.quantum_ns, hi = nq * D.quantum_ns;
    time_ns = (lo + D.interval_ns - 1) / D.interval_ns * D.interval_ns;
    if (time_ns > hi) return;
    repeat = (hi - time_ns) / D.interval_ns + 1;
  }
  // (the count is written by the last workgroup to arrive, after every
  // workgroup has read it)
  const uint64_t idx = __hip_atomic_load(&D.hdr[SH_COUNT], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  if (idx >= D.max_samples) {            // a full buffer stops the run: never a dropped sample
    if (lt == 0 && tid == 0) atomicOr(S.err, GG_DERR_SAMPLES);
    return;
  }
  unsigned long long* smp = D.samples + idx * D.stride;
  const bool repl = (D.statistics & GG_ST_CACHE_LINE_REPLICATION) != 0;
  if (repl) {
    if (tid < 4) cnt[tid] = 0;
    for (uint32_t i = tid; i <= P.T; i += nt) hist[i] = 0;
    __syncthreads();
    uint32_t c[4] = {0, 0, 0, 0};
    const size_t n1 = (size_t)P.s1 * P.a1, n2 = (size_t)P.s2 * P.a2;
    count_meta(S.l1_meta + lt * n1, n1, tid, nt, c[0], c[1]);
    count_meta(S.l2_meta + lt * n2, n2, tid, nt, c[2], c[3]);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const uint32_t w = wave_sum(c[k]);
      if ((tid & 63) == 0 && w) atomicAdd(&cnt[k], w);
    }
    count_entries(S.dir + (size_t)lt * P.E, P.E, P.T, tid, nt, hist, S);
    // replaced entries keep their sharers until their NULLIFY completes
    count_entries(S.rep + (size_t)lt * P.R, min(S.ts[lt].nrep, P.R), P.T, tid, nt, hist, S);
    __syncthreads();
    for (uint32_t i = 1 + tid; i <= P.T; i += nt)          // one atomic per non-zero bin
      if (hist[i]) atomicAdd(&smp[GG_NUM_ST_FIELDS + i], (unsigned long long)hist[i]);
    if (tid < 4 && cnt[tid]) atomicAdd(&smp[GG_STF_L1_EXCLUSIVE + tid], (unsigned long long)cnt[tid]);
  }
  // flits: workgroup b sums the owned tiles [b * 256, b * 256 + 256), one per
  // thread, in LDS; three global atomics per such workgroup
  if ((D.statistics & GG_ST_NETWORK_UTILIZATION) && lt * nt < P.L) {
    if (tid < 3) fl[tid] = 0;
    __syncthreads();
    const uint32_t tl = lt * nt + tid;
    if (tl < P.L) {
      const GG_DP uint64_t* c = S.ctr + (size_t)S.gtile[tl] * GG_NUM_NET_COUNTERS;
      const uint64_t a = c[GG_NC_FLITS_SENT], b = c[GG_NC_FLITS_BROADCASTED], r = c[GG_NC_FLITS_RECEIVED];
      if (a) atomicAdd(&fl[0], (unsigned long long)a);
      if (b) atomicAdd(&fl[1], (unsigned long long)b);
      if (r) atomicAdd(&fl[2], (unsigned long long)r);
    }
    __syncthreads();
    if (tid < 3 && fl[tid]) atomicAdd(&smp[GG_STF_FLITS_SENT + tid], fl[tid]);
  }
  __threadfence();
  __syncthreads();
  if (tid != 0) return;
  // (one counter: two levels of counters changed nothing, profiles/r09/README.md)
  if (atomicAdd(&D.hdr[SH_ARRIVED], 1ull) != gridDim.x - 1) return;
  __threadfence();
  // the last workgroup: the run's totals so far become the interval's flits
  if (D.statistics & GG_ST_NETWORK_UTILIZATION)
    for (int k = 0; k < 3; ++k) {
      const uint64_t cum = __hip_atomic_load(&smp[GG_STF_FLITS_SENT + k], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      smp[GG_STF_FLITS_SENT + k] = cum - D.hdr[SH_PREV_SENT + k];
      D.hdr[SH_PREV_SENT + k] = cum;
    }
  smp[GG_STF_TIME_NS] = time_ns;
  smp[GG_STF_REPEAT] = repeat;
  D.hdr[SH_ARRIVED] = 0;
  __hip_atomic_store(&D.hdr[SH_COUNT], idx + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  __threadfence();
}

__global__ void __launch_bounds__(256) k_stats_scan(CP P, CS S, StatsDev D, uint32_t L, uint64_t barrier_ns)
{
  stats_scan_body(P, S, D, L, barrier_ns, blockDim.x);
}

// The scan of slot L for the live instances of an ensemble
// (gg_coherent_advance_many), grid (owned tiles, live instances): devs[j] is
// the trace of the instance at pairs[j], statistics = 0 for one without.  A
// slot ends a quantum with a sample due about once in a thousand, so what
// counts is the way out: the instance's words are wave-uniform and constant
// for the launch (the host writes them with the live list), read through the
// constant address space as the other ensemble kernels read P and S, and the
// quantum state is written by earlier launches only — scalar loads up to the
// return, two in a row (the record carries CS::qs, so the way to QS_START
// does not lead through the pair and the instance's CS).
struct StatsMany { StatsDev D; const uint64_t* qs; };
__global__ void __launch_bounds__(256) k_stats_scan_many(const ManyPair* __restrict__ pairs,
                                                         const StatsMany* __restrict__ devs, uint32_t L)
{
  const StatsMany& E = *launch_const(devs + blockIdx.y);
  if (E.D.statistics == 0) return;
  typedef const uint64_t __attribute__((address_space(4))) * CQ;
  if (((CQ)(uintptr_t)E.qs)[QS_START] != (uint64_t)L + 1) return;   // (the body's own test, on the scalar path)
  const ManyPair pr = *launch_const(pairs + blockIdx.y);
  stats_scan_body(*launch_const(pr.P), *launch_const(pr.S), E.D, L, kSlotTime, blockDim.x);
}

}  // namespace ggc

using namespace ggc;

struct gg_stats_state {
  // as configured: the trace of the runs begun from now on
  uint32_t statistics = 0;
  uint64_t interval_ns = 0, max_samples = 0;
  // of the run begun last (gg_stats_begin)
  StatsDev D{};                          // (the view the kernels take: D.hdr / D.samples point into the two below)
  gg_dbuf<unsigned long long> hdr, samples;
};

void gg_stats_free(gg_ctx* ctx)
{
  delete ctx->stats;
  ctx->stats = nullptr;
}

bool gg_stats_on(const gg_ctx* ctx) { return ctx->stats && ctx->stats->statistics != 0; }

gg_status gg_stats_trace_configure(gg_ctx* ctx, uint32_t statistics, uint64_t sampling_interval_ns, uint64_t max_samples)
{
  if (!ctx) return gg_fail(GG_ERR_INVALID, "NULL argument");
  if (statistics & ~(uint32_t)(GG_ST_NETWORK_UTILIZATION | GG_ST_CACHE_LINE_REPLICATION))
    return gg_fail(GG_ERR_INVALID, "statistics_trace: unknown statistics bits 0x%x", statistics);
  if (statistics) {
    const uint64_t Q = ctx->cfg.quantum_ns;
    if (sampling_interval_ns == 0 || Q == 0 || sampling_interval_ns % Q)
      return gg_fail(GG_ERR_INVALID, "statistics_trace: sampling_interval %llu ns must be a multiple of the lax "
                                     "barrier quantum (%llu ns)", (unsigned long long)sampling_interval_ns, (unsigned long long)Q);
    if (max_samples == 0) return gg_fail(GG_ERR_INVALID, "statistics_trace: max_samples == 0");
    // the buffer is allocated whole and zeroed at every begin: bounded (which also keeps the size in 64 bits)
    const uint64_t per = sizeof(unsigned long long) * ((uint64_t)GG_NUM_ST_FIELDS + ctx->cfg.num_tiles + 1);
    if (max_samples > GG_ST_MAX_BUFFER_BYTES / per)
      return gg_fail(GG_ERR_INVALID, "statistics_trace: max_samples %llu x %llu bytes a sample is above the %llu MiB "
                                     "a sample buffer may take (at most %llu samples at %u tiles)",
                     (unsigned long long)max_samples, (unsigned long long)per,
                     (unsigned long long)(GG_ST_MAX_BUFFER_BYTES >> 20), (unsigned long long)(GG_ST_MAX_BUFFER_BYTES / per),
                     ctx->cfg.num_tiles);
    if ((statistics & GG_ST_CACHE_LINE_REPLICATION) && ctx->cfg.protocol != GG_PROTO_MSI && ctx->cfg.protocol != GG_PROTO_MOSI)
      return gg_fail(GG_ERR_UNSUPPORTED, "statistics_trace: cache_line_replication needs a private-L2 protocol "
                                         "(pr_l1_pr_l2_dram_directory_mosi, or _msi as an extension)");
  }
  if (!ctx->stats) ctx->stats = new gg_stats_state();
  ctx->stats->statistics = statistics;
  ctx->stats->interval_ns = statistics ? sampling_interval_ns : 0;
  ctx->stats->max_samples = statistics ? max_samples : 0;
  return GG_OK;
}

gg_status gg_stats_begin(gg_ctx* ctx, hipStream_t s)
{
  gg_stats_state* st = ctx->stats;
  if (!st) return GG_OK;
  StatsDev& D = st->D;
  D.statistics = st->statistics;
  D.interval_ns = st->interval_ns;
  D.max_samples = st->max_samples;
  D.quantum_ns = ctx->cfg.quantum_ns;
  D.stride = GG_NUM_ST_FIELDS + ctx->cfg.num_tiles + 1;
  if (!D.statistics) return GG_OK;
  const uint64_t words = D.max_samples * D.stride;
  D.hdr = D.samples = nullptr;
  if (gg_status e = st->hdr.reserve(SH_N)) return e;
  if (gg_status e = st->samples.reserve(words)) return e;
  D.hdr = st->hdr.get(); D.samples = st->samples.get();
  GG_HIP(hipMemsetAsync(D.hdr, 0, sizeof(unsigned long long) * SH_N, s));
  GG_HIP(hipMemsetAsync(D.samples, 0, sizeof(unsigned long long) * words, s));
  return GG_OK;
}

static gg_status stats_launch(gg_ctx* ctx, hipStream_t s, uint32_t L, uint64_t barrier_ns)
{
  const CP* P; const CS* S; bool begun;
  if (gg_status e = gg_coh_launch_state(ctx, &P, &S, &begun)) return e;
  const StatsDev& D = ctx->stats->D;
  const size_t lds = (D.statistics & GG_ST_CACHE_LINE_REPLICATION) ? sizeof(uint32_t) * ((size_t)P->T + 1) : 0;
  hipLaunchKernelGGL(k_stats_scan, dim3(P->L), dim3(256), lds, s, *P, *S, D, L, barrier_ns);
  return GG_OK;
}

gg_status gg_stats_slot(gg_ctx* ctx, hipStream_t s, uint32_t L)
{
  if (!ctx->stats || !ctx->stats->D.statistics) return GG_OK;
  return stats_launch(ctx, s, L, kSlotTime);     // (a launch failure: the batch's hipGetLastError)
}

// ---- the ensemble (gg_coherent_advance_many): one record per live instance,
// rebuilt with the live list, and one scan launch per slot for all of them
uint32_t gg_stats_run_bits(const gg_ctx* ctx) { return ctx->stats ? ctx->stats->D.statistics : 0; }
size_t gg_stats_many_bytes() { return sizeof(StatsMany); }
void gg_stats_many_fill(gg_ctx* ctx, const CS& S, void* rec)
{
  StatsMany e{};
  if (gg_stats_run_bits(ctx)) { e.D = ctx->stats->D; e.qs = (const uint64_t*)S.qs; }
  std::memcpy(rec, &e, sizeof(e));
}
void gg_stats_many_slot(const ManyPair* pairs, const void* recs, uint32_t tiles, uint32_t live, size_t lds, hipStream_t s,
                        uint32_t L)
{
  hipLaunchKernelGGL(k_stats_scan_many, dim3(tiles, live), dim3(256), lds, s, pairs, (const StatsMany*)recs, L);
}

static gg_status stats_active(gg_ctx* ctx, const char* what)
{
  if (!ctx) return gg_fail(GG_ERR_INVALID, "NULL argument");
  if (!ctx->stats || !ctx->stats->D.statistics)
    return gg_fail(GG_ERR_INVALID, "%s: no statistics trace on this context's run (gg_stats_trace_configure, then "
                                   "gg_coherent_begin / _run)", what);
  return GG_OK;
}

gg_status gg_stats_trace_sample(gg_ctx* ctx, uint64_t barrier_time_ns)
{
  if (gg_status e = stats_active(ctx, "gg_stats_trace_sample")) return e;
  if (barrier_time_ns == kSlotTime) return gg_fail(GG_ERR_INVALID, "gg_stats_trace_sample: time out of range");
  const CP* P; const CS* S; bool begun;
  if (gg_status e = gg_coh_launch_state(ctx, &P, &S, &begun)) return e;
  if (!begun) return gg_fail(GG_ERR_INVALID, "gg_coherent_begin first");
  hipSetDevice(ctx->device);
  hipStream_t s = ctx->last_stream;
  if (gg_status e = stats_launch(ctx, s, 0, barrier_time_ns)) return e;
  GG_HIP(hipGetLastError());
  GG_HIP(hipStreamSynchronize(s));
  return gg_coh_check(ctx);
}

gg_status gg_stats_trace_get(gg_ctx* ctx, uint64_t* fields, uint64_t* sharer_hist, uint64_t cap, uint64_t* count)
{
  if (gg_status e = stats_active(ctx, "gg_stats_trace_get")) return e;
  if (!count) return gg_fail(GG_ERR_INVALID, "NULL argument");
  hipSetDevice(ctx->device);
  const StatsDev& D = ctx->stats->D;
  GG_HIP(hipStreamSynchronize(ctx->last_stream));
  unsigned long long n = 0;
  GG_HIP(hipMemcpy(&n, D.hdr + SH_COUNT, sizeof(n), hipMemcpyDeviceToHost));
  *count = n;
  const uint64_t m = n < cap ? n : cap;
  if (m == 0 || (!fields && !sharer_hist)) return GG_OK;
  std::vector<unsigned long long> v((size_t)m * D.stride);
  GG_HIP(hipMemcpy(v.data(), D.samples, sizeof(unsigned long long) * v.size(), hipMemcpyDeviceToHost));
  const size_t nh = D.stride - GG_NUM_ST_FIELDS;
  for (uint64_t i = 0; i < m; ++i) {
    const unsigned long long* r = v.data() + (size_t)i * D.stride;
    if (fields) for (int k = 0; k < GG_NUM_ST_FIELDS; ++k) fields[(size_t)i * GG_NUM_ST_FIELDS + k] = r[k];
    if (sharer_hist) for (size_t k = 0; k < nh; ++k) sharer_hist[(size_t)i * nh + k] = r[GG_NUM_ST_FIELDS + k];
  }
  return GG_OK;
}

gg_status gg_stats_trace_dump(gg_ctx* ctx, int which, char* buf, uint64_t cap, uint64_t* needed)
{
  if (gg_status e = stats_active(ctx, "gg_stats_trace_dump")) return e;
  if (!needed) return gg_fail(GG_ERR_INVALID, "NULL argument");
  if (which != GG_ST_NETWORK_UTILIZATION && which != GG_ST_CACHE_LINE_REPLICATION)
    return gg_fail(GG_ERR_INVALID, "gg_stats_trace_dump: which = %d", which);
  const StatsDev& D = ctx->stats->D;
  if (!(D.statistics & (uint32_t)which)) return gg_fail(GG_ERR_INVALID, "gg_stats_trace_dump: statistic %d is not traced", which);
  uint64_t n = 0;
  if (gg_status e = gg_stats_trace_get(ctx, nullptr, nullptr, 0, &n)) return e;
  const uint32_t T = ctx->cfg.num_tiles, total = ctx->cfg.total_tiles ? ctx->cfg.total_tiles : T + 2;
  std::vector<uint64_t> f((size_t)n * GG_NUM_ST_FIELDS), h((size_t)n * (T + 1));
  if (n) if (gg_status e = gg_stats_trace_get(ctx, f.data(), h.data(), n, &n)) return e;
  std::ostringstream os;
  if (which == GG_ST_NETWORK_UTILIZATION) graphite_amd::writeNetworkUtilizationTrace(os, total, D.interval_ns, f.data(), n);
  else graphite_amd::writeCacheLineReplicationTrace(os, total, T, f.data(), h.data(), n);
  const std::string text = os.str();
  *needed = (uint64_t)text.size() + 1;
  if (!buf || cap < *needed) return buf ? gg_fail(GG_ERR_RANGE, "statistics trace needs %llu bytes", (unsigned long long)*needed)
                                        : GG_OK;
  std::memcpy(buf, text.c_str(), text.size() + 1);
  return GG_OK;
}

// ---- snapshot / restore of a run's trace (gg_coherent_snapshot):
// {statistics, interval_ns, max_samples} of the run begun last, then, with a
// trace on, the header words and the samples taken so far
gg_status gg_stats_snapshot(gg_ctx* ctx, std::vector<uint64_t>& w)
{
  w.assign(3, 0);
  const gg_stats_state* st = ctx->stats;
  if (!st || !st->D.statistics) return GG_OK;
  const StatsDev& D = st->D;
  w[0] = D.statistics; w[1] = D.interval_ns; w[2] = D.max_samples;
  w.resize(3 + SH_N);
  GG_HIP(hipMemcpy(w.data() + 3, D.hdr, sizeof(uint64_t) * SH_N, hipMemcpyDeviceToHost));
  const uint64_t n = std::min<uint64_t>(w[3 + SH_COUNT], D.max_samples) * D.stride;
  w.resize(3 + SH_N + n);
  if (n) GG_HIP(hipMemcpy(w.data() + 3 + SH_N, D.samples, sizeof(uint64_t) * n, hipMemcpyDeviceToHost));
  return GG_OK;
}
// the words' shape against the context (nothing is changed)
bool gg_stats_snapshot_ok(const gg_ctx* ctx, const uint64_t* w, uint64_t n)
{
  if (n < 3) return false;
  if (w[0] == 0) return n == 3;
  if (n < 3 + SH_N) return false;
  const uint64_t stride = (uint64_t)GG_NUM_ST_FIELDS + ctx->cfg.num_tiles + 1, cnt = w[3 + SH_COUNT];
  if (cnt > w[2] || w[2] > GG_ST_MAX_BUFFER_BYTES / (8 * stride)) return false;
  return n == 3 + SH_N + cnt * stride;
}
// before gg_coherent_begin: the snapshot's trace becomes the context's
gg_status gg_stats_restore_configure(gg_ctx* ctx, const uint64_t* w)
{
  if (w[0] == 0 && !ctx->stats) return GG_OK;
  return gg_stats_trace_configure(ctx, (uint32_t)w[0], w[1], w[2]);
}
// after it: the header words and the samples
gg_status gg_stats_restore_upload(gg_ctx* ctx, const uint64_t* w, uint64_t n, hipStream_t s)
{
  if (w[0] == 0) return GG_OK;
  const StatsDev& D = ctx->stats->D;
  GG_HIP(hipMemcpyAsync(D.hdr, w + 3, sizeof(uint64_t) * SH_N, hipMemcpyHostToDevice, s));
  const uint64_t m = n - 3 - SH_N;
  if (m) GG_HIP(hipMemcpyAsync(D.samples, w + 3 + SH_N, sizeof(uint64_t) * m, hipMemcpyHostToDevice, s));
  GG_HIP(hipStreamSynchronize(s));
  return GG_OK;
}
