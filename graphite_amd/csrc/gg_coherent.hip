// gg_coherent.hip — the coherent ("Mode C") path on MI355X (gfx950): the
// small kernels (reset, import / export, the round) and the host side of
// gg_coherent_* / the round.  Device code and the design notes: gg_coh_dev.h;
// the step and walker kernels: gg_coh_step.hip, gg_coh_walk.hip.
#include "gg_coh_many.h"
#include "gg_stats.h"
#include "gg_snapshot.h"
#include "gg_coh_window.h"

#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

namespace ggc {

__global__ void k_c_import(CP P, CS S, const gg_cmsg* in, uint32_t n)
{
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  import_one(P, S, in[i], &S.imp[0]);
}

// any BARRIER record in the trace (gg_coherent_quantum has no release: its caller picks the next quantum)
__global__ void k_has_barrier(const uint32_t* meta, uint64_t n, uint32_t* flag)
{
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x)
    if (meta[i] == GG_META_BARRIER) { *flag = 1; return; }
}

// Status after a quantum: active / blocked tiles, least next-access start.
__global__ void k_c_status(CP P, CS S, uint64_t* out /* [active, blocked, min_next] */)
{
  const uint32_t lt = blockIdx.x * blockDim.x + threadIdx.x;
  if (lt >= P.L) return;
  const uint64_t r = S.ts[lt].rec;
  if (r >= S.ts[lt].rec_end) return;
  atomicAdd((unsigned long long*)&out[0], 1ull);
  if (S.ts[lt].blocked) { atomicAdd((unsigned long long*)&out[1], 1ull); return; }
  const uint64_t s = S.ts[lt].clk + rec_gap(S.meta[r]) * P.gap_ps;
  atomicMin((unsigned long long*)&out[2], (unsigned long long)s);
}

// constructor state of one owned tile per workgroup (its threads stride the
// tile's arrays); directory sharer words are zeroed when a slot is first used
__global__ void __launch_bounds__(256) k_c_reset(CP P, CS S, const uint64_t* offs)
{
  const uint32_t lt = blockIdx.x, tid = threadIdx.x, nt = blockDim.x;
  if (lt >= P.L) return;
  const size_t n1 = (size_t)P.s1 * P.a1, n2 = (size_t)P.s2 * P.a2;
  for (size_t i = tid; i < n1; i += nt) { S.l1_tag[lt * n1 + i] = INV_ADDR; S.l1_meta[lt * n1 + i] = (uint8_t)((i % P.a1) << 3); }
  for (size_t i = tid; i < P.s1; i += nt) S.l1_rr[(size_t)lt * P.s1 + i] = (uint8_t)(P.a1 - 1);
  for (size_t i = tid; i < n2; i += nt) { S.l2_tag[lt * n2 + i] = INV_ADDR; S.l2_meta[lt * n2 + i] = (uint8_t)((i % P.a2) << 3); }
  for (size_t i = tid; i < P.s2; i += nt) S.l2_rr[(size_t)lt * P.s2 + i] = (uint8_t)(P.a2 - 1);
  for (size_t i = tid; i < P.E; i += nt) S.dir[(size_t)lt * P.E + i] = DEnt{INV_ADDR, -1, DS_UNCACHED, 0};
  if (tid < 2 * GG_NUM_CACHE_COUNTERS) S.cc[(size_t)lt * 2 * GG_NUM_CACHE_COUNTERS + tid] = 0;
  if (tid < GG_NUM_TILE_STATS) S.st[(size_t)lt * GG_NUM_TILE_STATS + tid] = 0;
  if (P.mosi && tid < GG_NUM_PROTO_STATS) S.ps[(size_t)lt * GG_NUM_PROTO_STATS + tid] = 0;
  if (P.mosi && tid == 0) S.ncdl[lt] = 0;
  if (tid == 0) {
    S.ts[lt].nrep = 0; S.ts[lt].nrq = 0;
    const uint32_t tile = S.gtile[lt];
    S.ts[lt].rec = offs[tile]; S.ts[lt].rec_end = offs[tile + 1];
    S.ts[lt].clk = 0; S.ts[lt].pend_start = 0; S.ts[lt].out_addr = INV_ADDR; S.ts[lt].out_time = 0;
    S.ts[lt].blocked = 0; S.ts[lt].seq = 0;
    reinterpret_cast<uint4*>(S.cnt4)[lt] = make_uint4(0, 0, 0, 0);
    if (P.dram_qm)                                   // QueueModel::create(dram/queue_model/type, min_processing_time)
      hq_init(S.dq + lt, S.dnd + (size_t)lt * P.max_list, P.max_list, P.dram_qtype, P.dram_qaux);
  }
}

__global__ void k_c_final_stats(CP P, CS S)
{
  const uint32_t lt = blockIdx.x * blockDim.x + threadIdx.x;
  if (lt >= P.L || !P.dram_qm) return;
  S.st[(size_t)lt * GG_NUM_TILE_STATS + GG_CT_DRAM_QUEUE_ANALYTICAL] = S.dq[lt].analytical;
  S.st[(size_t)lt * GG_NUM_TILE_STATS + GG_CT_DRAM_QUEUE_UTILIZED_NS] = S.dq[lt].util;
  S.st[(size_t)lt * GG_NUM_TILE_STATS + GG_CT_DRAM_QUEUE_LAST_NS] = S.dq[lt].last_req;
}

// export: group the boundary records by the shard they continue in
__device__ __forceinline__ uint32_t rec_shard(const CS& S, const gg_cmsg& m)
{
  return S.shard[m.hop == GG_HOP_NONE ? m.dst : m.hop];
}
__global__ void k_c_export_count(CS S, const gg_cmsg* b, uint32_t n, uint32_t* counts)
{
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  atomicAdd(&counts[rec_shard(S, b[i])], 1u);
}
__global__ void k_c_export_scatter(CS S, const gg_cmsg* b, uint32_t n, const uint32_t* base, uint32_t* cursor,
                                   gg_cmsg* out)
{
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const uint32_t k = rec_shard(S, b[i]);
  out[base[k] + atomicAdd(&cursor[k], 1u)] = b[i];
}

// gg_round_exchange's device side (k_c_round_tail / _commit / _import, k_c_import_slots)
__global__ void k_c_ri_quantum(CS S, uint64_t q)
{
  S.ri[GG_RI_QUANTA]++;
  S.ri[GG_RI_FINAL_QUANTUM] = q;
}
// ---- one round of gg_round_exchange with one host sync (see there) --------
// words of a rank's round status (gathered over the ranks, reduced by each): RW_* in gg_internal.h
// before RCCL: if the quantum's steps have finished (quiet), the status of the
// owned tiles (quantum_end's: the tiles waiting at a BARRIER record apart from
// the tiles blocked on a miss, and out of the least next start) and the held
// records scattered into the send slots by owning rank; else empty slots and
// the not-done flag.  Nothing here changes the context's state: a round
// another rank has not finished is repeated.
__global__ void __launch_bounds__(1024) k_c_round_tail(CP P, CS S, gg_cmsg* slots, uint32_t world, uint32_t per_rank,
                                                      uint64_t region, const uint32_t* err, uint32_t host_err,
                                                      uint64_t* dv)
{
  __shared__ unsigned long long st[5];                 // active, blocked, least next start, barrier waiters, their latest clock
  const uint32_t tid = threadIdx.x, nt = blockDim.x;
  const uint32_t quiet = *(volatile uint32_t*)S.quiet;
  for (uint32_t r = tid; r < world; r += nt) slots[(size_t)r * (region + 1)].addr = 0;
  if (tid < 5) st[tid] = tid == 2 ? ~0ull : 0ull;
  __syncthreads();
  if (quiet) {
    for (uint32_t lt = tid; lt < P.L; lt += nt) {      // k_c_status, with quantum_end's barrier words
      const uint64_t r = S.ts[lt].rec;
      if (r >= S.ts[lt].rec_end) continue;
      atomicAdd(&st[0], 1ull);
      const uint32_t b = S.ts[lt].blocked;
      if (b == kBarWait) { atomicAdd(&st[3], 1ull); atomicMax(&st[4], (unsigned long long)S.ts[lt].clk); continue; }
      if (b) { atomicAdd(&st[1], 1ull); continue; }
      atomicMin(&st[2], (unsigned long long)(S.ts[lt].clk + rec_gap(S.meta[r]) * P.gap_ps));
    }
    const uint32_t n = *(volatile uint32_t*)S.bnd_cnt;
    for (uint32_t i = tid; i < n; i += nt) {           // the held records, by owning rank
      const uint32_t r = rec_shard(S, S.bnd[i]) / per_rank;
      gg_cmsg* sl = slots + (size_t)r * (region + 1);
      const uint64_t j = atomicAdd((unsigned long long*)&sl[0].addr, 1ull);
      if (j < region) sl[1 + j] = S.bnd[i];
      else atomicOr(S.err, GG_DERR_CAP);
    }
  }
  __threadfence();
  __syncthreads();
  if (tid != 0) return;
  uint64_t sent = 0, mx = 0;
  for (uint32_t r = 0; r < world; ++r) {
    const uint64_t c = __hip_atomic_load(&slots[(size_t)r * (region + 1)].addr, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    sent += c; mx = c > mx ? c : mx;
  }
  dv[RW_SENT] = sent; dv[RW_ACTIVE] = st[0]; dv[RW_BLOCKED] = st[1];
  dv[RW_FLAGS] = (uint64_t)(__hip_atomic_load(err, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) | host_err) |
                 (quiet ? (uint64_t)(quiet - 1) << kRwStepsShift : kRwNotDone);
  dv[RW_MAXSLOT] = mx; dv[RW_MINNEXT] = st[2];
  dv[RW_BWAIT] = st[3]; dv[RW_BMAX] = st[4];
}
__device__ __forceinline__ bool round_go(const uint64_t* dv_all, uint32_t world)
{
  uint64_t bad = 0;
  for (uint32_t r = 0; r < world; ++r) bad |= dv_all[(size_t)r * RW_N + RW_FLAGS] & (kRwErrMask | kRwNotDone);
  return bad == 0;
}
// after RCCL, when every rank finished its quantum with no error: the
// quantum's end on this rank (step counters, held list, run info, record
// pools for the import) and the barrier release, quantum_end's rule over the
// gathered words of every rank (so every rank stores the same value): with
// nothing in flight, no tile blocked on a miss and every unfinished tile at a
// BARRIER record, all continue at the latest arrival — step 0 of the next
// quantum takes S.qs[QS_REL] = that clock + 1; 0 releases nobody.  Rewritten
// at every commit; a repeated round commits nothing and continues past step 0.
__global__ void k_c_round_commit(CP P, CS S, uint64_t q, const uint64_t* dv_all, uint32_t world)
{
  if (threadIdx.x != 0 || !round_go(dv_all, world)) return;
  uint64_t msgs = 0, active = 0, blocked = 0, bwait = 0, bmax = 0;
  for (uint32_t r = 0; r < world; ++r) {
    const uint64_t* w = dv_all + (size_t)r * RW_N;
    msgs += w[RW_SENT]; active += w[RW_ACTIVE]; blocked += w[RW_BLOCKED]; bwait += w[RW_BWAIT];
    bmax = w[RW_BMAX] > bmax ? w[RW_BMAX] : bmax;
  }
  S.qs[QS_REL] = (msgs == 0 && blocked == 0 && bwait == active && active != 0) ? bmax + 1 : 0ull;
  for (int i = 0; i < 7; ++i) S.ring[i] = 0;           // ring[4], quiet, imp[2]
  *S.bnd_cnt = 0;
  S.ri[GG_RI_QUANTA]++;
  S.ri[GG_RI_FINAL_QUANTUM] = q;
  S.npool[0] = S.npool[1] = P.L * kChunk;              // the next quantum's first step reads pool 1
}
// the received records [0, min(count, slot)) of every peer (nothing unless
// round_go), and the send / receive slot counts for the host.  The rank's
// own slot is read where the tail wrote it (its records never leave the GPU)
__global__ void k_c_round_import(CP P, CS S, const gg_cmsg* send, const gg_cmsg* recv, uint32_t world, uint32_t self,
                                 uint64_t region, uint64_t slot, const uint64_t* dv_all, uint64_t* counts)
{
  if (blockIdx.x == 0 && blockIdx.y == 0)
    for (uint32_t r = threadIdx.x; r < world; r += blockDim.x) {
      counts[r] = send[(size_t)r * (region + 1)].addr;
      counts[world + r] = (r == self ? send : recv)[(size_t)r * (region + 1)].addr;
    }
  if (!round_go(dv_all, world)) return;
  const gg_cmsg* sl = (blockIdx.y == self ? send : recv) + (size_t)blockIdx.y * (region + 1);
  const uint64_t c = sl[0].addr;
  const uint64_t e = c < slot ? c : slot;
  for (uint64_t i = blockIdx.x * blockDim.x + threadIdx.x; i < e; i += (uint64_t)gridDim.x * blockDim.x)
    import_one(P, S, sl[1 + i], &S.imp[0]);
}

__global__ void k_c_import_slots(CP P, CS S, const gg_cmsg* slots, uint64_t region, uint64_t lo, uint64_t hi,
                                 const uint64_t* skip)
{
  if (skip && *skip) return;
  const gg_cmsg* sl = slots + (size_t)blockIdx.y * (region + 1);
  const uint64_t c = sl[0].addr;
  const uint64_t e = c < hi ? c : hi;
  for (uint64_t i = lo + blockIdx.x * blockDim.x + threadIdx.x; i < e; i += (uint64_t)gridDim.x * blockDim.x)
    import_one(P, S, sl[1 + i], &S.imp[0]);
}

// gg_coherent_run_many's look at a batch: the run-over word and the error
// words of every live instance into one buffer (one copy, one sync)
__global__ void k_many_poll(const ManyPair* __restrict__ pairs, uint32_t live, ManyPoll* __restrict__ out)
{
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= live) return;
  const CS* S = pairs[i].S;
  const uint32_t* err = S->err;
  out[i].done = S->qs[QS_DONE];
  out[i].err = err[0];
  out[i].err_line = err[1];
}

}  // namespace ggc

using namespace ggc;
using namespace gg;

// ---------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------
struct gg_coh_state {
  CP P{};
  CS S{};
  CP* Pd = nullptr;                  // device copies of P / S (k_c_step reads its launch state through them)
  CS* Sd = nullptr;
  gg_arena mem;                      // owns every array of the state but the three buffers below
  uint64_t* status_dev = nullptr;
  uint32_t* ecount_dev = nullptr;    // export counts + cursors
  uint64_t* offs_dev = nullptr;
  uint64_t n_records = 0;
  size_t step_lds = 0, walk_lds = 0;
  uint32_t wtx = 64, wty = 64;          // threads of an X / Y walker workgroup
  bool persist_lc = false;
  bool begun = false;
  uint64_t gen = 0;                     // gg_coherent_begin count: a round in progress belongs to one run
  bool has_barrier = false;             // the bound trace holds BARRIER records (not for gg_coherent_quantum)
  // a windowed run (gg_coherent_begin_window): S.win's array,
  // a window's final flags on the device (its tile offsets go through
  // offs_dev), the hand-over kernel's verdict, the window-state kernel's
  // output [2][T]
  bool windowed = false;
  uint64_t* win_dev = nullptr;
  uint8_t* win_fin_dev = nullptr;
  uint32_t* win_bad_dev = nullptr;
  uint64_t* win_state_dev = nullptr;
  // who drives the begun run: nobody yet, the device loop (gg_coherent_run /
  // _advance) or the host (gg_coherent_quantum, the round) — they keep
  // different state words, so one run takes one of them
  enum { DRV_NONE = 0, DRV_DEVICE, DRV_HOST };
  int drv = DRV_NONE;
  // the state arrays as allocated (coh_alloc's A list): a snapshot's section
  // table comes from here
  struct Arr { const char* name; void* p; uint64_t bytes; };
  std::vector<Arr> arrs;
  std::vector<uint64_t> offs_host;      // the bound trace's tile offsets
  // packing scratch of a snapshot (gg_snapshot.hip): per-tile counts, their scan, the records
  uint32_t* pk_counts = nullptr;
  uint64_t* pk_base = nullptr;
  gg_dbuf<uint8_t> pk_stage;            // (sized in bytes; holds uint64_t records)
  // gg_coherent_run_many with this context first: the live pairs and the poll
  // words, device and pinned host ([cap] ManyPair then [cap] ManyPoll each)
  gg_dbuf<uint8_t> many_dev;
  gg_dbuf<uint8_t, gg_mem_pinned> many_host;
  uint32_t* bar_flag = nullptr;
  // live kernel timing (gg_set_timing): an event pair around every
  // kTimeSample-th launch of each kernel (mode 1; a pair around every launch,
  // mode 2, costs ~18 % of a hop-by-hop run), harvested at the batch syncs;
  // since gg_coherent_begin
  std::vector<hipEvent_t> tev;
  std::vector<int> tkind;
  uint32_t tused = 0;
  // mode 2: in-kernel spans, slot s of kind k at kt[2 * (k * kKtRing + s)]
  unsigned long long* kt_dev = nullptr;
  std::vector<unsigned long long> kt_host;
  std::vector<int> kt_kind;             // kind of each slot used since the last harvest
  double kt_tick_ns = 10.0;             // s_memrealtime period
  double ksum[5] = {0, 0, 0, 0, 0};
  uint64_t kcnt[5] = {0, 0, 0, 0, 0};      // timed launches
  uint64_t nlaunch[5] = {0, 0, 0, 0, 0};   // all launches
};
constexpr uint64_t kTimeSample = 16;
constexpr uint32_t kKtRing = 1024;      // in-kernel timing slots between two harvests (a batch is <= 256 steps)
static StepArgs step_args(const gg_coh_state* C) { return StepArgs{C->Pd, C->Sd, C->S.kt, C->S.kt_slot}; }
static void launch_walk(gg_coh_state* C, hipStream_t s, uint32_t blocks, uint32_t threads, uint32_t L, int stage,
                        bool qend = false)
{
  ggc::launch_walk(threads > 64, walk_regq(C->P), blocks, threads, C->walk_lds, s, step_args(C), L, stage, qend);
}
constexpr uint32_t kPersistTiles = 64;        // owned tiles up to which gg_coherent_run uses k_c_persist
constexpr uint32_t kPersistLaunches = 16384;  // launch indices per k_c_persist launch
static const char* kKernelNames[5] = {"coherent_step", "coherent_walk_x", "coherent_walk_y", "coherent_persist",
                                     "coherent_unused"};

template <class F> static void timed_launch(gg_ctx* ctx, gg_coh_state* C, hipStream_t s, int kind, F&& fn)
{
  if (ctx->timing >= 2 && !C->kt_dev) C->mem.alloc(&C->kt_dev, (uint64_t)C->S.kt_stride * kKtRing);   // (failure: no in-kernel spans)
  if (ctx->timing >= 2 && C->kt_dev && kind < 3 && C->kt_kind.size() < kKtRing) {
    C->nlaunch[kind]++;
    cs_set(C->S.kt, C->kt_dev);
    C->S.kt_slot = (uint32_t)C->kt_kind.size();
    C->kt_kind.push_back(kind);
    fn();
    C->S.kt = nullptr;
    return;
  }
  if (!ctx->timing || C->nlaunch[kind]++ % (ctx->timing >= 2 ? 1 : kTimeSample)) { fn(); return; }
  if (C->tev.size() < 2 * (size_t)(C->tused + 1)) {
    const size_t n0 = C->tev.size();
    C->tev.resize(n0 + 512);
    for (size_t i = n0; i < C->tev.size(); ++i) hipEventCreate(&C->tev[i]);
    C->tkind.resize(C->tev.size() / 2);
  }
  hipEventRecord(C->tev[2 * C->tused], s);
  fn();
  hipEventRecord(C->tev[2 * C->tused + 1], s);
  C->tkind[C->tused++] = kind;
}
static void timed_harvest(gg_coh_state* C)
{
  if (!C->kt_kind.empty()) {
    const size_t n = C->kt_kind.size(), st = C->S.kt_stride;
    C->kt_host.resize(n * st);
    if (hipMemcpy(C->kt_host.data(), C->kt_dev, 8 * n * st, hipMemcpyDeviceToHost) == hipSuccess) {
      for (size_t i = 0; i < n; ++i) {
        const int k = C->kt_kind[i];
        const uint32_t nb = k == 0 ? C->P.L : k == 1 ? C->P.nsx : C->P.nsy;   // every block stamps both words
        unsigned long long a = ~0ull, b = 0;
        for (uint32_t j = 0; j < nb; ++j) {
          a = std::min(a, C->kt_host[i * st + 2 * j]);
          b = std::max(b, C->kt_host[i * st + 2 * j + 1]);
        }
        if (nb && b >= a) { C->ksum[k] += (double)(b - a) * C->kt_tick_ns * 1e-6; C->kcnt[k]++; }
      }
    }
    C->kt_kind.clear();
  }
  for (uint32_t i = 0; i < C->tused; ++i) {
    float ms = 0;
    if (hipEventElapsedTime(&ms, C->tev[2 * i], C->tev[2 * i + 1]) == hipSuccess) {
      C->ksum[C->tkind[i]] += ms;
      C->kcnt[C->tkind[i]]++;
    }
  }
  C->tused = 0;
}

uint64_t gg_coherent_msg_cap(gg_ctx* ctx) { return ctx->coh ? ctx->coh->P.msg_cap : 0; }

gg_status gg_coh_kernel_stats(gg_ctx* ctx, const char* name, double* total_ms, uint64_t* launches)
{
  gg_coh_state* C = ctx->coh;
  for (int k = 0; k < 5; ++k)
    if (C && std::strcmp(name, kKernelNames[k]) == 0) {
      *total_ms = C->kcnt[k] ? C->ksum[k] / (double)C->kcnt[k] * (double)C->nlaunch[k] : 0.0;
      *launches = C->nlaunch[k];
      return GG_OK;
    }
  *total_ms = 0; *launches = 0;
  return GG_ERR_INVALID;
}

static int ilog2(uint64_t v) { int p = -1; while (v) { v >>= 1; ++p; } return p; }
// both record pools empty: their shared parts start above the owned tiles'
// first-chunk slices (Tile::alloc)
__global__ void k_pool_reset(uint32_t* npool, uint32_t base) { if (threadIdx.x < 2) npool[threadIdx.x] = base; }
static hipError_t coh_pool_reset(gg_coh_state* C, hipStream_t s)
{
  hipLaunchKernelGGL(k_pool_reset, dim3(1), dim3(64), 0, s, C->S.npool, C->P.L * kChunk);
  return hipGetLastError();
}
static int clog2(uint64_t v) { int p = ilog2(v); return ((1ull << p) == v) ? p : p + 1; }
static uint64_t lat_ps_host(uint64_t cycles, double f) { return (uint64_t)ceil(((double)1000 * cycles) / f); }

template <class D, class T> static gg_status dupload(gg_coh_state* C, D* p, const std::vector<T>& v)
{
  T* d = nullptr;
  if (gg_status st = C->mem.alloc(&d, v.size())) return st;
  if (!v.empty()) GG_HIP(hipMemcpy(d, v.data(), sizeof(T) * v.size(), hipMemcpyHostToDevice));
  cs_set(*p, d);
  return GG_OK;
}

// an array of coh_alloc's list: allocated, and entered by name and size
template <class T> static gg_status arr_alloc(gg_coh_state* C, const char* name, T** p, uint64_t n)
{
  if (gg_status st = C->mem.alloc(p, n)) return st;
  C->arrs.push_back(gg_coh_state::Arr{name, (void*)*p, sizeof(T) * n});
  return GG_OK;
}
// What a snapshot does with an array of the list.  SN_DENSE: copied whole.
// SN_PACKED: the directory arrays, the miss-type tables and the caches' tag
// arrays (~0 = an invalid line; their meta bytes carry LRU ages and stay
// dense), as records of the slots in use.  SN_PREFIX: record pools and lists, up to their live counts.
// SN_NONE: scratch that holds nothing at a quantum boundary.
enum { SN_DENSE = 0, SN_PACKED, SN_PREFIX, SN_NONE };
static int snap_policy(const char* name)
{
  for (const char* k : {"dir", "dsh", "rep", "rsh", "drng", "rrng", "mtab", "l1_tag", "l2_tag"}) if (!std::strcmp(name, k)) return SN_PACKED;
  for (const char* k : {"pool0", "pool1", "bnd", "xl", "yl"}) if (!std::strcmp(name, k)) return SN_PREFIX;
  for (const char* k : {"gscr", "gbar"}) if (!std::strcmp(name, k)) return SN_NONE;
  return SN_DENSE;
}

void gg_coh_free(gg_ctx* ctx)
{
  gg_coh_state* C = ctx->coh;
  if (!C) return;
  for (hipEvent_t e : C->tev) hipEventDestroy(e);
  delete C;
  ctx->coh = nullptr;
}

static gg_status coh_alloc(gg_ctx* ctx)
{
  GG_NOT_ATAC(ctx, "coherent mode");
  if (ctx->coh) return GG_OK;
  const gg_config& c = ctx->cfg;
  gg_coh_state* C = new gg_coh_state();
  ctx->coh = C;
  CP& P = C->P;
  CS& S = C->S;
  P.T = c.num_tiles;
  P.K = c.num_shards ? c.num_shards : 1;
  const uint32_t k0 = c.shard_begin, k1 = c.shard_end ? c.shard_end : P.K;
  if (k0 >= k1 || k1 > P.K || P.K > P.T) return gg_fail(GG_ERR_INVALID, "bad shard range [%u, %u) of %u", k0, k1, P.K);
  if (P.T > 4096) return gg_fail(GG_ERR_UNSUPPORTED, "coherent mode: more than 4096 tiles (sharer words per lane)");
  if (c.l1d_assoc > 31 || c.l2_assoc > 31) return gg_fail(GG_ERR_UNSUPPORTED, "coherent mode: associativity above 31");
  if (c.dir_assoc > 64) return gg_fail(GG_ERR_UNSUPPORTED, "coherent mode: directory associativity above 64");
  if (c.line_size != 64)       // AddressHomeLookup and the directory auto sizing use 64-byte lines here and in the oracle
    return gg_fail(GG_ERR_UNSUPPORTED, "coherent mode: line size %u (64 only)", c.line_size);
  // logical shards (the reference's hop-by-hop process blocks) and the owned tiles
  std::vector<uint32_t> shard(P.T);
  if (gg_status st = gg_shard_map(P.T, P.K, shard.data())) return st;
  std::vector<std::vector<uint32_t>> by(P.K);
  for (uint32_t t = 0; t < P.T; ++t) by[shard[t]].push_back(t);
  std::vector<uint32_t> gtile;
  {
    // equal owned shards are interleaved, so blocks b, b + ns, ... of one shard
    // share an XCD under round-robin placement (speed only)
    const uint32_t ns = k1 - k0;
    bool eq = true;
    for (uint32_t s = k0; s < k1; ++s) eq = eq && by[s].size() == by[k0].size();
    if (eq) {
      for (size_t j = 0; j < by[k0].size(); ++j)
        for (uint32_t s = 0; s < ns; ++s) gtile.push_back(by[k0 + s][j]);
    } else {
      for (uint32_t s = k0; s < k1; ++s) gtile.insert(gtile.end(), by[s].begin(), by[s].end());
    }
  }
  P.L = (uint32_t)gtile.size();
  std::vector<int32_t> ltile(P.T, -1);
  for (uint32_t l = 0; l < P.L; ++l) ltile[gtile[l]] = (int32_t)l;
  P.log_line = (uint32_t)ilog2(c.line_size);
  P.s1 = c.l1d_size_kb * 1024u / (c.l1d_assoc * c.line_size); P.a1 = c.l1d_assoc; P.pol1 = c.l1d_policy;
  P.s2 = c.l2_size_kb * 1024u / (c.l2_assoc * c.line_size); P.a2 = c.l2_assoc; P.pol2 = c.l2_policy;
  const double f = c.frequency_ghz;
  P.lat_l1d = lat_ps_host(c.l1d_data_cycles, f); P.lat_l1t = lat_ps_host(c.l1d_tags_cycles, f);
  P.lat_l2d = lat_ps_host(c.l2_data_cycles, f); P.lat_l2t = lat_ps_host(c.l2_tags_cycles, f);
  P.gap_ps = lat_ps_host(1, f);
  // DirectoryCache sizing and access time (directory_cache.cc:46-90, 243-322)
  P.dassoc = c.dir_assoc;
  const uint32_t slices = P.T;
  uint32_t entries;
  if (c.dir_total_entries == 0) {
    uint32_t sets = (uint32_t)ceil(2.0 * c.l2_size_kb * 1024 * P.T / (64.0 * c.dir_assoc * slices));
    sets = 1u << clog2(sets);
    entries = sets * c.dir_assoc;
  } else entries = c.dir_total_entries;
  P.E = entries;
  const uint32_t dsets = entries / c.dir_assoc;
  // computeSetIndex folds floorLog2(sets)-bit fields (directory_cache.cc:64, 332-348): a set count that is no
  // power of two uses its first 2^floorLog2 sets only; one set folds 0-bit fields and never ends in the reference
  if (dsets < 2) return gg_fail(GG_ERR_UNSUPPORTED, "the directory needs at least two sets (dir_total_entries / dir_assoc)");
  P.log_dsets = (uint32_t)ilog2(dsets);
  P.log_slices = (uint32_t)clog2(slices);
  const uint64_t dir_size = (uint64_t)entries * (uint64_t)ceil(1.0 * P.T / 8);
  uint64_t cyc = c.dir_access_cycles;
  if (cyc == 0) {
    const uint32_t kb = (uint32_t)ceil(1.0 * dir_size / 1024);
    cyc = kb <= 16 ? 1 : kb <= 32 ? 2 : kb <= 64 ? 4 : kb <= 128 ? 6 : kb <= 256 ? 8 :
          kb <= 512 ? 10 : kb <= 1024 ? 13 : kb <= 2048 ? 16 : 20;
  }
  P.lat_dir = lat_ps_host(cyc, f);
  P.W = (P.T + 63) / 64;
  P.R = 64;
  P.QC = P.T + P.R + 8;
  P.IC = 2 * P.T + 256;
  const uint32_t idb = P.T > 1 ? (uint32_t)clog2(P.T) : 0;
  P.bits_req = 2 * idb + 4 + 48;
  P.bits_data = P.bits_req + 8 * c.line_size;
  P.bits_ifc = P.bits_req + idb;                 // …mosi/shmem_msg.cc:137-139: + the single receiver
  if (c.protocol > GG_PROTO_SHL2_MESI)
    return gg_fail(GG_ERR_INVALID, "protocol must be GG_PROTO_MSI, _MOSI, _SHL2_MSI or _SHL2_MESI");
  P.mosi = c.protocol == GG_PROTO_MOSI ? 1u : 0u;
  P.shl2 = c.protocol == GG_PROTO_SHL2_MSI || c.protocol == GG_PROTO_SHL2_MESI ? 1u : 0u;
  P.mesi = c.protocol == GG_PROTO_SHL2_MESI ? 1u : 0u;
  if (P.shl2) {
    // pr_l1_sh_l2_msi / _mesi: the directory entries are the L2 slice's lines
    // (ShL2CacheLineInfo); set = L2CacheHashFn (l2_cache_hash_fn.cc:18-34),
    // the directory's XOR fold with log2(L2 sets) bits and no slice bits
    if (P.s2 < 2 || (P.s2 & (P.s2 - 1))) return gg_fail(GG_ERR_UNSUPPORTED, "pr_l1_sh_l2_msi: L2 sets must be a power of two >= 2");
    if (P.a2 > 64) return gg_fail(GG_ERR_UNSUPPORTED, "pr_l1_sh_l2_msi: at most 64 L2 ways");
    if (c.l2_track_miss_types) return gg_fail(GG_ERR_UNSUPPORTED, "pr_l1_sh_l2_msi: L2 miss types are not tracked");
    P.E = P.s2 * P.a2; P.dassoc = P.a2; P.log_dsets = (uint32_t)ilog2(P.s2); P.log_slices = 0;
  }
  P.dram_qm = c.dram_queue_model_enabled;
  P.dram_qtype = c.dram_queue_model_type;
  P.dram_qaux = hq_aux(c.dram_queue_model_type, c.basic_moving_avg, c.history_list_no_interleaving);
  P.max_list = c.max_list_size ? c.max_list_size : 100;
  if (P.dram_qm)
    if (gg_status e = gg_check_queue_model(P.dram_qtype, P.dram_qaux, P.max_list)) return e;
  P.analytical = c.analytical_enabled;
  P.dram_proc = (uint64_t)((float)c.line_size / c.dram_bandwidth) + 1;
  P.dram_cost = (uint64_t)(float)c.dram_latency_ns;
  P.msg_cap = (uint32_t)std::min<uint64_t>((uint64_t)64 * P.T + (uint64_t)kChunk * 2 * P.T + 65536, 0x7FFFFFFFull);
  P.np = gg_noc_params(ctx);
  P.net = c.net_model;
  P.mw = P.np.w; P.mh = P.np.h;
  P.qimg = (uint32_t)((sizeof(HQueue) + (size_t)P.np.max_size * sizeof(HNode) + 15) & ~(size_t)15);
  // hop-by-hop chain segments: the runs of each row / column inside one owned shard
  std::vector<Seg> segx, segy;
  std::vector<uint32_t> tseg((size_t)P.T * 2, ~0u);
  P.seg_xcd = 0;
  if (P.net == GG_NET_EMESH_HOP_BY_HOP) {
    if (P.mw * P.mh != P.T) return gg_fail(GG_ERR_UNSUPPORTED, "emesh_hop_by_hop needs a full W x H mesh (hop_by_hop.cc:55-59)");
    auto owned = [&](uint32_t t) { return ltile[t] >= 0; };
    const uint32_t ns = k1 - k0;
    bool inter = true;                 // every owned shard has the same number of runs per pass
    for (int pass = 0; pass < 2; ++pass) {
      const uint32_t lines = pass == 0 ? P.mh : P.mw, len = pass == 0 ? P.mw : P.mh;
      std::vector<std::vector<Seg>> per(ns);
      for (uint32_t ln = 0; ln < lines; ++ln) {
        auto at = [&](uint32_t pos) { return pass == 0 ? ln * P.mw + pos : pos * P.mw + ln; };
        uint32_t a = 0;
        while (a < len) {
          uint32_t b = a;
          while (b + 1 < len && shard[at(b + 1)] == shard[at(a)]) ++b;
          if (owned(at(a))) per[shard[at(a)] - k0].push_back(Seg{ln, a, b, 0});
          a = b + 1;
        }
      }
      for (uint32_t k = 1; k < ns; ++k) inter = inter && per[k].size() == per[0].size();
      // runs of one shard interleaved (run j of shard k at slot j * ns + k), so
      // with the walker block decode of k_c_walk a shard's walkers share the
      // XCD of its tiles under round-robin placement (speed only)
      std::vector<Seg>& out = pass == 0 ? segx : segy;
      if (inter) {
        for (size_t j = 0; j < per[0].size(); ++j)
          for (uint32_t k = 0; k < ns; ++k) out.push_back(per[k][j]);
      } else {
        for (uint32_t k = 0; k < ns; ++k) out.insert(out.end(), per[k].begin(), per[k].end());
      }
      for (uint32_t i = 0; i < out.size(); ++i) {
        const Seg& g = out[i];
        for (uint32_t q = g.lo; q <= g.hi; ++q) {
          const uint32_t t = pass == 0 ? g.line * P.mw + q : q * P.mw + g.line;
          tseg[(size_t)t * 2 + pass] = i;
        }
      }
    }
    P.seg_xcd = inter ? ns : 0;
  }
  P.nsx = (uint32_t)segx.size() * 2; P.nsy = (uint32_t)segy.size() * 2;
  uint32_t maxrun = 1, mrx = 1, mry = 1;
  for (const Seg& s : segx) mrx = std::max(mrx, s.hi - s.lo + 1);
  for (const Seg& s : segy) mry = std::max(mry, s.hi - s.lo + 1);
  maxrun = std::max(mrx, mry);
  {
    // walkers: one wave per position (the pipeline) when a run has at most
    // kMaxWalkWaves routers, else one wave sweeping the positions
    const char* sw = getenv("GG_COH_WALK_SWEEP");
    const bool sweep = sw && atoi(sw);
    C->wtx = !sweep && mrx <= kMaxWalkWaves ? 64 * mrx : 64;
    C->wty = !sweep && mry <= kMaxWalkWaves ? 64 * mry : 64;
  }
  {
    const size_t fixed = (size_t)maxrun * (P.qimg + kNetCtr * 8) + kWalkSync;
    if (P.net == GG_NET_EMESH_HOP_BY_HOP && fixed + 64 * kWalkPkBytes > kWalkLdsMax)
      return gg_fail(GG_ERR_UNSUPPORTED, "emesh_hop_by_hop: a shard's %u-router run does not fit the LDS of one walker", maxrun);
    P.walk_pk = (uint32_t)std::min<size_t>(4096, (kWalkLdsMax - fixed) / kWalkPkBytes);
    C->walk_lds = fixed + (size_t)P.walk_pk * kWalkPkBytes;
  }
  P.seg_cap = P.msg_cap;
  {
    const char* te = getenv("GG_COH_TOUCH_EACH");
    P.touch_each = te && atoi(te) ? 1u : 0u;
    const char* ww = getenv("GG_COH_WALK_WIDE");
    P.walk_wide = ww && atoi(ww) ? 1u : 0u;
    P.no_hit_runs = 0u;
  }
  C->step_lds = sizeof(StepLds);
  {
    // cache state in LDS for persistent launches of closed-form networks (no walkers)
    const size_t n1 = (size_t)P.s1 * P.a1, n2 = (size_t)P.s2 * P.a2;
    P.cache_lds_off = (uint32_t)((C->step_lds + 15) & ~(size_t)15);
    P.cache_lds_bytes = (uint32_t)(9 * (n1 + n2) + P.s1 + P.s2);
    C->persist_lc = P.net != GG_NET_EMESH_HOP_BY_HOP && (size_t)P.cache_lds_off + P.cache_lds_bytes <= 160 * 1024;
  }
  GG_HIP(step_set_lds(C->step_lds, C->persist_lc ? (size_t)P.cache_lds_off + P.cache_lds_bytes : 0,
                      std::max(C->walk_lds, C->step_lds)));
  if (P.net == GG_NET_EMESH_HOP_BY_HOP) GG_HIP(walk_set_lds(C->walk_lds));
  const uint64_t L = P.L;
  gg_status st = GG_OK;
#define A(ptr, n) if (st == GG_OK) st = arr_alloc(C, #ptr, &S.ptr, (n))
  A(l1_tag, L * P.s1 * P.a1); A(l1_meta, L * P.s1 * P.a1); A(l1_rr, L * P.s1);
  A(l2_tag, L * P.s2 * P.a2); A(l2_meta, L * P.s2 * P.a2); A(l2_rr, L * P.s2);
  A(cc, L * 2 * GG_NUM_CACHE_COUNTERS); A(st, L * GG_NUM_TILE_STATS);
  // miss-type tracking (default off): one address table per (tile, cache)
  // (MSI's L1CacheCntlr hands the L1-D the L1-I flag, l1_cache_cntlr.cc:69; MOSI its own, …mosi/l1:68)
  P.mt1 = ((P.mosi || P.shl2) ? ctx->cfg.l1d_track_miss_types : ctx->cfg.l1i_track_miss_types) ? 1u : 0u;   // (sh_l2: its own flag, …sh_l2_msi/l1:67)
  P.mt2 = ctx->cfg.l2_track_miss_types ? 1u : 0u;
  {
    // the fast step instance: every queue it serves a history tree held in
    // registers (or no queue model), no miss types; GG_COH_NO_FAST=1 forces
    // the general instance (A/B)
    const bool rq_net = !P.np.qm || (P.np.qtype == GG_QM_HISTORY_TREE && P.np.max_size <= kQMax);
    const bool rq_dram = !P.dram_qm || (P.dram_qtype == GG_QM_HISTORY_TREE && P.max_list <= kQMax);
    const char* nf = getenv("GG_COH_NO_FAST");
    P.fast = rq_net && rq_dram && !P.mt1 && !P.mt2 && !P.mosi && !P.shl2 && !(nf && atoi(nf)) ? 1u : 0u;
  }
  if (P.mt1 || P.mt2) {
    const uint32_t lines = ctx->cfg.miss_track_lines ? ctx->cfg.miss_track_lines : 65536u;
    if (lines & (lines - 1) || lines < 64) return gg_fail(GG_ERR_INVALID, "miss_track_lines must be a power of two >= 64");
    P.mt_log = (uint32_t)__builtin_ctz(lines);
    A(mtab, (size_t)L * 2 << P.mt_log); A(mtc, L * 2 * GG_NUM_MISS_TYPES);
  }
  A(ts, L);
  A(dir, L * P.E); A(dsh, L * P.E * P.W);
  A(rep, L * P.R); A(rsh, L * P.R * P.W);
  A(rq, L * P.QC);
  if (P.mosi) {
    A(rqx, L * P.QC); A(drng, L * P.E); A(rrng, L * P.R); A(cdl, L * kCdl); A(ncdl, L); A(ps, L * GG_NUM_PROTO_STATS);
  }
  A(dq, L); A(dnd, L * P.max_list);
  A(pool0, P.msg_cap); A(pool1, P.msg_cap); A(npool, 2);
  A(inb0, L * P.IC); A(inb1, L * P.IC); A(cnt4, L * 4);
  const uint64_t al = P.net == GG_NET_EMESH_HOP_BY_HOP ? L * P.IC : 1;
  A(arv0, al); A(arv1, al);
  A(xl, (uint64_t)std::max(P.nsx, 1u) * P.seg_cap); A(nxl, std::max(P.nsx, 1u));
  A(yl, (uint64_t)std::max(P.nsy, 1u) * P.seg_cap); A(nyl, std::max(P.nsy, 1u));
  A(bnd, P.msg_cap); A(bnd_cnt, 1);
  A(ring, 11); A(ri, GG_NUM_RUN_INFO); A(qs, QS_N); A(gbar, 4);
  A(gscr, L * 6 * P.IC);
#undef A
  {
    // in-kernel launch timing slots (timing mode 2): allocated at the first
    // timed launch (timed_launch), not for every context
    S.kt_stride = 2 * std::max(std::max(P.L, P.nsx), std::max(P.nsy, 1u));
    S.kt = nullptr; S.kt_slot = 0;
  }
  S.trs = nullptr; S.trw = nullptr; S.tr_n = 0; S.tr_wb = std::max(std::max(P.nsx, P.nsy), 1u);
  // the diagnostic buffers exist only in a diagnostics build (the product
  // kernels ignore them: no buffers, no dumps of all-zero traces)
  const bool diag = GG_COH_DIAG != 0;
  if (!diag && (getenv("GG_COH_TRACE") || getenv("GG_COH_TRACE_EV") || getenv("GG_COH_PROFILE")))
    fprintf(stderr, "[gg_coh] GG_COH_TRACE / _EV / GG_COH_PROFILE need a diagnostics build "
                    "(tools/build_variant.sh diag -DGG_COH_DIAG=1; GG_LIB=variants/diag/libgraphite_gpu.so); ignored\n");
  if (diag && getenv("GG_COH_TRACE") && atoi(getenv("GG_COH_TRACE")) > 0) {
    S.tr_n = (uint32_t)atoi(getenv("GG_COH_TRACE"));
    if ((st = C->mem.alloc(&S.trs, (size_t)S.tr_n * P.L * kTrStep))) return st;
    if ((st = C->mem.alloc(&S.trw, (size_t)S.tr_n * 2 * S.tr_wb * 8))) return st;
  }
  S.tre = nullptr; S.tre_n = 0;
  if (diag && getenv("GG_COH_TRACE_EV") && atoi(getenv("GG_COH_TRACE_EV")) > 0) {
    S.tre_n = (uint32_t)atoi(getenv("GG_COH_TRACE_EV"));
    if ((st = C->mem.alloc(&S.tre, (size_t)S.tre_n * 2 * S.tr_wb * (kTrEvMax * 4 + 4)))) return st;
  }
  if (diag && getenv("GG_COH_PROFILE") && atoi(getenv("GG_COH_PROFILE"))) {
    if ((st = C->mem.alloc(&S.prof, 1024 + 8 * 65536))) return st;
    GG_HIP(hipMemset(S.prof, 0, sizeof(unsigned long long) * (1024 + 8 * 65536)));
  }
  if (st) return st;
  // what a snapshot copies whole starts as zeros, so its bytes depend on the
  // run alone (the packed arrays are not touched: 2 GB at 1024 tiles)
  for (const gg_coh_state::Arr& a : C->arrs)
    if (snap_policy(a.name) == SN_DENSE && a.bytes) GG_HIP(hipMemset(a.p, 0, a.bytes));
  if ((st = C->mem.alloc(&C->pk_counts, L))) return st;
  if ((st = C->mem.alloc(&C->pk_base, L + 1))) return st;
  S.quiet = S.ring + 4; S.imp = S.ring + 5; S.live = S.ring + 7;
  if ((st = dupload(C, &S.gtile, gtile))) return st;
  if ((st = dupload(C, &S.ltile, ltile))) return st;
  if ((st = dupload(C, &S.shard, shard))) return st;
  if ((st = dupload(C, &S.segx, segx))) return st;
  if ((st = dupload(C, &S.segy, segy))) return st;
  if ((st = dupload(C, &S.tseg, tseg))) return st;
  {
    std::vector<uint4> ti(P.L);
    for (uint32_t l = 0; l < P.L; ++l)
      ti[l] = make_uint4(gtile[l], tseg[(size_t)gtile[l] * 2], tseg[(size_t)gtile[l] * 2 + 1], 0u);
    if ((st = dupload(C, &S.tinfo, ti))) return st;
  }
  if ((st = C->mem.alloc(&C->status_dev, 4))) return st;
  if ((st = C->mem.alloc(&C->Pd, 1))) return st;
  if ((st = C->mem.alloc(&C->Sd, 1))) return st;
  if ((st = C->mem.alloc(&C->ecount_dev, 2 * (uint64_t)P.K + 2))) return st;
  if ((st = C->mem.alloc(&C->offs_dev, (uint64_t)P.T + 1))) return st;
  cs_set(S.ctr, gg_noc_ctr(ctx));
  {
    gg::HQueue* q; gg::HNode* nd;
    gg_noc_queues(ctx, &q, &nd);
    cs_set(S.nq, q); cs_set(S.nnd, nd);
  }
  cs_set(S.err, ctx->err_dev);
  {
    // (hq_init writes a queue's header and first node only)
    gg::HQueue* q; gg::HNode* nd;
    gg_noc_queues(ctx, &q, &nd);
    GG_HIP(hipMemset(nd, 0, sizeof(gg::HNode) * ((size_t)P.T * 6 + 1) * P.np.max_size));
  }
  return GG_OK;
}

// the backstop of a windowed run (qend_window): the safe-quantum rule let a
// tile run off a window that is not the end of its trace
static gg_status coh_window_exhausted()
{
  return gg_fail(GG_ERR_STATE, "coherent mode: window exhausted (a tile reached the end of a window that is not the "
                               "end of its trace; the run's results are void)");
}
static gg_status coh_check(gg_ctx* ctx)
{
  uint32_t ew[2] = {0, 0};
  GG_HIP(hipMemcpy(ew, ctx->err_dev, sizeof(ew), hipMemcpyDeviceToHost));
  const uint32_t e = ew[0];
  if (e & GG_DERR_CAP) return gg_fail(GG_ERR_UNSUPPORTED, "coherent mode: a device capacity (records / inbox / "
                                      "request queue / replaced entries / call chain / segment, or with miss-type "
                                      "tracking the miss_track_lines address table of a tile) was exceeded");
  if (e & GG_DERR_STATE) return gg_fail(GG_ERR_STATE, "coherent mode: a state the reference would reject "
                                        "(LOG_ASSERT_ERROR / assert; first at gg_coh_dev.h:%u)", ew[1]);
  if (e & GG_DERR_SHARERS) return gg_fail(GG_ERR_STATE, "statistics trace: a directory entry holds more sharers than "
                                          "there are tiles (the scan of gg_stats.hip)");
  if (e & GG_DERR_SAMPLES) return gg_fail(GG_ERR_UNSUPPORTED, "statistics trace: the sample buffer is full "
                                          "(max_samples of gg_stats_trace_configure); no sample was dropped silently");
  if (e & GG_DERR_WINDOW) return coh_window_exhausted();
  return GG_OK;
}

gg_status gg_coh_launch_state(gg_ctx* ctx, const CP** P, const CS** S, bool* begun)
{
  hipSetDevice(ctx->device);
  if (gg_status st = coh_alloc(ctx)) return st;
  *P = &ctx->coh->P; *S = &ctx->coh->S; *begun = ctx->coh->begun;
  return GG_OK;
}

gg_status gg_coherent_begin(gg_ctx* ctx, const gg_trace* tr, uint64_t* access_out_dev, void* stream)
{
  GG_NOT_ATAC(ctx, "gg_coherent_begin");
  if (!ctx || !tr || !tr->tile_offsets) return gg_fail(GG_ERR_INVALID, "NULL argument");
  hipSetDevice(ctx->device);
  hipStream_t s = (hipStream_t)stream;
  ctx->last_stream = s;
  if (gg_status st = coh_alloc(ctx)) return st;
  gg_coh_state* C = ctx->coh;
  const CP& P = C->P;
  if (tr->tile_offsets[P.T] != tr->num_records) return gg_fail(GG_ERR_INVALID, "tile_offsets[num_tiles] != num_records");
  for (uint32_t t = 0; t < P.T; ++t)
    if (tr->tile_offsets[t] > tr->tile_offsets[t + 1]) return gg_fail(GG_ERR_INVALID, "tile_offsets not monotone");
  if (tr->num_records && (!tr->addr_dev || !tr->meta_dev)) return gg_fail(GG_ERR_INVALID, "NULL trace pointers");
  cs_set(C->S.addr, tr->addr_dev); cs_set(C->S.meta, tr->meta_dev); cs_set(C->S.out, access_out_dev);
  C->S.win = nullptr; C->windowed = false;           // (gg_coherent_begin_window sets them after this begin)
  GG_HIP(hipMemcpyAsync(C->Pd, &C->P, sizeof(CP), hipMemcpyHostToDevice, s));
  GG_HIP(hipMemcpyAsync(C->Sd, &C->S, sizeof(CS), hipMemcpyHostToDevice, s));
  C->n_records = tr->num_records;
  C->offs_host.assign(tr->tile_offsets, tr->tile_offsets + P.T + 1);
  C->drv = gg_coh_state::DRV_NONE;
  ++C->gen;
  for (int k = 0; k < 5; ++k) { C->ksum[k] = 0; C->kcnt[k] = 0; C->nlaunch[k] = 0; }
  C->tused = 0;
  GG_HIP(hipMemcpyAsync(C->offs_dev, tr->tile_offsets, sizeof(uint64_t) * (P.T + 1), hipMemcpyHostToDevice, s));
  if (gg_status st = gg_noc_reset(ctx, s)) return st;
  GG_HIP(hipMemsetAsync(ctx->err_dev, 0, 2 * sizeof(uint32_t), s));
  GG_HIP(hipMemsetAsync(C->S.ri, 0, sizeof(uint64_t) * GG_NUM_RUN_INFO, s));
  GG_HIP(coh_pool_reset(C, s));
  GG_HIP(hipMemsetAsync(C->S.ring, 0, sizeof(uint32_t) * 11, s));
  {
    uint64_t q0[QS_N] = {0, 0, 0, 0, 0, 0, ~0ull, 0, (uint64_t)ctx->cfg.quantum_ns * 1000ull, 0, 0, 0, ~0ull};
    GG_HIP(hipMemcpyAsync(C->S.qs, q0, sizeof(q0), hipMemcpyHostToDevice, s));
  }
  GG_HIP(hipMemsetAsync(C->S.bnd_cnt, 0, sizeof(uint32_t), s));
  if (C->S.tre)
    GG_HIP(hipMemsetAsync(C->S.tre, 0, sizeof(unsigned long long) * C->S.tre_n * 2 * C->S.tr_wb * (kTrEvMax * 4 + 4), s));
  if (C->S.trs) {
    GG_HIP(hipMemsetAsync(C->S.trs, 0, sizeof(unsigned long long) * C->S.tr_n * P.L * kTrStep, s));
    GG_HIP(hipMemsetAsync(C->S.trw, 0, sizeof(unsigned long long) * C->S.tr_n * 2 * C->S.tr_wb * 8, s));
  }
  if (C->S.mtab) {                                   // the miss-type address sets start empty
    GG_HIP(hipMemsetAsync(C->S.mtab, 0xFF, sizeof(uint64_t) * ((size_t)P.L * 2 << P.mt_log), s));
    GG_HIP(hipMemsetAsync(C->S.mtc, 0, sizeof(uint64_t) * P.L * 2 * GG_NUM_MISS_TYPES, s));
  }
  GG_HIP(hipMemsetAsync(C->S.nxl, 0, sizeof(uint32_t) * std::max(P.nsx, 1u), s));
  GG_HIP(hipMemsetAsync(C->S.nyl, 0, sizeof(uint32_t) * std::max(P.nsy, 1u), s));
  if (gg_status st = gg_stats_begin(ctx, s)) return st;   // (nothing without a configured statistics trace)
  hipLaunchKernelGGL(k_c_reset, dim3(P.L), dim3(256), 0, s, P, C->S, (const uint64_t*)C->offs_dev);
  GG_HIP(hipGetLastError());
  uint32_t hb = 0;
  if (tr->num_records) {
    if (!C->bar_flag) if (gg_status st = C->mem.alloc(&C->bar_flag, 1)) return st;
    GG_HIP(hipMemsetAsync(C->bar_flag, 0, sizeof(uint32_t), s));
    const uint64_t nb = std::min<uint64_t>(4096, (tr->num_records + 255) / 256);
    hipLaunchKernelGGL(k_has_barrier, dim3((uint32_t)nb), dim3(256), 0, s, tr->meta_dev, tr->num_records, C->bar_flag);
    GG_HIP(hipGetLastError());
    GG_HIP(hipMemcpyAsync(&hb, C->bar_flag, sizeof(uint32_t), hipMemcpyDeviceToHost, s));
  }
  GG_HIP(hipStreamSynchronize(s));
  C->has_barrier = hb != 0;
  C->begun = true;
  return coh_check(ctx);
}

// gg_coherent_quantum / the round on a run the device loop has advanced
static gg_status coh_host_driven(gg_coh_state* C)
{
  if (C->drv == gg_coh_state::DRV_DEVICE)
    return gg_fail(GG_ERR_INVALID, "this run is driven by gg_coherent_advance (or was restored from a snapshot): "
                                   "gg_coherent_quantum and the round keep different state words");
  C->drv = gg_coh_state::DRV_HOST;
  return GG_OK;
}

// the steps of quantum q on the owned shards (host-driven batches, one sync
// per batch to look at the quiet flag), then, enqueued without a sync: the
// step counters reset for the next quantum, the status kernel into
// C->status_dev = {active, blocked, min next start, -} and the run-info
// quantum count
static gg_status coh_quantum_steps(gg_ctx* ctx, uint64_t q)
{
  gg_coh_state* C = ctx->coh;
  if (C->has_barrier)
    return gg_fail(GG_ERR_UNSUPPORTED, "BARRIER records are released by gg_coherent_run and the round "
                                       "(gg_round_*, gg_coherent_run_ranks), not quantum by quantum");
  if (gg_status e = coh_host_driven(C)) return e;
  hipStream_t s = ctx->last_stream;
  const CP& P = C->P;
  const uint64_t quantum_ps = (uint64_t)ctx->cfg.quantum_ns * 1000ull;
  const uint64_t barrier = (q + 1) * quantum_ps;
  const bool hbh = P.net == GG_NET_EMESH_HOP_BY_HOP;
  uint32_t k = 0, batch = 8;
  for (;;) {
    for (uint32_t b = 0; b < batch; ++b, ++k) {
      timed_launch(ctx, C, s, 0, [&] { launch_step(P, step_args(C), C->step_lds, s, k, 0u, barrier); });
      if (hbh) {
        if (P.nsx) timed_launch(ctx, C, s, 1, [&] { launch_walk(C, s, P.nsx, C->wtx, k, 0); });
        if (P.nsy) timed_launch(ctx, C, s, 2, [&] { launch_walk(C, s, P.nsy, C->wty, k, 1); });
      }
    }
    GG_HIP(hipGetLastError());
    uint32_t quiet = 0, err = 0;
    GG_HIP(hipMemcpyAsync(&quiet, C->S.quiet, sizeof(uint32_t), hipMemcpyDeviceToHost, s));
    GG_HIP(hipMemcpyAsync(&err, ctx->err_dev, sizeof(uint32_t), hipMemcpyDeviceToHost, s));
    GG_HIP(hipStreamSynchronize(s));
    timed_harvest(C);
    if (err) return coh_check(ctx);
    if (quiet) break;
    if (batch < 64) batch *= 2;
  }
  // the next quantum starts from empty step counters (ring, quiet, imported packets)
  GG_HIP(hipMemsetAsync(C->S.ring, 0, sizeof(uint32_t) * 7, s));
  const uint64_t init[4] = {0, 0, ~0ull, 0};
  GG_HIP(hipMemcpyAsync(C->status_dev, init, sizeof(init), hipMemcpyHostToDevice, s));
  hipLaunchKernelGGL(k_c_status, dim3((P.L + 63) / 64), dim3(64), 0, s, P, C->S, C->status_dev);
  hipLaunchKernelGGL(k_c_ri_quantum, dim3(1), dim3(1), 0, s, C->S, q);
  GG_HIP(hipGetLastError());
  return GG_OK;
}

gg_status gg_coherent_quantum(gg_ctx* ctx, uint64_t q, gg_coherent_status* out)
{
  GG_NOT_ATAC(ctx, "gg_coherent_quantum");
  if (!ctx || !out) return gg_fail(GG_ERR_INVALID, "NULL argument");
  gg_coh_state* C = ctx->coh;
  if (!C || !C->begun) return gg_fail(GG_ERR_INVALID, "gg_coherent_begin first");
  hipSetDevice(ctx->device);
  hipStream_t s = ctx->last_stream;
  if (gg_status st = coh_quantum_steps(ctx, q)) return st;
  uint64_t res[4];
  uint32_t nb = 0;
  GG_HIP(hipMemcpyAsync(res, C->status_dev, sizeof(res), hipMemcpyDeviceToHost, s));
  GG_HIP(hipMemcpyAsync(&nb, C->S.bnd_cnt, sizeof(uint32_t), hipMemcpyDeviceToHost, s));
  GG_HIP(hipStreamSynchronize(s));
  out->steps = 0;
  out->boundary_msgs = nb;
  out->min_next_ps = res[2];
  out->active_tiles = (uint32_t)res[0];
  out->blocked_tiles = (uint32_t)res[1];
  return coh_check(ctx);
}

// ---- the exchange of gg_round_exchange (gg_round.hip), enqueued on the
// context's stream without a host sync.  Send slots: per destination rank r
// a header record (word 0 = count) and `region` records; the records held at
// the quantum boundary are scattered to the rank that owns their shard (export
// order inside a slot does not matter: import lists them by atomics and every
// consumer orders by the canonical keys).
// Steps [k0, k0 + n) of quantum q (host-indexed launches; the launches after
// the quantum's quiet step return at once)
gg_status gg_coh_steps_async(gg_ctx* ctx, uint64_t q, uint32_t k0, uint32_t n)
{
  gg_coh_state* C = ctx->coh;
  if (!C || !C->begun) return gg_fail(GG_ERR_INVALID, "gg_coherent_begin first");
  if (gg_status e = coh_host_driven(C)) return e;
  hipSetDevice(ctx->device);
  hipStream_t s = ctx->last_stream;
  const CP& P = C->P;
  const uint64_t barrier = (q + 1) * (uint64_t)ctx->cfg.quantum_ns * 1000ull;
  const bool hbh = P.net == GG_NET_EMESH_HOP_BY_HOP;
  for (uint32_t k = k0; k < k0 + n; ++k) {
    timed_launch(ctx, C, s, 0, [&] { launch_step(P, step_args(C), C->step_lds, s, k, 0u, barrier); });
    if (hbh) {
      if (P.nsx) timed_launch(ctx, C, s, 1, [&] { launch_walk(C, s, P.nsx, C->wtx, k, 0); });
      if (P.nsy) timed_launch(ctx, C, s, 2, [&] { launch_walk(C, s, P.nsy, C->wty, k, 1); });
    }
  }
  GG_HIP(hipGetLastError());
  return GG_OK;
}
gg_status gg_coh_round_tail(gg_ctx* ctx, gg_cmsg* slots, uint32_t world, uint32_t per_rank, uint64_t region,
                            uint32_t host_err, uint64_t* dv_own)
{
  gg_coh_state* C = ctx->coh;
  if (!C || !C->begun) return gg_fail(GG_ERR_INVALID, "gg_coherent_begin first");
  hipLaunchKernelGGL(k_c_round_tail, dim3(1), dim3(1024), 0, ctx->last_stream, C->P, C->S, slots, world, per_rank, region,
                     (const uint32_t*)ctx->err_dev, host_err, dv_own);
  GG_HIP(hipGetLastError());
  return GG_OK;
}
gg_status gg_coh_round_import(gg_ctx* ctx, uint64_t q, const gg_cmsg* send, const gg_cmsg* recv, uint32_t world,
                              uint32_t self, uint64_t region, uint64_t slot, const uint64_t* dv_all, uint64_t* counts)
{
  gg_coh_state* C = ctx->coh;
  if (!C || !C->begun) return gg_fail(GG_ERR_INVALID, "gg_coherent_begin first");
  hipStream_t s = ctx->last_stream;
  hipLaunchKernelGGL(k_c_round_commit, dim3(1), dim3(64), 0, s, C->P, C->S, q, dv_all, world);
  hipLaunchKernelGGL(k_c_round_import, dim3(64, world), dim3(256), 0, s, C->P, C->S, send, recv, world, self, region,
                     slot, dv_all, counts);
  GG_HIP(hipGetLastError());
  return GG_OK;
}
void gg_coh_harvest(gg_ctx* ctx) { if (ctx->coh) timed_harvest(ctx->coh); }

// import records [lo, min(count, hi)) of every received slot; `first`: the
// quantum's first import (the record pools of its first step start empty);
// nothing when *skip_if_dev != 0 (the round's reduced error flag)
gg_status gg_coh_import_slots(gg_ctx* ctx, const gg_cmsg* slots, uint32_t world, uint64_t region, uint64_t lo,
                              uint64_t hi, bool first, const uint64_t* skip_if_dev)
{
  gg_coh_state* C = ctx->coh;
  if (!C || !C->begun) return gg_fail(GG_ERR_INVALID, "gg_coherent_begin first");
  hipStream_t s = ctx->last_stream;
  if (first) GG_HIP(coh_pool_reset(C, s));
  hipLaunchKernelGGL(k_c_import_slots, dim3(64, world), dim3(256), 0, s, C->P, C->S, slots, region, lo, hi, skip_if_dev);
  GG_HIP(hipGetLastError());
  return GG_OK;
}

gg_status gg_coh_check(gg_ctx* ctx) { return coh_check(ctx); }
uint64_t gg_coh_generation(gg_ctx* ctx) { return ctx->coh ? ctx->coh->gen : 0; }
bool gg_coh_windowed(const gg_ctx* ctx) { return ctx && ctx->coh && ctx->coh->begun && ctx->coh->windowed; }

gg_status gg_coherent_export(gg_ctx* ctx, gg_cmsg* out_dev, uint64_t cap, uint64_t* per_shard_counts)
{
  GG_NOT_ATAC(ctx, "gg_coherent_export");
  if (!ctx || !per_shard_counts) return gg_fail(GG_ERR_INVALID, "NULL argument");
  gg_coh_state* C = ctx->coh;
  if (!C || !C->begun) return gg_fail(GG_ERR_INVALID, "gg_coherent_begin first");
  hipSetDevice(ctx->device);
  hipStream_t s = ctx->last_stream;
  const CP& P = C->P;
  uint32_t nb = 0;
  GG_HIP(hipMemcpy(&nb, C->S.bnd_cnt, sizeof(uint32_t), hipMemcpyDeviceToHost));
  if (nb > cap) return gg_fail(GG_ERR_RANGE, "export buffer holds %llu records, %u waiting",
                               (unsigned long long)cap, nb);
  if (nb && !out_dev) return gg_fail(GG_ERR_INVALID, "NULL export buffer");
  std::vector<uint32_t> counts(P.K, 0), base(P.K, 0);
  if (nb) {
    GG_HIP(hipMemsetAsync(C->ecount_dev, 0, sizeof(uint32_t) * 2 * P.K, s));
    hipLaunchKernelGGL(k_c_export_count, dim3((nb + 255) / 256), dim3(256), 0, s, C->S, C->S.bnd, nb, C->ecount_dev);
    GG_HIP(hipMemcpyAsync(counts.data(), C->ecount_dev, sizeof(uint32_t) * P.K, hipMemcpyDeviceToHost, s));
    GG_HIP(hipStreamSynchronize(s));
    uint32_t a = 0;
    for (uint32_t k = 0; k < P.K; ++k) { base[k] = a; a += counts[k]; }
    GG_HIP(hipMemcpyAsync(C->ecount_dev, base.data(), sizeof(uint32_t) * P.K, hipMemcpyHostToDevice, s));
    GG_HIP(hipMemsetAsync(C->ecount_dev + P.K, 0, sizeof(uint32_t) * P.K, s));
    hipLaunchKernelGGL(k_c_export_scatter, dim3((nb + 255) / 256), dim3(256), 0, s, C->S, C->S.bnd, nb,
                       C->ecount_dev, C->ecount_dev + P.K, out_dev);
    GG_HIP(hipGetLastError());
  }
  GG_HIP(hipMemsetAsync(C->S.bnd_cnt, 0, sizeof(uint32_t), s));
  GG_HIP(hipStreamSynchronize(s));
  for (uint32_t k = 0; k < P.K; ++k) per_shard_counts[k] = counts[k];
  return GG_OK;
}

gg_status gg_coherent_import(gg_ctx* ctx, const gg_cmsg* in_dev, uint64_t n)
{
  GG_NOT_ATAC(ctx, "gg_coherent_import");
  if (!ctx) return gg_fail(GG_ERR_INVALID, "NULL argument");
  gg_coh_state* C = ctx->coh;
  if (!C || !C->begun) return gg_fail(GG_ERR_INVALID, "gg_coherent_begin first");
  if (n == 0) return GG_OK;
  if (!in_dev) return gg_fail(GG_ERR_INVALID, "NULL import buffer");
  if (n > C->P.msg_cap) return gg_fail(GG_ERR_UNSUPPORTED, "import of %llu records beyond the step pool",
                                       (unsigned long long)n);
  hipSetDevice(ctx->device);
  hipStream_t s = ctx->last_stream;
  // the quantum's first step reads pool 1 (messages) and walks pool 0 (held packets)
  GG_HIP(coh_pool_reset(C, s));
  hipLaunchKernelGGL(k_c_import, dim3((uint32_t)((n + 255) / 256)), dim3(256), 0, s, C->P, C->S, in_dev, (uint32_t)n);
  GG_HIP(hipGetLastError());
  GG_HIP(hipStreamSynchronize(s));
  return coh_check(ctx);
}

// The device-driven loop from the context's current quantum state until the
// run is over or pauses (qend_pick: the next quantum >= QS_STOP); *done_out =
// QS_DONE at the end.  The launch index starts at 0 (QS_START = 0 after
// gg_coherent_begin and after coh_resume).  may_persist: small meshes take
// the persistent kernels; a leg with a finite stop takes the per-step launches.
static gg_status coh_drive(gg_ctx* ctx, bool may_persist, uint64_t* done_out)
{
  gg_coh_state* C = ctx->coh;
  hipStream_t s = ctx->last_stream;
  C->drv = gg_coh_state::DRV_DEVICE;
  gg_timer_begin(ctx, "coherent_run", s);
  // the quantum loop on the device (k_c_step's quantum_end): the host only
  // streams launches and looks at the run-over flag once per batch
  const CP& P = C->P;
  const bool hbh = P.net == GG_NET_EMESH_HOP_BY_HOP;
  uint32_t L = 0, batch = 16;
  // small meshes: the whole loop in persistent launches (k_c_persist), one
  // workgroup per owned tile, all resident (<= kPersistTiles << CUs)
  const char* np_env = getenv("GG_COH_NO_PERSIST");
  const char* nl_env = getenv("GG_COH_NO_LDS_CACHE");
  const bool plc = C->persist_lc && !(nl_env && atoi(nl_env));
  bool persist = may_persist && P.L <= kPersistTiles && !P.mosi && !P.shl2 && !(np_env && atoi(np_env));   // (no persistent MOSI / sh_l2 instance)
  // a windowed run: never (k_c_persist keeps a TraceWin across steps, has no
  // clean point for a hand-over, and its scheduler reads next_start's kNsFin,
  // which takes a tile at the end of a window for a finished one)
  if (C->windowed) persist = false;
  // a statistics trace: one more launch per slot, the scan, which returns at
  // once unless the slot ended a quantum with a sample due (gg_stats.hip); the
  // per-step launches on every mesh size (a persistent launch holds cache
  // state in LDS and runs many quanta: no point at which a scan could look)
  const bool strace = gg_stats_on(ctx);
  if (strace) persist = false;
  if (persist) {
    // the grid barrier needs every workgroup resident at once (a partitioned
    // device has fewer CUs): else the per-step launches
    const size_t lds = plc ? (size_t)P.cache_lds_off + P.cache_lds_bytes : std::max(C->walk_lds, C->step_lds);
    int per_cu = 0;
    if (persist_occupancy(plc, lds, &per_cu) != hipSuccess ||
        (uint64_t)per_cu * (uint64_t)ctx->num_cus < P.L)
      persist = false;
  }
  while (persist) {
    GG_HIP(hipMemsetAsync(C->S.gbar, 0, 4 * sizeof(uint32_t), s));   // counter + the three stop-vote words
    if (plc) {
      const size_t lds = P.cache_lds_off + P.cache_lds_bytes;
      timed_launch(ctx, C, s, 3, [&] { launch_persist(true, P, step_args(C), lds, s, L, L + kPersistLaunches); });
    } else {
      const size_t lds = std::max(C->walk_lds, C->step_lds);
      timed_launch(ctx, C, s, 3, [&] { launch_persist(false, P, step_args(C), lds, s, L, L + kPersistLaunches); });
    }
    GG_HIP(hipGetLastError());
    L += kPersistLaunches;
    uint64_t done = 0;
    uint32_t err = 0;
    GG_HIP(hipMemcpyAsync(&done, C->S.qs + QS_DONE, sizeof(done), hipMemcpyDeviceToHost, s));
    GG_HIP(hipMemcpyAsync(&err, ctx->err_dev, sizeof(err), hipMemcpyDeviceToHost, s));
    GG_HIP(hipStreamSynchronize(s));
    timed_harvest(C);
    if (err || done) break;
  }
  // hop-by-hop: the first walker launch of a slot ends the quantum when the
  // slot's step sent nothing (quantum_end_walk), so no launch is spent on the
  // quantum end; GG_COH_QEND_STEP=1 (A/B knob): the step launch after it does,
  // as for the closed-form networks (k_c_step's quantum_end)
  const char* qs_env = getenv("GG_COH_QEND_STEP");
  const bool qend_walk = hbh && !(qs_env && atoi(qs_env));
  for (; !persist;) {
    for (uint32_t b = 0; b < batch; ++b, ++L) {
      timed_launch(ctx, C, s, 0, [&] { launch_step(P, step_args(C), C->step_lds, s, L, 1u, (uint64_t)0); });
      if (hbh) {
        if (P.nsx) timed_launch(ctx, C, s, 1, [&] { launch_walk(C, s, P.nsx, C->wtx, L, 0, qend_walk); });
        if (P.nsy) timed_launch(ctx, C, s, 2, [&] { launch_walk(C, s, P.nsy, C->wty, L, 1, qend_walk && !P.nsx); });
      }
      if (strace) if (gg_status e = gg_stats_slot(ctx, s, L)) return e;
    }
    GG_HIP(hipGetLastError());
    uint64_t done = 0;
    uint32_t err = 0;
    GG_HIP(hipMemcpyAsync(&done, C->S.qs + QS_DONE, sizeof(done), hipMemcpyDeviceToHost, s));
    GG_HIP(hipMemcpyAsync(&err, ctx->err_dev, sizeof(err), hipMemcpyDeviceToHost, s));
    GG_HIP(hipStreamSynchronize(s));
    timed_harvest(C);
    if (err) break;
    if (done) break;
    if (batch < 256) batch *= 2;
  }
  gg_timer_end(ctx, "coherent_run", s);
  GG_HIP(hipStreamSynchronize(s));
  if (C->S.trs && getenv("GG_COH_TRACE_OUT")) {
    // raw dumps for tools/coh_trace.py: steps [n][L][16], walkers [n][2][wb][8] (u64)
    const std::string pre = getenv("GG_COH_TRACE_OUT");
    const size_t ns = (size_t)C->S.tr_n * P.L * kTrStep, nw = (size_t)C->S.tr_n * 2 * C->S.tr_wb * 8;
    std::vector<unsigned long long> h(std::max(ns, nw));
    for (int k = 0; k < 2; ++k) {
      const size_t cnt = k ? nw : ns;
      GG_HIP(hipMemcpy(h.data(), k ? C->S.trw : C->S.trs, 8 * cnt, hipMemcpyDeviceToHost));
      if (FILE* f = fopen((pre + (k ? ".walk" : ".step")).c_str(), "wb")) { fwrite(h.data(), 8, cnt, f); fclose(f); }
    }
    if (C->S.tre) {
      const size_t ne = (size_t)C->S.tre_n * 2 * C->S.tr_wb * (kTrEvMax * 4 + 4);
      std::vector<unsigned long long> he(ne);
      GG_HIP(hipMemcpy(he.data(), C->S.tre, 8 * ne, hipMemcpyDeviceToHost));
      if (FILE* f = fopen((pre + ".ev").c_str(), "wb")) { fwrite(he.data(), 8, ne, f); fclose(f); }
    }
    if (FILE* f = fopen((pre + ".meta").c_str(), "w")) {
      fprintf(f, "{\"launches\": %u, \"tiles\": %u, \"walk_blocks\": %u, \"nsx\": %u, \"nsy\": %u, \"wtx\": %u, \"wty\": %u, "
              "\"ev_first\": %u, \"ev_launches\": %u, \"ev_max\": %u}\n",
              C->S.tr_n, P.L, C->S.tr_wb, P.nsx, P.nsy, C->wtx, C->wty, kTrEv0, C->S.tre_n, kTrEvMax);
      fclose(f);
    }
  }
  if (C->S.prof) {
    // per-launch maxima in slots L mod 65536
    std::vector<unsigned long long> h(1024 + 8 * 65536);
    GG_HIP(hipMemcpy(h.data(), C->S.prof, sizeof(unsigned long long) * h.size(), hipMemcpyDeviceToHost));
    unsigned long long crit = 0, wx = 0, wy = 0;
    for (int i = 0; i < 65536; ++i) { crit += h[1024 + i]; wx += h[1024 + 65536 + 2 * i]; wy += h[1024 + 65536 + 2 * i + 1]; }
    fprintf(stderr, "[gg_coh] step cycles over tiles: self %llu inbox+handlers %llu (order %llu) trace %llu publish %llu "
            "writeback %llu | slowest tile per launch %llu\n"
            "[gg_coh] walkers: %llu launches, staging %llu events %llu loop %llu handoff %llu, max events X %llu Y %llu | "
            "slowest walker per launch X %llu Y %llu | sweep: batch %llu queue load %llu requests %llu store %llu (s_memtime cycles); requests fast %llu M/G/1 %llu search %llu\n",
            h[0], h[1], h[9], h[2], h[3], h[4], crit, h[22], h[16], h[19], h[17], h[18], h[24], h[25], wx, wy, h[26], h[27], h[28], h[29], h[30], h[31], h[32]);
    {
      unsigned long long mt = 0, mx = 0, my = 0;
      for (int i = 0; i < 65536; ++i) { mt += h[1024 + 3 * 65536 + i]; mx += h[1024 + 4 * 65536 + 2 * i]; my += h[1024 + 4 * 65536 + 2 * i + 1]; }
      fprintf(stderr, "[gg_coh] tiles with SELF arrivals: %llu; cycles prologue %llu, narv %llu, gather %llu, order %llu, queue load %llu, "
              "requests + store %llu | tiles without: %llu, prologue %llu\n", h[96], h[90], h[91], h[92], h[93], h[94], h[95], h[98], h[97]);
      fprintf(stderr, "[gg_coh] per-launch max requests summed: tile (self+sent) %llu walker X %llu Y %llu\n", mt, mx, my);
      fprintf(stderr, "[gg_coh] walkers: most packets in one run X %llu Y %llu; pipelined runs past 64 packets (a lane's second "
              "candidate; past 128 wave 0 sweeps) %llu\n", h[46], h[47], h[48]);
      fprintf(stderr, "[gg_coh] walkers, armed waits: arms %llu hits %llu (%.1f %% of %llu serves) misses %llu; "
              "same-bound continues %llu\n", h[100], h[101], h[19] ? 100.0 * (double)h[101] / (double)h[19] : 0.0, h[19],
              h[103], h[102]);
      unsigned long long sn = 0, sa = 0, ss = 0, c1 = 0, c2 = 0, c3 = 0, ct = 0, nl = 0;
      for (int i = 0; i < 16384; ++i) {
        const unsigned long long* b = &h[1024 + 6 * 65536 + 4 * i];
        if (!b[0]) continue;
        ++nl; ct += b[0] >> 24;
        sn += (b[0] >> 16) & 255; sa += (b[0] >> 8) & 255; ss += b[0] & 255;
        c1 += (b[1] & 0xFFFFFF) << 8; c2 += (b[2] & 0xFFFFFF) << 8; c3 += (b[3] & 0xFFFFFF) << 8;
      }
      fprintf(stderr, "[gg_coh] slowest tile per launch (%llu launches, last 16384 indices): cycles %llu; inbox msgs %llu, SELF arrivals %llu, "
              "sent %llu; cycles self-phase %llu inbox+handlers %llu trace %llu\n", nl, ct, sn, sa, ss, c1, c2, c3);
      const char* kn[3] = {"SELF", "injection", "walker"};
      for (int k = 0; k < 3; ++k)
        fprintf(stderr, "[gg_coh] %s batches, requests by size 1|2-3|4-7|8-15|16-31|32-63|64+: %llu %llu %llu %llu %llu %llu %llu; tail requests %llu\n",
                kn[k], h[50 + 8 * k], h[51 + 8 * k], h[52 + 8 * k], h[53 + 8 * k], h[54 + 8 * k], h[55 + 8 * k], h[56 + 8 * k], h[80 + k]);
    }
    fprintf(stderr, "[gg_coh] trace: hit runs %llu cycles for %llu records (%llu calls, look-up part %llu; %llu row updates: "
            "loop %llu stores %llu); other accesses %llu cycles for %llu\n",
            h[33], h[34], h[38], h[37] - h[39], h[42], h[40] - h[37] + 0, h[41] - h[40], h[35], h[36]);
  }
  if (gg_status e = coh_check(ctx)) return e;
  uint64_t done = 0;
  GG_HIP(hipMemcpy(&done, C->S.qs + QS_DONE, sizeof(done), hipMemcpyDeviceToHost));
  *done_out = done;
  if (done == 2) return gg_fail(GG_ERR_STATE, "coherent run deadlocked: tiles blocked with no message in flight");
  return GG_OK;
}

static gg_status coh_owns_all(const gg_ctx* ctx, gg_status code, const char* what)
{
  const gg_config& c = ctx->cfg;
  const uint32_t K = c.num_shards ? c.num_shards : 1;
  if (c.shard_begin != 0 || (c.shard_end != 0 && c.shard_end != K))
    return gg_fail(code, "%s needs a context that owns every shard", what);
  return GG_OK;
}

gg_status gg_coherent_run(gg_ctx* ctx, const gg_trace* tr, uint64_t* access_out_dev, void* stream)
{
  GG_NOT_ATAC(ctx, "gg_coherent_run");
  if (!ctx) return gg_fail(GG_ERR_INVALID, "NULL argument");
  if (gg_status st = coh_owns_all(ctx, GG_ERR_INVALID, "gg_coherent_run")) return st;
  if (gg_status st = gg_coherent_begin(ctx, tr, access_out_dev, stream)) return st;
  uint64_t done = 0;
  return coh_drive(ctx, true, &done);
}

// ---- gg_coherent_advance: the device-driven loop in legs ----
gg_status gg_coherent_advance(gg_ctx* ctx, uint64_t stop_quantum, uint64_t* next_quantum, int* done)
{
  GG_NOT_ATAC(ctx, "gg_coherent_advance");
  if (!ctx || !next_quantum || !done) return gg_fail(GG_ERR_INVALID, "NULL argument");
  if (gg_status st = coh_owns_all(ctx, GG_ERR_UNSUPPORTED, "gg_coherent_advance")) return st;
  gg_coh_state* C = ctx->coh;
  if (!C || !C->begun) return gg_fail(GG_ERR_INVALID, "gg_coherent_begin or gg_coherent_restore first");
  if (C->drv == gg_coh_state::DRV_HOST)
    return gg_fail(GG_ERR_INVALID, "this run is driven by gg_coherent_quantum / the round: gg_coherent_advance "
                                   "keeps different state words");
  hipSetDevice(ctx->device);
  hipStream_t s = ctx->last_stream;
  uint64_t qs[QS_N];
  GG_HIP(hipStreamSynchronize(s));
  GG_HIP(hipMemcpy(qs, C->S.qs, sizeof(qs), hipMemcpyDeviceToHost));
  *next_quantum = qs[QS_Q];
  *done = (int)(qs[QS_DONE] & 3);
  if (*done == 2) return gg_fail(GG_ERR_STATE, "coherent run deadlocked: tiles blocked with no message in flight");
  if (C->windowed) {
    // test knob: GG_WINDOW_FAIL_EXHAUSTED=1 sets the backstop's error bit on
    // the host, as qend_window does for a tile off a window that is not the
    // end of its trace (no tile is driven there); the run fails from here on
    const char* e = getenv("GG_WINDOW_FAIL_EXHAUSTED");
    if (e && atoi(e)) {
      uint32_t ew = 0;
      GG_HIP(hipMemcpy(&ew, ctx->err_dev, sizeof(ew), hipMemcpyDeviceToHost));
      ew |= GG_DERR_WINDOW;
      GG_HIP(hipMemcpy(ctx->err_dev, &ew, sizeof(ew), hipMemcpyHostToDevice));
    }
  }
  if (*done || stop_quantum <= qs[QS_Q]) return coh_check(ctx);   // over, or already there: no launch, no change
  if (C->windowed) {
    // the quantum to run next against the horizon the last quantum end or
    // hand-over left: windows already too short ask for the next ones at once
    uint64_t hor = 0;
    GG_HIP(hipMemcpy(&hor, C->win_dev + WN_HOR, sizeof(hor), hipMemcpyDeviceToHost));
    if ((qs[QS_Q] + 1) * qs[QS_QPS] > hor) { *done = GG_ADV_NEED_WINDOW; return coh_check(ctx); }
  }
  // resume: the launch index restarts at 0, so the quantum's step 0 is launch
  // 0 (k = L - QS_START) and no slot of the live ring is a step; the rest of
  // the quantum state, QS_REL (a barrier release for step 0) included, stays
  qs[QS_STOP] = stop_quantum; qs[QS_DONE] = 0; qs[QS_START] = 0;
  GG_HIP(hipMemcpyAsync(C->S.qs, qs, sizeof(qs), hipMemcpyHostToDevice, s));
  GG_HIP(hipMemsetAsync(C->S.live, 0, 4 * sizeof(uint32_t), s));
  GG_HIP(hipStreamSynchronize(s));                     // (qs is a stack array)
  uint64_t d = 0;
  const gg_status st = coh_drive(ctx, stop_quantum == ~0ull && !C->windowed, &d);   // (k_c_persist keeps a TraceWin across steps)
  *done = d == kQsWindow ? GG_ADV_NEED_WINDOW : (int)(d & 3);
  if (C->windowed && st != GG_OK && *done == 1) *done = 0;   // a failed windowed run is never reported over
  uint64_t q = 0;
  if (hipMemcpy(&q, C->S.qs + QS_Q, sizeof(q), hipMemcpyDeviceToHost) == hipSuccess) *next_quantum = q;
  return st;
}

// ---- a run fed its trace in windows -------------------------
// a window's offsets and final flags onto the device; the host-side checks
// both entries share
static gg_status win_upload(gg_ctx* ctx, const char* what, const gg_trace* win, const uint8_t* final_tiles, hipStream_t s)
{
  gg_coh_state* C = ctx->coh;
  const uint32_t T = C->P.T;
  if (win->tile_offsets[T] != win->num_records) return gg_fail(GG_ERR_INVALID, "%s: tile_offsets[num_tiles] != num_records", what);
  for (uint32_t t = 0; t < T; ++t)
    if (win->tile_offsets[t] > win->tile_offsets[t + 1]) return gg_fail(GG_ERR_INVALID, "%s: tile_offsets not monotone", what);
  if (win->num_records && (!win->addr_dev || !win->meta_dev)) return gg_fail(GG_ERR_INVALID, "%s: NULL trace pointers", what);
  if (!C->win_dev) {
    if (gg_status st = C->mem.alloc(&C->win_dev, (uint64_t)WN_HDR + (uint64_t)C->P.L * WN_TILE)) return st;
    if (gg_status st = C->mem.alloc(&C->win_fin_dev, (uint64_t)T)) return st;
    if (gg_status st = C->mem.alloc(&C->win_bad_dev, 2)) return st;
    if (gg_status st = C->mem.alloc(&C->win_state_dev, 2 * (uint64_t)T)) return st;
  }
  // (offs_dev is read by k_c_reset at begin only: between begins it stages a window's offsets)
  GG_HIP(hipMemcpyAsync(C->offs_dev, win->tile_offsets, sizeof(uint64_t) * (T + 1), hipMemcpyHostToDevice, s));
  if (final_tiles) GG_HIP(hipMemcpyAsync(C->win_fin_dev, final_tiles, T, hipMemcpyHostToDevice, s));
  else GG_HIP(hipMemsetAsync(C->win_fin_dev, 0, T, s));
  const uint32_t bad0[2] = {0u, ~0u};
  GG_HIP(hipMemcpyAsync(C->win_bad_dev, bad0, sizeof(bad0), hipMemcpyHostToDevice, s));
  GG_HIP(hipStreamSynchronize(s));                     // (the sources are the caller's and a stack array)
  return GG_OK;
}

gg_status gg_coherent_begin_window(gg_ctx* ctx, const gg_trace* win, uint64_t* access_out_dev, const uint8_t* final_tiles,
                                   void* stream)
{
  const char* const what = "gg_coherent_begin_window";
  GG_NOT_ATAC(ctx, what);
  if (!ctx || !win || !win->tile_offsets) return gg_fail(GG_ERR_INVALID, "%s: NULL argument", what);
  if (gg_status st = coh_owns_all(ctx, GG_ERR_UNSUPPORTED, what)) return st;
  hipSetDevice(ctx->device);
  if (gg_status st = coh_alloc(ctx)) return st;
  gg_coh_state* C = ctx->coh;
  if (C->P.lat_l1d == 0)
    return gg_fail(GG_ERR_UNSUPPORTED, "%s: with zero L1-D data cycles a record can cost no time, so no window "
                                       "bounds what a tile consumes in a quantum", what);
  for (uint32_t t = 0; t < C->P.T; ++t)
    if (win->tile_offsets[t] == win->tile_offsets[t + 1] && !(final_tiles && final_tiles[t]))
      return gg_fail(GG_ERR_INVALID, "%s: tile %u is not final and its window holds no record", what, t);
  hipStream_t s = (hipStream_t)stream;
  if (gg_status st = gg_coherent_begin(ctx, win, access_out_dev, stream)) return st;
  // from here a failure leaves no begun run: a begun run over the first
  // window alone would take the end of each window for the end of a trace
  auto install = [&]() -> gg_status {
    if (gg_status st = win_upload(ctx, what, win, final_tiles, s)) return st;
    cs_set(C->S.win, C->win_dev);
    const uint64_t w0[WN_HDR] = {~0ull, ~0ull};
    GG_HIP(hipMemcpyAsync(C->win_dev, w0, sizeof(w0), hipMemcpyHostToDevice, s));
    GG_HIP(hipMemcpyAsync(C->Sd, &C->S, sizeof(CS), hipMemcpyHostToDevice, s));
    launch_window_install(C->P, C->S, win->addr_dev, win->meta_dev, C->offs_dev, C->win_fin_dev, 0, C->win_bad_dev, s);
    GG_HIP(hipGetLastError());
    GG_HIP(hipStreamSynchronize(s));
    return GG_OK;
  };
  if (gg_status st = install()) { C->begun = false; C->windowed = false; C->S.win = nullptr; return st; }
  C->windowed = true;
  C->drv = gg_coh_state::DRV_DEVICE;                 // only gg_coherent_advance drives a windowed run
  return GG_OK;
}

gg_status gg_coherent_next_window(gg_ctx* ctx, const gg_trace* win, uint64_t* access_out_dev, const uint8_t* final_tiles,
                                  void* stream)
{
  const char* const what = "gg_coherent_next_window";
  GG_NOT_ATAC(ctx, what);
  if (!ctx || !win || !win->tile_offsets) return gg_fail(GG_ERR_INVALID, "%s: NULL argument", what);
  gg_coh_state* C = ctx->coh;
  if (!C || !C->begun || !C->windowed) return gg_fail(GG_ERR_INVALID, "%s: gg_coherent_begin_window first", what);
  hipSetDevice(ctx->device);
  hipStream_t s = (hipStream_t)stream;
  GG_HIP(hipStreamSynchronize(ctx->last_stream));
  uint64_t done = 0;
  uint32_t err = 0;
  GG_HIP(hipMemcpy(&done, C->S.qs + QS_DONE, sizeof(done), hipMemcpyDeviceToHost));
  GG_HIP(hipMemcpy(&err, ctx->err_dev, sizeof(err), hipMemcpyDeviceToHost));
  if ((done & 3) || err)
    return gg_fail(GG_ERR_INVALID, "%s: the run is not at the device loop's clean point (it is over or has failed); "
                                   "a window goes in after begin or a paused gg_coherent_advance", what);
  if (gg_status st = win_upload(ctx, what, win, final_tiles, s)) return st;
  launch_window_install(C->P, C->S, win->addr_dev, win->meta_dev, C->offs_dev, C->win_fin_dev, 1, C->win_bad_dev, s);
  GG_HIP(hipGetLastError());
  uint32_t bad[2] = {0, 0};
  GG_HIP(hipMemcpyAsync(bad, C->win_bad_dev, sizeof(bad), hipMemcpyDeviceToHost, s));
  GG_HIP(hipStreamSynchronize(s));
  if (bad[0]) {
    const uint32_t t = bad[1] - 1;
    const char* why = (bad[0] & WB_STATE)  ? "a tile stands past the end of its window"
                    : (bad[0] & WB_EMPTY)  ? "an unfinished tile's window holds no record"
                    : (bad[0] & WB_RECORD) ? "a window's first record is not the record its tile stands on (addr or meta)"
                    : (bad[0] & WB_FINAL)  ? "a final tile made non-final, or with another number of records left"
                                           : "a finished tile's range is not empty";
    return gg_fail(GG_ERR_INVALID, "%s: %s (first at tile %u); nothing changed", what, why, t);
  }
  const uint64_t hor0 = ~0ull;
  GG_HIP(hipMemcpyAsync(C->win_dev + WN_HOR, &hor0, sizeof(hor0), hipMemcpyHostToDevice, s));
  launch_window_install(C->P, C->S, win->addr_dev, win->meta_dev, C->offs_dev, C->win_fin_dev, 2, C->win_bad_dev, s);
  GG_HIP(hipGetLastError());
  cs_set(C->S.addr, win->addr_dev); cs_set(C->S.meta, win->meta_dev); cs_set(C->S.out, access_out_dev);
  GG_HIP(hipMemcpyAsync(C->Sd, &C->S, sizeof(CS), hipMemcpyHostToDevice, s));
  GG_HIP(hipStreamSynchronize(s));                     // the old arrays are the caller's again
  C->n_records = win->num_records;
  C->offs_host.assign(win->tile_offsets, win->tile_offsets + C->P.T + 1);
  ctx->last_stream = s;
  return GG_OK;
}

gg_status gg_coherent_window_state(gg_ctx* ctx, uint64_t* consumed, uint64_t* min_records)
{
  const char* const what = "gg_coherent_window_state";
  GG_NOT_ATAC(ctx, what);
  if (!ctx) return gg_fail(GG_ERR_INVALID, "%s: NULL argument", what);
  gg_coh_state* C = ctx->coh;
  if (!C || !C->begun || !C->windowed) return gg_fail(GG_ERR_INVALID, "%s: gg_coherent_begin_window first", what);
  hipSetDevice(ctx->device);
  hipStream_t s = ctx->last_stream;
  const uint32_t T = C->P.T;
  GG_HIP(hipMemsetAsync(C->win_state_dev, 0, sizeof(uint64_t) * 2 * T, s));
  launch_window_state(C->P, C->S, C->win_state_dev, C->win_state_dev + T, s);
  GG_HIP(hipGetLastError());
  GG_HIP(hipStreamSynchronize(s));
  if (consumed) GG_HIP(hipMemcpy(consumed, C->win_state_dev, sizeof(uint64_t) * T, hipMemcpyDeviceToHost));
  if (min_records) GG_HIP(hipMemcpy(min_records, C->win_state_dev + T, sizeof(uint64_t) * T, hipMemcpyDeviceToHost));
  return GG_OK;
}

// ---- gg_coherent_run_many: independent runs side by side in one set of
// launches.  What fixes the shape of an ensemble launch —
// grids, block sizes, kernel variants — must be the same in every context;
// it is read from the derived launch state, so any two configs that derive
// the same shape go together.  Returns the first field that differs.
static const char* many_mismatch(const gg_ctx* a, const gg_ctx* b)
{
  const gg_coh_state *A = a->coh, *B = b->coh;
  const CP &p = A->P, &q = B->P;
  if (a->device != b->device) return "device";
  if (p.T != q.T) return "num_tiles";
  if (p.K != q.K) return "num_shards";
  if (p.mosi != q.mosi || p.shl2 != q.shl2 || p.mesi != q.mesi) return "protocol";
  if (p.net != q.net) return "net_model";
  if (p.L != q.L) return "owned tiles";
  if (p.fast != q.fast) return "step kernel variant (register queues and no miss types, or the general form)";
  if (p.nsx != q.nsx || p.nsy != q.nsy) return "walker run counts";
  if (p.nsx + p.nsy && walk_regq(p) != walk_regq(q)) return "walker kernel variant (register queues)";
  if (p.nsx + p.nsy && (A->wtx != B->wtx || A->wty != B->wty)) return "walker block sizes";
  return nullptr;
}

// What gg_coherent_run_many and gg_coherent_advance_many ask of their set,
// after n and the argument pointers: no NULL or repeated context, no ATAC
// context, every shard owned (shard_code: the status of a context that does
// not), then, for advance_many, a begun run of the device loop in each, and
// launch compatibility.  Nothing is launched and no run state changes (a
// context that has not run yet gets its derived launch state: allocation
// only, as gg_coherent_begin's first call).
static gg_status many_validate(const char* what, gg_ctx* const* ctxs, uint32_t n, gg_status shard_code, bool need_begun)
{
  {
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
  }
  for (uint32_t i = 0; i < n; ++i) {
    if (!need_begun) GG_NOT_ATAC(ctxs[i], what);      // (gg_coherent_run_many's wording stays)
    char who[64];
    snprintf(who, sizeof(who), "%s: context %u", what, i);
    GG_NOT_ATAC(ctxs[i], who);
  }
  for (uint32_t i = 0; i < n; ++i) {
    const gg_config& c = ctxs[i]->cfg;
    const uint32_t K = c.num_shards ? c.num_shards : 1;
    if (c.shard_begin != 0 || (c.shard_end != 0 && c.shard_end != K))
      return gg_fail(shard_code, "%s: context %u does not own every shard (shard range [%u, %u) of %u)",
                     what, i, c.shard_begin, c.shard_end, K);
  }
  for (uint32_t i = 0; i < n; ++i)
    if (gg_coh_windowed(ctxs[i]))
      return gg_fail(GG_ERR_UNSUPPORTED, "%s: context %u has a run fed in windows (gg_coherent_begin_window): "
                                         "gg_coherent_advance and gg_coherent_next_window drive it", what, i);
  if (need_begun)
    for (uint32_t i = 0; i < n; ++i) {
      const gg_coh_state* C = ctxs[i]->coh;
      if (!C || !C->begun)
        return gg_fail(GG_ERR_INVALID, "%s: context %u: gg_coherent_begin or gg_coherent_restore first", what, i);
      if (C->drv == gg_coh_state::DRV_HOST)
        return gg_fail(GG_ERR_INVALID, "%s: context %u: this run is driven by gg_coherent_quantum / the round: "
                                       "gg_coherent_advance keeps different state words", what, i);
    }
  for (uint32_t i = 0; i < n; ++i) {
    hipSetDevice(ctxs[i]->device);
    if (gg_status st = coh_alloc(ctxs[i])) return st;
  }
  for (uint32_t i = 1; i < n; ++i)
    if (const char* f = many_mismatch(ctxs[0], ctxs[i]))
      return gg_fail(GG_ERR_INVALID, "%s: context %u differs from context 0 in %s", what, i, f);
  return GG_OK;
}

// the driver's buffers, kept by the set's first context: [n] pairs, [n] poll
// words and [n] scan records (gg_stats.h), device and pinned host
static gg_status many_reserve(gg_coh_state* C0, uint32_t n)
{
  const uint64_t bytes = (uint64_t)n * (sizeof(ManyPair) + sizeof(ManyPoll) + gg_stats_many_bytes());
  return gg_reserve_all(bytes, bytes, C0->many_dev, C0->many_host);
}

// The ensemble's driver loop (gg_coherent_run_many after its begins,
// gg_coherent_advance_many after its resumes): the instances in live, each at
// launch index 0 of a begun run (QS_START = 0), in one set of launches on s
// until each is over, paused or failed.  stv[i] comes in as GG_OK for the
// live instances and goes out as what gg_coherent_run / _advance would return;
// the others are not touched.  many_reserve(ctxs[0]->coh, n) has been called.
static void many_drive(gg_ctx* const* ctxs, uint32_t n, std::vector<uint32_t> live, hipStream_t s, std::vector<gg_status>& stv)
{
  gg_ctx* c0 = ctxs[0];
  gg_coh_state* C0 = c0->coh;
  hipSetDevice(c0->device);
  ManyPair* pairs_d = reinterpret_cast<ManyPair*>(C0->many_dev.get());
  ManyPoll* poll_d = (ManyPoll*)(pairs_d + n);
  uint8_t* recs_d = (uint8_t*)(poll_d + n);
  ManyPair* pairs_h = reinterpret_cast<ManyPair*>(C0->many_host.get());
  ManyPoll* poll_h = (ManyPoll*)(pairs_h + n);
  uint8_t* recs_h = (uint8_t*)(poll_h + n);
  const size_t rec = gg_stats_many_bytes();

  std::vector<uint64_t> done(n, 0);
  std::vector<uint32_t> err(n, 0);
  size_t walk_lds = 0, step_lds = 0;
  for (uint32_t i = 0; i < n; ++i) {
    walk_lds = std::max(walk_lds, ctxs[i]->coh->walk_lds);
    step_lds = std::max(step_lds, ctxs[i]->coh->step_lds);
  }
  const CP& P = C0->P;                              // the shared launch shape
  const bool hbh = P.net == GG_NET_EMESH_HOP_BY_HOP;
  // every instance lays its LDS out from its own CP inside its own size: the
  // launch takes the largest (the sizes need not match)
  gg_status hip_st = GG_OK;
  auto hip = [&](hipError_t e, const char* what) { if (e != hipSuccess && hip_st == GG_OK) hip_st = gg_hip_check(e, what); return e == hipSuccess; };
  if (!live.empty()) {
    hip(step_many_set_lds(step_lds), "hipFuncSetAttribute(k_c_step_many)");
    if (hbh) hip(walk_many_set_lds(walk_lds), "hipFuncSetAttribute(k_c_walk_many)");
  }
  gg_timer_begin(c0, "coherent_run", s);
  // per-step launches only: the persistent kernel's grid barrier needs every
  // workgroup of every instance resident at once (no ensemble form).  After
  // each batch the instances that finished, paused or failed leave the live
  // list.
  uint32_t L = 0, batch = 16;
  while (!live.empty() && hip_st == GG_OK) {
    const uint32_t m = (uint32_t)live.size();
    // a statistics trace in a live instance (gg_coherent_advance_many only):
    // one more launch per slot, the scan for all of them (gg_stats.hip)
    uint32_t st_bits = 0;
    for (uint32_t j = 0; j < m; ++j) {
      pairs_h[j] = ManyPair{ctxs[live[j]]->coh->Pd, ctxs[live[j]]->coh->Sd};
      st_bits |= gg_stats_run_bits(ctxs[live[j]]);
    }
    if (!hip(hipMemcpyAsync(pairs_d, pairs_h, sizeof(ManyPair) * m, hipMemcpyHostToDevice, s), "hipMemcpyAsync(live list)")) break;
    if (st_bits) {
      for (uint32_t j = 0; j < m; ++j) gg_stats_many_fill(ctxs[live[j]], ctxs[live[j]]->coh->S, recs_h + rec * j);
      if (!hip(hipMemcpyAsync(recs_d, recs_h, rec * m, hipMemcpyHostToDevice, s), "hipMemcpyAsync(scan records)")) break;
    }
    const size_t scan_lds = (st_bits & GG_ST_CACHE_LINE_REPLICATION) ? sizeof(uint32_t) * ((size_t)P.T + 1) : 0;
    for (uint32_t b = 0; b < batch; ++b, ++L) {
      launch_step_many(P, pairs_d, m, step_lds, s, L);
      if (hbh) {
        if (P.nsx) launch_walk_many(C0->wtx > 64, walk_regq(P), P.nsx, C0->wtx, pairs_d, m, walk_lds, s, L, 0);
        if (P.nsy) launch_walk_many(C0->wty > 64, walk_regq(P), P.nsy, C0->wty, pairs_d, m, walk_lds, s, L, 1);
      }
      if (st_bits) gg_stats_many_slot(pairs_d, recs_d, P.L, m, scan_lds, s, L);
    }
    hipLaunchKernelGGL(k_many_poll, dim3((m + 63) / 64), dim3(64), 0, s, (const ManyPair*)pairs_d, m, poll_d);
    if (!hip(hipGetLastError(), "ensemble launches")) break;
    if (!hip(hipMemcpyAsync(poll_h, poll_d, sizeof(ManyPoll) * m, hipMemcpyDeviceToHost, s), "hipMemcpyAsync(poll)")) break;
    if (!hip(hipStreamSynchronize(s), "hipStreamSynchronize")) break;
    std::vector<uint32_t> next;
    for (uint32_t j = 0; j < m; ++j) {
      const uint32_t i = live[j];
      done[i] = poll_h[j].done; err[i] = poll_h[j].err;
      if (!err[i] && !done[i]) next.push_back(i);
    }
    live.swap(next);
    if (batch < 256) batch *= 2;
  }
  gg_timer_end(c0, "coherent_run", s);
  if (hip_st == GG_OK) hip(hipStreamSynchronize(s), "hipStreamSynchronize");
  for (uint32_t i : live) stv[i] = hip_st;            // (only a HIP failure leaves instances live)
  for (uint32_t i = 0; i < n; ++i) {
    if (stv[i] != GG_OK) continue;
    if (err[i]) stv[i] = coh_check(ctxs[i]);
    else if (done[i] == 2)
      stv[i] = gg_fail(GG_ERR_STATE, "coherent run deadlocked: tiles blocked with no message in flight (instance %u)", i);
  }
}

gg_status gg_coherent_run_many(gg_ctx* const* ctxs, uint32_t n, const gg_trace* traces, uint64_t* const* access_out_dev,
                               gg_status* statuses, void* stream)
{
  // every rejection comes before a launch or a change of any context's run state
  if (n == 0) return gg_fail(GG_ERR_INVALID, "gg_coherent_run_many: n == 0");
  if (n > GG_MANY_MAX) return gg_fail(GG_ERR_INVALID, "gg_coherent_run_many: n = %u above GG_MANY_MAX = %u", n, (unsigned)GG_MANY_MAX);
  if (!ctxs || !traces) return gg_fail(GG_ERR_INVALID, "gg_coherent_run_many: NULL argument");
  // (a traced sweep: gg_coherent_begin per context, then gg_coherent_advance_many)
  for (uint32_t i = 0; i < n; ++i)
    if (ctxs[i] && gg_stats_on(ctxs[i]))
      return gg_fail(GG_ERR_UNSUPPORTED, "gg_coherent_run_many: context %u has a statistics trace configured "
                                         "(gg_coherent_run samples; turn it off with gg_stats_trace_configure(ctx, 0, 0, 0))", i);
  if (gg_status st = many_validate("gg_coherent_run_many", ctxs, n, GG_ERR_INVALID, false)) return st;
  if (gg_status st = many_reserve(ctxs[0]->coh, n)) return st;

  std::vector<gg_status> stv(n, GG_OK);
  std::vector<uint32_t> live;
  for (uint32_t i = 0; i < n; ++i) {
    stv[i] = gg_coherent_begin(ctxs[i], &traces[i], access_out_dev ? access_out_dev[i] : nullptr, stream);
    if (stv[i] == GG_OK) live.push_back(i);
  }
  many_drive(ctxs, n, live, (hipStream_t)stream, stv);
  gg_status first = GG_OK;
  for (uint32_t i = 0; i < n; ++i) {
    if (statuses) statuses[i] = stv[i];
    if (first == GG_OK) first = stv[i];
  }
  return first;
}

// ---- gg_coherent_advance_many: the ensemble in legs, and with statistics
// traces: gg_coherent_advance's resume per
// instance, then the driver loop above
gg_status gg_coherent_advance_many(gg_ctx* const* ctxs, uint32_t n, const uint64_t* stop_quanta, uint64_t* next_quanta,
                                   int* dones, gg_status* statuses, void* stream)
{
  const char* const what = "gg_coherent_advance_many";
  // every rejection comes before a launch or a write to any context's state
  if (n == 0) return gg_fail(GG_ERR_INVALID, "%s: n == 0", what);
  if (n > GG_MANY_MAX) return gg_fail(GG_ERR_INVALID, "%s: n = %u above GG_MANY_MAX = %u", what, n, (unsigned)GG_MANY_MAX);
  if (!ctxs || !next_quanta || !dones) return gg_fail(GG_ERR_INVALID, "%s: NULL argument", what);
  if (gg_status st = many_validate(what, ctxs, n, GG_ERR_UNSUPPORTED, true)) return st;
  if (gg_status st = many_reserve(ctxs[0]->coh, n)) return st;

  hipStream_t s = (hipStream_t)stream;
  std::vector<gg_status> stv(n, GG_OK);
  std::vector<uint32_t> live;
  // begin or restore may have used another stream: each context's own first,
  // then its quantum state (what gg_coherent_advance looks at)
  std::vector<uint64_t> qs((size_t)n * QS_N);
  for (uint32_t i = 0; i < n; ++i) {
    hipSetDevice(ctxs[i]->device);
    GG_HIP(hipStreamSynchronize(ctxs[i]->last_stream));
    GG_HIP(hipMemcpy(&qs[(size_t)i * QS_N], ctxs[i]->coh->S.qs, sizeof(uint64_t) * QS_N, hipMemcpyDeviceToHost));
  }
  for (uint32_t i = 0; i < n; ++i) {
    uint64_t* q = &qs[(size_t)i * QS_N];
    gg_coh_state* C = ctxs[i]->coh;
    const uint64_t stop = stop_quanta ? stop_quanta[i] : ~0ull;
    next_quanta[i] = q[QS_Q];
    dones[i] = (int)(q[QS_DONE] & 3);
    // over, or already there: no launch, no change, not in the live list
    if (dones[i] == 2) { stv[i] = gg_fail(GG_ERR_STATE, "coherent run deadlocked: tiles blocked with no message in flight (instance %u)", i); continue; }
    if (dones[i] || stop <= q[QS_Q]) { stv[i] = coh_check(ctxs[i]); continue; }
    // resume as gg_coherent_advance: the launch index restarts at 0 for all
    // of them together (one L, §4f); QS_REL stays
    q[QS_STOP] = stop; q[QS_DONE] = 0; q[QS_START] = 0;
    GG_HIP(hipMemcpyAsync(C->S.qs, q, sizeof(uint64_t) * QS_N, hipMemcpyHostToDevice, s));
    GG_HIP(hipMemsetAsync(C->S.live, 0, 4 * sizeof(uint32_t), s));
    ctxs[i]->last_stream = s;
    C->drv = gg_coh_state::DRV_DEVICE;
    live.push_back(i);
  }
  GG_HIP(hipStreamSynchronize(s));                    // (qs is this call's)
  const std::vector<uint32_t> ran = live;
  many_drive(ctxs, n, live, s, stv);
  for (uint32_t i : ran) {
    uint64_t w[3] = {0, 0, 0};                         // QS_Q, QS_START, QS_DONE
    if (hipMemcpy(w, ctxs[i]->coh->S.qs + QS_Q, sizeof(w), hipMemcpyDeviceToHost) != hipSuccess) continue;
    next_quanta[i] = w[QS_Q];
    dones[i] = (int)(w[QS_DONE] & 3);
  }
  gg_status first = GG_OK;
  for (uint32_t i = 0; i < n; ++i) {
    if (statuses) statuses[i] = stv[i];
    if (first == GG_OK) first = stv[i];
  }
  return first;
}

gg_status gg_coherent_get_miss_types(gg_ctx* ctx, uint64_t* out)
{
  if (!ctx || !out) return gg_fail(GG_ERR_INVALID, "NULL argument");
  gg_coh_state* C = ctx->coh;
  if (!C) return gg_fail(GG_ERR_INVALID, "no coherent run on this context");
  hipSetDevice(ctx->device);
  const CP& P = C->P;
  const size_t per = 2 * GG_NUM_MISS_TYPES;
  std::memset(out, 0, sizeof(uint64_t) * P.T * per);
  if (!C->S.mtc) return GG_OK;
  GG_HIP(hipStreamSynchronize(ctx->last_stream));
  std::vector<uint64_t> v((size_t)P.L * per);
  std::vector<uint32_t> gtile(P.L);
  GG_HIP(hipMemcpy(v.data(), C->S.mtc, sizeof(uint64_t) * v.size(), hipMemcpyDeviceToHost));
  GG_HIP(hipMemcpy(gtile.data(), C->S.gtile, sizeof(uint32_t) * P.L, hipMemcpyDeviceToHost));
  for (uint32_t l = 0; l < P.L; ++l)
    std::memcpy(out + (size_t)gtile[l] * per, v.data() + (size_t)l * per, sizeof(uint64_t) * per);
  return coh_check(ctx);
}

gg_status gg_coherent_get_protocol_stats(gg_ctx* ctx, uint64_t* out)
{
  if (!ctx || !out) return gg_fail(GG_ERR_INVALID, "NULL argument");
  gg_coh_state* C = ctx->coh;
  if (!C) return gg_fail(GG_ERR_INVALID, "no coherent run on this context");
  hipSetDevice(ctx->device);
  const CP& P = C->P;
  std::memset(out, 0, sizeof(uint64_t) * P.T * GG_NUM_PROTO_STATS);
  if (!C->S.ps) return GG_OK;                        // MSI: no MOSI counters
  GG_HIP(hipStreamSynchronize(ctx->last_stream));
  std::vector<uint64_t> v((size_t)P.L * GG_NUM_PROTO_STATS);
  std::vector<uint32_t> gtile(P.L);
  GG_HIP(hipMemcpy(v.data(), C->S.ps, sizeof(uint64_t) * v.size(), hipMemcpyDeviceToHost));
  GG_HIP(hipMemcpy(gtile.data(), C->S.gtile, sizeof(uint32_t) * P.L, hipMemcpyDeviceToHost));
  for (uint32_t l = 0; l < P.L; ++l)
    std::memcpy(out + (size_t)gtile[l] * GG_NUM_PROTO_STATS, v.data() + (size_t)l * GG_NUM_PROTO_STATS,
                sizeof(uint64_t) * GG_NUM_PROTO_STATS);
  return coh_check(ctx);
}

gg_status gg_coherent_get_stats(gg_ctx* ctx, uint64_t* tile_stats, uint64_t* cache, uint64_t* run_info)
{
  if (!ctx) return gg_fail(GG_ERR_INVALID, "NULL argument");
  gg_coh_state* C = ctx->coh;
  if (!C) return gg_fail(GG_ERR_INVALID, "no coherent run on this context");
  hipSetDevice(ctx->device);
  hipStream_t s = ctx->last_stream;
  const CP& P = C->P;
  hipLaunchKernelGGL(k_c_final_stats, dim3((P.L + 63) / 64), dim3(64), 0, s, P, C->S);
  GG_HIP(hipGetLastError());
  GG_HIP(hipStreamSynchronize(s));
  std::vector<uint32_t> gtile(P.L);
  GG_HIP(hipMemcpy(gtile.data(), C->S.gtile, sizeof(uint32_t) * P.L, hipMemcpyDeviceToHost));
  if (tile_stats) {
    std::vector<uint64_t> v((size_t)P.L * GG_NUM_TILE_STATS);
    GG_HIP(hipMemcpy(v.data(), C->S.st, sizeof(uint64_t) * v.size(), hipMemcpyDeviceToHost));
    std::memset(tile_stats, 0, sizeof(uint64_t) * P.T * GG_NUM_TILE_STATS);
    for (uint32_t l = 0; l < P.L; ++l)
      std::memcpy(tile_stats + (size_t)gtile[l] * GG_NUM_TILE_STATS, v.data() + (size_t)l * GG_NUM_TILE_STATS,
                  sizeof(uint64_t) * GG_NUM_TILE_STATS);
  }
  if (cache) {
    const size_t per = 2 * GG_NUM_CACHE_COUNTERS;
    std::vector<uint64_t> v((size_t)P.L * per);
    GG_HIP(hipMemcpy(v.data(), C->S.cc, sizeof(uint64_t) * v.size(), hipMemcpyDeviceToHost));
    std::memset(cache, 0, sizeof(uint64_t) * P.T * per);
    for (uint32_t l = 0; l < P.L; ++l)
      std::memcpy(cache + (size_t)gtile[l] * per, v.data() + (size_t)l * per, sizeof(uint64_t) * per);
  }
  if (run_info) GG_HIP(hipMemcpy(run_info, C->S.ri, sizeof(uint64_t) * GG_NUM_RUN_INFO, hipMemcpyDeviceToHost));
  return coh_check(ctx);
}

// ---------------------------------------------------------------------------
// snapshot / restore (the container: gg_snapshot.h; the packed
// sections: gg_snapshot.hip)
// ---------------------------------------------------------------------------
static_assert(sizeof(CP) == 48 * 4 + 8 * 8 + sizeof(NocParams) && sizeof(NocParams) == 12 * 4 + 8,
              "the launch state is compared byte for byte: no padding");
namespace {
// the derived launch state a snapshot must meet again: CP and what coh_alloc
// derives beside it (env knobs included: they change P or these)
struct SnapLaunch { CP P; uint64_t wtx, wty, persist_lc, step_lds, walk_lds, diag; };
SnapLaunch snap_launch(const gg_coh_state* C)
{
  SnapLaunch l;
  std::memset(&l, 0, sizeof(l));
  l.P = C->P; l.wtx = C->wtx; l.wty = C->wty; l.persist_lc = C->persist_lc; l.step_lds = C->step_lds;
  l.walk_lds = C->walk_lds; l.diag = GG_COH_DIAG;
  return l;
}
// the packed sections: directory, replaced list, cache tags, miss-type tables
struct SnapPacked { const char* name; PackSrc src; };
std::vector<SnapPacked> snap_packed(const gg_coh_state* C)
{
  const CP& P = C->P; const CS& S = C->S;
  std::vector<SnapPacked> v;
  const uint32_t rw = 3 + P.W + (P.mosi ? 1u : 0u);
  v.push_back({"dir", PackSrc{(void*)S.dir, (uint64_t*)S.dsh, P.mosi ? (uint64_t*)S.drng : nullptr, nullptr, P.L, P.E, P.W, PK_DIR, rw}});
  v.push_back({"rep", PackSrc{(void*)S.rep, (uint64_t*)S.rsh, P.mosi ? (uint64_t*)S.rrng : nullptr, (const TileSt*)S.ts, P.L, P.R, P.W, PK_REP, rw}});
  v.push_back({"l1_tag", PackSrc{(void*)S.l1_tag, nullptr, nullptr, nullptr, P.L, P.s1 * P.a1, 0, PK_TAB, 2}});
  v.push_back({"l2_tag", PackSrc{(void*)S.l2_tag, nullptr, nullptr, nullptr, P.L, P.s2 * P.a2, 0, PK_TAB, 2}});
  if (S.mtab) v.push_back({"mtab", PackSrc{(void*)S.mtab, nullptr, nullptr, nullptr, P.L, 2u << P.mt_log, 0, PK_TAB, 2}});
  return v;
}
// the live counts of the prefix sections, from the count arrays (host copies)
struct SnapCounts { uint32_t npool[2], bnd; std::vector<uint32_t> nxl, nyl; };
uint64_t list_words(const std::vector<uint32_t>& n, uint32_t cap)
{
  uint64_t t = 0;
  for (uint32_t c : n) t += std::min(c, cap);
  return t;
}
const gg_coh_state::Arr* find_arr(const gg_coh_state* C, const char* name)
{
  for (const gg_coh_state::Arr& a : C->arrs) if (!std::strcmp(a.name, name)) return &a;
  return nullptr;
}
gg_status snap_valid(gg_ctx* ctx, const char* what)
{
  GG_NOT_ATAC(ctx, what);
  gg_coh_state* C = ctx->coh;
  if (!C || !C->begun) return gg_fail(GG_ERR_INVALID, "%s: gg_coherent_begin or gg_coherent_restore first", what);
  if (gg_status st = coh_owns_all(ctx, GG_ERR_UNSUPPORTED, what)) return st;
  if (C->windowed)
    return gg_fail(GG_ERR_UNSUPPORTED, "%s: a run fed in windows (gg_coherent_begin_window) has no snapshot: "
                                       "the trace it continues on is not there yet", what);
  if (C->drv == gg_coh_state::DRV_HOST)
    return gg_fail(GG_ERR_INVALID, "%s: a run driven by gg_coherent_quantum / the round is not at the device loop's "
                                   "clean point (after begin, an advance or a restore)", what);
  return GG_OK;
}
}  // namespace

// The records live at a quantum boundary and the lists that hold them, on the
// host.  quantum_end delivers the held records by atomics, so their pool
// slots and their order inside a list differ from run to run (every consumer
// orders by the canonical keys: the results do not).  A snapshot stores the
// canonical form — each list sorted by its records' bytes, the records packed
// from the pools' shared base in list order, as after k_c_round_commit's
// pool reset — so the same state gives the same bytes.
namespace {
struct SnapLive {
  std::vector<uint32_t> cnt4, inb0, inb1, arv0, arv1;
  std::vector<uint64_t> xl, yl;                        // the lists' live prefixes, run after run
  std::vector<gg_cmsg> pool0, pool1;
};
struct LiveRef { uint32_t list, idx; uint32_t* s32; uint64_t* s64; };
bool canon_pool(uint32_t base, uint32_t cap, uint32_t& npool, std::vector<gg_cmsg>& pool, std::vector<LiveRef>& refs)
{
  // every reference into the shared part, each record once: else the state is left as it is
  if (npool > cap || pool.size() != npool) return false;
  std::vector<bool> seen(npool, false);
  for (const LiveRef& r : refs) {
    if (r.idx < base || r.idx >= npool || seen[r.idx]) return false;
    seen[r.idx] = true;
  }
  if ((uint64_t)base + refs.size() > cap) return false;
  std::vector<gg_cmsg> out(pool.begin(), pool.begin() + std::min<size_t>(base, pool.size()));
  out.resize(base);                                    // (npool below the base: nothing was allocated yet)
  for (size_t a = 0; a < refs.size();) {
    size_t b = a;
    while (b < refs.size() && refs[b].list == refs[a].list) ++b;
    std::vector<gg_cmsg> recs;
    for (size_t i = a; i < b; ++i) recs.push_back(pool[refs[i].idx]);
    std::sort(recs.begin(), recs.end(), [](const gg_cmsg& x, const gg_cmsg& y) { return std::memcmp(&x, &y, sizeof(gg_cmsg)) < 0; });
    for (size_t i = a; i < b; ++i) {
      const uint32_t ni = (uint32_t)out.size();
      const gg_cmsg& m = recs[i - a];
      if (refs[i].s32) *refs[i].s32 = ni; else *refs[i].s64 = (uint64_t)ni | ((uint64_t)m.dst << 32);
      out.push_back(m);
    }
    a = b;
  }
  pool.swap(out);
  npool = (uint32_t)pool.size();
  return true;
}
}  // namespace

static gg_status snap_live(gg_coh_state* C, SnapCounts& n, SnapLive& v)
{
  const CP& P = C->P; const CS& S = C->S;
  const bool hbh = P.net == GG_NET_EMESH_HOP_BY_HOP;
  v.cnt4.resize((size_t)P.L * 4); v.inb0.resize((size_t)P.L * P.IC); v.arv1.resize(hbh ? (size_t)P.L * P.IC : 1);
  GG_HIP(hipMemcpy(v.cnt4.data(), S.cnt4, 4 * v.cnt4.size(), hipMemcpyDeviceToHost));
  GG_HIP(hipMemcpy(v.inb0.data(), S.inb0, 4 * v.inb0.size(), hipMemcpyDeviceToHost));
  GG_HIP(hipMemcpy(v.arv1.data(), S.arv1, 4 * v.arv1.size(), hipMemcpyDeviceToHost));
  v.inb1.resize(v.inb0.size()); v.arv0.resize(v.arv1.size());
  GG_HIP(hipMemcpy(v.inb1.data(), S.inb1, 4 * v.inb1.size(), hipMemcpyDeviceToHost));
  GG_HIP(hipMemcpy(v.arv0.data(), S.arv0, 4 * v.arv0.size(), hipMemcpyDeviceToHost));
  // entries past a list's count are leftovers of earlier steps (slots handed
  // out by atomics): dead, and zero in a snapshot
  for (uint32_t lt = 0; lt < P.L; ++lt) {
    const uint32_t* c = &v.cnt4[(size_t)lt * 4];
    std::vector<uint32_t>* ls[4] = {&v.inb0, &v.inb1, &v.arv0, &v.arv1};
    for (int k = 0; k < 4; ++k) {
      if (k >= 2 && !hbh) continue;
      for (uint32_t j = std::min(c[k], P.IC); j < P.IC; ++j) (*ls[k])[(size_t)lt * P.IC + j] = 0;
    }
  }
  v.pool0.resize(std::min(n.npool[0], P.msg_cap)); v.pool1.resize(std::min(n.npool[1], P.msg_cap));
  if (!v.pool0.empty()) GG_HIP(hipMemcpy(v.pool0.data(), S.pool0, sizeof(gg_cmsg) * v.pool0.size(), hipMemcpyDeviceToHost));
  if (!v.pool1.empty()) GG_HIP(hipMemcpy(v.pool1.data(), S.pool1, sizeof(gg_cmsg) * v.pool1.size(), hipMemcpyDeviceToHost));
  for (int k = 0; k < 2; ++k) {
    const std::vector<uint32_t>& cnt = k ? n.nyl : n.nxl;
    std::vector<uint64_t>& o = k ? v.yl : v.xl;
    o.resize(list_words(cnt, P.seg_cap));
    size_t at = 0;
    for (size_t g = 0; g < cnt.size(); ++g) {
      const uint32_t c = std::min(cnt[g], P.seg_cap);
      if (c) GG_HIP(hipMemcpy(o.data() + at, (k ? S.yl : S.xl) + g * (size_t)P.seg_cap, 8ull * c, hipMemcpyDeviceToHost));
      at += c;
    }
  }
  // the references: inbox lists of the next quantum's step 0 into pool 1; its
  // SELF arrivals and run lists into pool 0 (import_one).  Lists of the other
  // parity hold nothing at a boundary; if they do, the state stays as it is.
  std::vector<LiveRef> r0, r1;
  uint32_t lid = 0;
  bool plain = true;
  for (uint32_t lt = 0; lt < P.L; ++lt, ++lid) {
    const uint32_t* c = &v.cnt4[(size_t)lt * 4];
    if (c[1] || c[2] || c[0] > P.IC || c[3] > P.IC || (!hbh && c[3])) { plain = false; break; }
    for (uint32_t j = 0; j < c[0]; ++j) { uint32_t* sl = &v.inb0[(size_t)lt * P.IC + j]; r1.push_back(LiveRef{lid, *sl, sl, nullptr}); }
  }
  for (uint32_t lt = 0; plain && hbh && lt < P.L; ++lt, ++lid)
    for (uint32_t j = 0; j < v.cnt4[(size_t)lt * 4 + 3]; ++j) { uint32_t* sl = &v.arv1[(size_t)lt * P.IC + j]; r0.push_back(LiveRef{lid, *sl, sl, nullptr}); }
  for (int k = 0; plain && k < 2; ++k) {
    const std::vector<uint32_t>& cnt = k ? n.nyl : n.nxl;
    std::vector<uint64_t>& o = k ? v.yl : v.xl;
    size_t at = 0;
    for (size_t g = 0; g < cnt.size(); ++g, ++lid)
      for (uint32_t j = 0; j < std::min(cnt[g], P.seg_cap); ++j, ++at) r0.push_back(LiveRef{lid, (uint32_t)o[at], nullptr, &o[at]});
  }
  if (!plain) return GG_OK;
  // (both pools or neither: copies, committed together)
  SnapLive w = v;
  auto rebase = [&](std::vector<LiveRef>& rs) {
    for (LiveRef& r : rs) {
      if (r.s32) r.s32 = (r.s32 >= v.inb0.data() && r.s32 < v.inb0.data() + v.inb0.size()) ? w.inb0.data() + (r.s32 - v.inb0.data())
                                                                                          : w.arv1.data() + (r.s32 - v.arv1.data());
      else r.s64 = (r.s64 >= v.xl.data() && r.s64 < v.xl.data() + v.xl.size()) ? w.xl.data() + (r.s64 - v.xl.data())
                                                                               : w.yl.data() + (r.s64 - v.yl.data());
    }
  };
  rebase(r0); rebase(r1);
  uint32_t np0 = (uint32_t)w.pool0.size(), np1 = (uint32_t)w.pool1.size();
  const uint32_t base = P.L * kChunk;
  if (np0 != n.npool[0] || np1 != n.npool[1]) return GG_OK;
  if (!canon_pool(base, P.msg_cap, np0, w.pool0, r0) || !canon_pool(base, P.msg_cap, np1, w.pool1, r1)) return GG_OK;
  v = std::move(w);
  n.npool[0] = np0; n.npool[1] = np1;
  return GG_OK;
}

// host_buf == nullptr: the size only
static gg_status coh_snapshot(gg_ctx* ctx, uint8_t* host_buf, uint64_t cap, uint64_t* bytes)
{
  gg_coh_state* C = ctx->coh;
  const CP& P = C->P; const CS& S = C->S;
  hipSetDevice(ctx->device);
  hipStream_t s = ctx->last_stream;
  GG_HIP(hipStreamSynchronize(s));
  if (gg_status e = coh_check(ctx)) return e;
  SnapCounts n;
  n.nxl.resize(std::max(P.nsx, 1u)); n.nyl.resize(std::max(P.nsy, 1u));
  GG_HIP(hipMemcpy(n.npool, S.npool, sizeof(n.npool), hipMemcpyDeviceToHost));
  GG_HIP(hipMemcpy(&n.bnd, S.bnd_cnt, sizeof(uint32_t), hipMemcpyDeviceToHost));
  GG_HIP(hipMemcpy(n.nxl.data(), S.nxl, sizeof(uint32_t) * n.nxl.size(), hipMemcpyDeviceToHost));
  GG_HIP(hipMemcpy(n.nyl.data(), S.nyl, sizeof(uint32_t) * n.nyl.size(), hipMemcpyDeviceToHost));
  SnapLive live;
  if (gg_status e = snap_live(C, n, live)) return e;
  std::vector<uint64_t> stw;
  if (gg_status e = gg_stats_snapshot(ctx, stw)) return e;
  std::vector<SnapPacked> pk = snap_packed(C);
  std::vector<std::vector<uint64_t>> base(pk.size(), std::vector<uint64_t>((size_t)P.L + 1));
  for (size_t i = 0; i < pk.size(); ++i) {
    GG_HIP(snap_count(pk[i].src, C->pk_counts, C->pk_base, s));
    GG_HIP(hipMemcpyAsync(base[i].data(), C->pk_base, sizeof(uint64_t) * (P.L + 1), hipMemcpyDeviceToHost, s));
    GG_HIP(hipStreamSynchronize(s));
  }
  const SnapLaunch sl = snap_launch(C);
  const uint64_t nqueues = (uint64_t)P.T * 6 + 1;
  ggsnap::Layout lay;
  lay.add("cfg", ggsnap::SK_DENSE, 0, sizeof(gg_config), 0);
  lay.add("launch", ggsnap::SK_DENSE, 0, sizeof(SnapLaunch), 0);
  lay.add("offsets", ggsnap::SK_DENSE, 0, sizeof(uint64_t) * C->offs_host.size(), 0);
  lay.add("stats", ggsnap::SK_DENSE, 0, sizeof(uint64_t) * stw.size(), 0);
  lay.add("err", ggsnap::SK_DENSE, 0, 2 * sizeof(uint32_t), 0);
  lay.add("noc_ctr", ggsnap::SK_DENSE, 0, sizeof(uint64_t) * P.T * GG_NUM_NET_COUNTERS, 0);
  lay.add("noc_q", ggsnap::SK_DENSE, 0, sizeof(HQueue) * nqueues, 0);
  lay.add("noc_nd", ggsnap::SK_DENSE, 0, sizeof(HNode) * nqueues * P.np.max_size, 0);
  const size_t first_arr = lay.sec.size();
  for (const gg_coh_state::Arr& a : C->arrs) {
    const int pol = snap_policy(a.name);
    if (pol == SN_DENSE) lay.add(a.name, ggsnap::SK_DENSE, 0, a.bytes, 0);
    else if (pol == SN_PREFIX) {
      uint64_t b = 0;
      if (!std::strcmp(a.name, "pool0")) b = sizeof(gg_cmsg) * std::min(n.npool[0], P.msg_cap);
      else if (!std::strcmp(a.name, "pool1")) b = sizeof(gg_cmsg) * std::min(n.npool[1], P.msg_cap);
      else if (!std::strcmp(a.name, "bnd")) b = sizeof(gg_cmsg) * std::min(n.bnd, P.msg_cap);
      else if (!std::strcmp(a.name, "xl")) b = 8 * list_words(n.nxl, P.seg_cap);
      else b = 8 * list_words(n.nyl, P.seg_cap);
      lay.add(a.name, ggsnap::SK_DENSE, 0, b, 0);
    }
  }
  const size_t first_pk = lay.sec.size();
  for (size_t i = 0; i < pk.size(); ++i)
    lay.add(pk[i].name, ggsnap::SK_PACKED, pk[i].src.rw * 8, base[i][P.L] * pk[i].src.rw * 8, base[i][P.L]);
  const uint64_t total = lay.finish();
  *bytes = total;
  if (!host_buf) return GG_OK;
  if (cap < total) return gg_fail(GG_ERR_RANGE, "snapshot needs %llu bytes, the buffer holds %llu",
                                  (unsigned long long)total, (unsigned long long)cap);
  // (the padding between sections is part of the checksummed payload: zero)
  for (size_t i = 0; i < lay.sec.size(); ++i) {
    const uint64_t e = lay.sec[i].off + lay.sec[i].bytes, nx = i + 1 < lay.sec.size() ? lay.sec[i + 1].off : total;
    if (nx > e) std::memset(host_buf + e, 0, nx - e);
  }
  auto at = [&](size_t i) { return host_buf + lay.sec[i].off; };
  std::memcpy(at(0), &ctx->cfg, sizeof(gg_config));
  std::memcpy(at(1), &sl, sizeof(sl));
  std::memcpy(at(2), C->offs_host.data(), lay.sec[2].bytes);
  std::memcpy(at(3), stw.data(), lay.sec[3].bytes);
  GG_HIP(hipMemcpy(at(4), ctx->err_dev, lay.sec[4].bytes, hipMemcpyDeviceToHost));
  GG_HIP(hipMemcpy(at(5), S.ctr, lay.sec[5].bytes, hipMemcpyDeviceToHost));
  GG_HIP(hipMemcpy(at(6), S.nq, lay.sec[6].bytes, hipMemcpyDeviceToHost));
  GG_HIP(hipMemcpy(at(7), S.nnd, lay.sec[7].bytes, hipMemcpyDeviceToHost));
  size_t si = first_arr;
  for (const gg_coh_state::Arr& a : C->arrs) {
    const int pol = snap_policy(a.name);
    if (pol != SN_DENSE && pol != SN_PREFIX) continue;
    const ggsnap::Section& sec = lay.sec[si];
    // the live records and their lists come from the host copies (snap_live)
    const void* host = nullptr;
    uint64_t hb = 0;
    auto from = [&](const char* nm, const void* p, uint64_t b) { if (!std::strcmp(a.name, nm)) { host = p; hb = b; } };
    from("npool", n.npool, sizeof(n.npool));
    from("inb0", live.inb0.data(), 4 * live.inb0.size()); from("arv1", live.arv1.data(), 4 * live.arv1.size());
    from("inb1", live.inb1.data(), 4 * live.inb1.size()); from("arv0", live.arv0.data(), 4 * live.arv0.size());
    from("xl", live.xl.data(), 8 * live.xl.size()); from("yl", live.yl.data(), 8 * live.yl.size());
    from("pool0", live.pool0.data(), sizeof(gg_cmsg) * live.pool0.size());
    from("pool1", live.pool1.data(), sizeof(gg_cmsg) * live.pool1.size());
    if (host) {
      if (hb != sec.bytes) return gg_fail(GG_ERR_STATE, "snapshot: section %s changed size while it was taken", a.name);
      if (hb) std::memcpy(at(si), host, hb);
    }
    else if (sec.bytes) GG_HIP(hipMemcpy(at(si), a.p, sec.bytes, hipMemcpyDeviceToHost));
    // the launch index is not state: a resume restarts it at 0 (QS_START = 0,
    // S.live[] zeroed), and the launch forms count differently — the ensemble
    // ends a quantum in a step launch, the single hop-by-hop run in a walker
    // launch.  Both words leave as a resume sets them, so the same state gives
    // the same bytes whoever drove the run.
    if (!std::strcmp(a.name, "qs")) std::memset(at(si) + sizeof(uint64_t) * QS_START, 0, sizeof(uint64_t));
    if (!std::strcmp(a.name, "ring")) std::memset(at(si) + sizeof(uint32_t) * 7, 0, sizeof(uint32_t) * 4);
    ++si;
  }
  for (size_t i = 0; i < pk.size(); ++i) {
    const ggsnap::Section& sec = lay.sec[first_pk + i];
    if (!sec.bytes) continue;
    if (gg_status e = C->pk_stage.reserve(sec.bytes)) return e;
    GG_HIP(hipMemcpyAsync(C->pk_base, base[i].data(), sizeof(uint64_t) * (P.L + 1), hipMemcpyHostToDevice, s));
    GG_HIP(snap_pack(pk[i].src, C->pk_base, sec.records, reinterpret_cast<uint64_t*>(C->pk_stage.get()), s));
    GG_HIP(hipMemcpyAsync(at(first_pk + i), C->pk_stage, sec.bytes, hipMemcpyDeviceToHost, s));
    GG_HIP(hipStreamSynchronize(s));
  }
  lay.write(host_buf, total);
  return GG_OK;
}

gg_status gg_coherent_snapshot_size(gg_ctx* ctx, uint64_t* bytes)
{
  if (!ctx || !bytes) return gg_fail(GG_ERR_INVALID, "NULL argument");
  if (gg_status st = snap_valid(ctx, "gg_coherent_snapshot_size")) return st;
  return coh_snapshot(ctx, nullptr, 0, bytes);
}

gg_status gg_coherent_snapshot(gg_ctx* ctx, void* host_buf, uint64_t cap, uint64_t* bytes)
{
  if (!ctx || !bytes || !host_buf) return gg_fail(GG_ERR_INVALID, "NULL argument");
  if (gg_status st = snap_valid(ctx, "gg_coherent_snapshot")) return st;
  return coh_snapshot(ctx, (uint8_t*)host_buf, cap, bytes);
}

gg_status gg_coherent_restore(gg_ctx* ctx, const gg_trace* tr, uint64_t* access_out_dev, const void* host_buf,
                              uint64_t bytes, void* stream)
{
  GG_NOT_ATAC(ctx, "gg_coherent_restore");
  if (!ctx || !tr || !tr->tile_offsets || !host_buf) return gg_fail(GG_ERR_INVALID, "NULL argument");
  if (gg_status st = coh_owns_all(ctx, GG_ERR_UNSUPPORTED, "gg_coherent_restore")) return st;
  hipSetDevice(ctx->device);
  if (gg_status st = coh_alloc(ctx)) return st;
  gg_coh_state* C = ctx->coh;
  const CP& P = C->P;
  // ---- everything is checked before anything is changed ----
  ggsnap::View v;
  if (const char* why = ggsnap::parse(host_buf, bytes, &v)) return gg_fail(GG_ERR_INVALID, "gg_coherent_restore: %s", why);
  auto bad = [](const char* what) { return gg_fail(GG_ERR_INVALID, "gg_coherent_restore: %s", what); };
  auto dense = [&](const char* name, uint64_t want) -> const ggsnap::Section* {
    const ggsnap::Section* x = v.find(name);
    return x && x->kind == ggsnap::SK_DENSE && x->bytes == want ? x : nullptr;
  };
  const ggsnap::Section* x;
  if (!(x = dense("cfg", sizeof(gg_config))) || std::memcmp(v.data(*x), &ctx->cfg, sizeof(gg_config)))
    return bad("the snapshot was taken under a different gg_config");
  const SnapLaunch sl = snap_launch(C);
  if (!(x = dense("launch", sizeof(SnapLaunch))) || std::memcmp(v.data(*x), &sl, sizeof(sl)))
    return bad("the snapshot was taken under a different derived launch state (environment knobs, build)");
  if (!(x = dense("offsets", sizeof(uint64_t) * (P.T + 1))) || std::memcmp(v.data(*x), tr->tile_offsets, x->bytes))
    return bad("the trace's tile_offsets are not the snapshot's");
  const ggsnap::Section* xst = v.find("stats");
  if (!xst || xst->kind != ggsnap::SK_DENSE || (xst->bytes & 7)) return bad("statistics-trace section");
  std::vector<uint64_t> stw(xst->bytes / 8);
  std::memcpy(stw.data(), v.data(*xst), xst->bytes);
  if (!gg_stats_snapshot_ok(ctx, stw.data(), stw.size())) return bad("statistics-trace section does not fit the context");
  const uint64_t nqueues = (uint64_t)P.T * 6 + 1;
  const ggsnap::Section* xerr = dense("err", 2 * sizeof(uint32_t));
  const ggsnap::Section* xctr = dense("noc_ctr", sizeof(uint64_t) * P.T * GG_NUM_NET_COUNTERS);
  const ggsnap::Section* xq = dense("noc_q", sizeof(HQueue) * nqueues);
  const ggsnap::Section* xnd = dense("noc_nd", sizeof(HNode) * nqueues * P.np.max_size);
  if (!xerr || !xctr || !xq || !xnd) return bad("a NoC or error-word section is missing or its size disagrees with the context");
  for (const gg_coh_state::Arr& a : C->arrs)
    if (snap_policy(a.name) == SN_DENSE && !dense(a.name, a.bytes))
      return gg_fail(GG_ERR_INVALID, "gg_coherent_restore: section %s is missing or its size disagrees with the context", a.name);
  // the prefix sections against the counts the snapshot itself carries
  SnapCounts n;
  n.nxl.resize(std::max(P.nsx, 1u)); n.nyl.resize(std::max(P.nsy, 1u));
  std::memcpy(n.npool, v.data(*v.find("npool")), sizeof(n.npool));
  std::memcpy(&n.bnd, v.data(*v.find("bnd_cnt")), sizeof(uint32_t));
  std::memcpy(n.nxl.data(), v.data(*v.find("nxl")), sizeof(uint32_t) * n.nxl.size());
  std::memcpy(n.nyl.data(), v.data(*v.find("nyl")), sizeof(uint32_t) * n.nyl.size());
  if (!dense("pool0", sizeof(gg_cmsg) * std::min(n.npool[0], P.msg_cap)) ||
      !dense("pool1", sizeof(gg_cmsg) * std::min(n.npool[1], P.msg_cap)) ||
      !dense("bnd", sizeof(gg_cmsg) * std::min(n.bnd, P.msg_cap)) ||
      !dense("xl", 8 * list_words(n.nxl, P.seg_cap)) || !dense("yl", 8 * list_words(n.nyl, P.seg_cap)))
    return bad("a record pool or list section disagrees with its count");
  std::vector<SnapPacked> pk = snap_packed(C);
  for (const SnapPacked& p : pk) {
    x = v.find(p.name);
    const uint64_t slots = (uint64_t)p.src.L * p.src.n;
    if (!x || x->kind != ggsnap::SK_PACKED || x->rec_bytes != p.src.rw * 8 || x->records > slots)
      return gg_fail(GG_ERR_INVALID, "gg_coherent_restore: packed section %s is missing or does not fit the context", p.name);
    const uint8_t* r = v.data(*x);
    uint64_t prev = 0;
    for (uint64_t i = 0; i < x->records; ++i, r += x->rec_bytes) {   // slot indices: inside the arrays, ascending
      uint64_t g;
      std::memcpy(&g, r, 8);
      if (g >= slots || (i && g <= prev))
        return gg_fail(GG_ERR_INVALID, "gg_coherent_restore: packed section %s, record %llu: slot index", p.name, (unsigned long long)i);
      prev = g;
    }
  }
  // ---- the usual reset, then the state ----
  if (gg_status st = gg_stats_restore_configure(ctx, stw.data())) return st;
  if (gg_status st = gg_coherent_begin(ctx, tr, access_out_dev, stream)) return st;
  hipStream_t s = ctx->last_stream;
  const CS& S = C->S;
  if (gg_status st = gg_stats_restore_upload(ctx, stw.data(), stw.size(), s)) return st;
  GG_HIP(hipMemcpy(ctx->err_dev, v.data(*xerr), xerr->bytes, hipMemcpyHostToDevice));
  GG_HIP(hipMemcpy(S.ctr, v.data(*xctr), xctr->bytes, hipMemcpyHostToDevice));
  GG_HIP(hipMemcpy(S.nq, v.data(*xq), xq->bytes, hipMemcpyHostToDevice));
  GG_HIP(hipMemcpy(S.nnd, v.data(*xnd), xnd->bytes, hipMemcpyHostToDevice));
  for (const gg_coh_state::Arr& a : C->arrs) {
    const int pol = snap_policy(a.name);
    if (pol != SN_DENSE && pol != SN_PREFIX) continue;
    x = v.find(a.name);
    const bool lists = !std::strcmp(a.name, "xl") || !std::strcmp(a.name, "yl");
    if (!lists) { if (x->bytes) GG_HIP(hipMemcpy(a.p, v.data(*x), x->bytes, hipMemcpyHostToDevice)); }
    else {
      const std::vector<uint32_t>& cnt = a.name[0] == 'x' ? n.nxl : n.nyl;
      const uint8_t* o = v.data(*x);
      for (size_t g = 0; g < cnt.size(); ++g) {
        const uint64_t b = 8ull * std::min(cnt[g], P.seg_cap);
        if (b) GG_HIP(hipMemcpy((uint8_t*)a.p + g * 8ull * P.seg_cap, o, b, hipMemcpyHostToDevice));
        o += b;
      }
    }
  }
  for (const SnapPacked& p : pk) {
    x = v.find(p.name);
    if (!x->bytes) continue;
    if (gg_status st = C->pk_stage.reserve(x->bytes)) return st;
    GG_HIP(hipMemcpyAsync(C->pk_stage, v.data(*x), x->bytes, hipMemcpyHostToDevice, s));
    GG_HIP(snap_unpack(p.src, reinterpret_cast<const uint64_t*>(C->pk_stage.get()), x->records, s));
    GG_HIP(hipStreamSynchronize(s));
  }
  GG_HIP(hipStreamSynchronize(s));
  C->drv = gg_coh_state::DRV_DEVICE;                  // a snapshot is of the device loop's state
  return GG_OK;
}
