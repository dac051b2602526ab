// gg_coh_many.hip — the host side of the ensembles on MI355X (gfx950):
// gg_coherent_run_many and gg_coherent_advance_many, their shared checks and
// their driver loop.  The launchers: gg_coh_many.h.
#include "gg_coh_host.h"
#include "gg_coh_many.h"
#include "gg_stats.h"

#include <algorithm>

namespace ggc {

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
    if (!coh_cfg_owns_all(c))
      return gg_fail(shard_code, "%s: context %u does not own every shard (shard range [%u, %u) of %u)",
                     what, i, c.shard_begin, c.shard_end, c.num_shards ? c.num_shards : 1);
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
    if (err[i]) stv[i] = gg_coh_check(ctxs[i]);
    else if (done[i] == 2) stv[i] = coh_deadlocked((int)i);
  }
}

// every instance's status out (when asked for); the call's: the first failing one
static gg_status many_fold(const std::vector<gg_status>& stv, gg_status* statuses)
{
  gg_status first = GG_OK;
  for (size_t i = 0; i < stv.size(); ++i) {
    if (statuses) statuses[i] = stv[i];
    if (first == GG_OK) first = stv[i];
  }
  return first;
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
  return many_fold(stv, statuses);
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
    if (gg_status st = coh_leg_look(ctxs[i], &qs[(size_t)i * QS_N], &next_quanta[i], &dones[i])) return st;
  }
  for (uint32_t i = 0; i < n; ++i) {
    uint64_t* q = &qs[(size_t)i * QS_N];
    const uint64_t stop = stop_quanta ? stop_quanta[i] : ~0ull;
    // over, or already there: no launch, no change, not in the live list
    if (dones[i] == 2) { stv[i] = coh_deadlocked((int)i); continue; }
    if (dones[i] || stop <= q[QS_Q]) { stv[i] = gg_coh_check(ctxs[i]); continue; }
    // the launch index restarts at 0 for all of them together (one L, §4f)
    if (gg_status st = coh_leg_resume(ctxs[i], q, stop, s)) return st;
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
  return many_fold(stv, statuses);
}
