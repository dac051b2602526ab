// gg_coh_window.hip — a coherent run fed its trace in windows.
// The hand-over kernel: a thread per owned tile rebases its trace position,
// checks that the window continues where the tile stands, and works out the
// guard and horizon of qend_window (gg_coh_dev.h).  Then the host entries.
#include "gg_coh_host.h"
#include "gg_coh_window.h"

namespace ggc {

// the window's last record that is neither a GG_META_CONT line nor a BARRIER
// record; lo when there is none above lo (the horizon is then 0: no quantum is safe)
__device__ __forceinline__ uint64_t win_guard(const uint32_t* meta, uint64_t lo, uint64_t hi)
{
  uint64_t g = hi;
  while (g > lo) {
    const uint32_t m = meta[--g];
    if (m != GG_META_BARRIER && !(m & GG_META_CONT)) return g;
  }
  return lo;
}

__global__ void __launch_bounds__(256) k_c_window_install(CP P, CS S, const uint64_t* addr, const uint32_t* meta,
                                                          const uint64_t* offs, const uint8_t* fin, int mode, uint32_t* bad)
{
  const uint32_t lt = blockIdx.x * blockDim.x + threadIdx.x;
  if (lt >= P.L) return;
  const uint32_t tile = S.gtile[lt];
  const uint64_t ns = offs[tile], ne = offs[tile + 1];
  const uint64_t nf = fin && fin[tile] ? 1ull : 0ull;
  uint64_t* w = (uint64_t*)S.win + WN_HDR + (size_t)lt * WN_TILE;
  TileSt* ts = (TileSt*)S.ts + lt;
  const uint64_t r = ts->rec, e = ts->rec_end;
  if (mode == 1) {
    const bool was = w[WN_FINAL] != 0;
    uint32_t b = 0;
    if (r >= e) b = !was ? WB_STATE : !nf ? WB_FINAL : ne != ns ? WB_FINISHED : 0u;
    else if (ne == ns) b = WB_EMPTY;
    else if (addr[ns] != S.addr[r] || meta[ns] != S.meta[r]) b = WB_RECORD;
    else if (was && (!nf || ne - ns != e - r)) b = WB_FINAL;
    if (b) { atomicOr(&bad[0], b); atomicMin(&bad[1], tile + 1); }
    return;
  }
  if (mode == 0) {
    w[WN_FINAL] = nf; w[WN_CBASE] = 0; w[WN_FIRST] = ns;
  } else {                                             // (after a clean mode 1)
    w[WN_CBASE] += r - w[WN_FIRST]; w[WN_FIRST] = ns; w[WN_FINAL] = nf;
    ts->rec = ns; ts->rec_end = ne;
  }
  uint64_t g = ~0ull;
  if (!nf) {
    g = win_guard(meta, ns, ne);
    atomicMin((unsigned long long*)&S.win[WN_HOR], (unsigned long long)win_horizon(P, ns, ts->clk, g));
  }
  w[WN_GUARD] = g;
}

// consumed: the records the tile has passed since begin; min_records: what a
// non-final tile's next window must hold, up to its guard, for the quantum
// picked to run next: its barrier B, the records the tile could start before
// B at the L1-D hit path from its own clock, one BARRIER record, the guard
__global__ void __launch_bounds__(256) k_c_window_state(CP P, CS S, uint64_t* consumed, uint64_t* min_records)
{
  const uint32_t lt = blockIdx.x * blockDim.x + threadIdx.x;
  if (lt >= P.L) return;
  const uint32_t tile = S.gtile[lt];
  const uint64_t* w = (const uint64_t*)S.win + WN_HDR + (size_t)lt * WN_TILE;
  const uint64_t r = S.ts[lt].rec, clk = S.ts[lt].clk;
  consumed[tile] = w[WN_CBASE] + (r - w[WN_FIRST]);
  uint64_t need = 0;
  if (!w[WN_FINAL]) {
    const uint64_t B = (S.qs[QS_Q] + 1) * S.qs[QS_QPS];
    need = 2 + (B > clk ? (B - clk + P.lat_l1d - 1) / P.lat_l1d : 0ull);
  }
  min_records[tile] = need;
}

// A windowed run's snapshot: what of a tile's state is relative to the bound
// window leaves in a form that is not — the position as the count of consumed
// records, the record the tile stands on by value.  Into staging only.
__global__ void __launch_bounds__(256) k_c_window_gather(CP P, CS S, TileSt* ts_out, uint64_t* recs)
{
  const uint32_t lt = blockIdx.x * blockDim.x + threadIdx.x;
  if (lt >= P.L) return;
  const uint32_t tile = S.gtile[lt];
  const uint64_t* w = (const uint64_t*)S.win + WN_HDR + (size_t)lt * WN_TILE;
  TileSt t = *((const TileSt*)S.ts + lt);
  const uint64_t consumed = w[WN_CBASE] + (t.rec - w[WN_FIRST]);
  const bool fin = t.rec >= t.rec_end;                 // (of a final tile: the host has refused a failed run)
  uint64_t* o = recs + (size_t)tile * 4;
  o[0] = consumed; o[1] = fin ? 1ull : 0ull;
  o[2] = fin ? 0ull : S.addr[t.rec]; o[3] = fin ? 0ull : (uint64_t)S.meta[t.rec];
  t.rec = consumed; t.rec_end = 0;
  ts_out[lt] = t;
}

// Its restore.  Phase 0 reads the new windows and the snapshot's records
// alone; phase 1 is mode 2 of the hand-over with the consumed count from the
// snapshot (S.ts[lt].rec holds the same count, clk the tile's clock).
__global__ void __launch_bounds__(256) k_c_window_restore(CP P, CS S, const uint64_t* addr, const uint32_t* meta,
                                                          const uint64_t* offs, const uint8_t* fin, const uint64_t* recs,
                                                          int phase, uint32_t* bad)
{
  const uint32_t lt = blockIdx.x * blockDim.x + threadIdx.x;
  if (lt >= P.L) return;
  const uint32_t tile = S.gtile[lt];
  const uint64_t ns = offs[tile], ne = offs[tile + 1];
  const uint64_t nf = fin && fin[tile] ? 1ull : 0ull;
  const uint64_t* r = recs + (size_t)tile * 4;
  if (phase == 0) {
    uint32_t b = 0;
    if (r[1]) b = ne != ns ? WB_FINISHED : !nf ? WB_FINAL : 0u;
    else if (ne == ns) b = WB_EMPTY;
    else if (addr[ns] != r[2] || (uint64_t)meta[ns] != r[3]) b = WB_RECORD;
    if (b) { atomicOr(&bad[0], b); atomicMin(&bad[1], tile + 1); }
    return;
  }
  uint64_t* w = (uint64_t*)S.win + WN_HDR + (size_t)lt * WN_TILE;
  TileSt* ts = (TileSt*)S.ts + lt;
  w[WN_FINAL] = nf; w[WN_CBASE] = r[0]; w[WN_FIRST] = ns;
  ts->rec = ns; ts->rec_end = ne;
  uint64_t g = ~0ull;
  if (!nf) {
    g = win_guard(meta, ns, ne);
    atomicMin((unsigned long long*)&S.win[WN_HOR], (unsigned long long)win_horizon(P, ns, ts->clk, g));
  }
  w[WN_GUARD] = g;
}

void launch_window_gather(const CP& P, const CS& S, TileSt* ts_out, uint64_t* recs, hipStream_t s)
{
  hipLaunchKernelGGL(k_c_window_gather, dim3((P.L + 255) / 256), dim3(256), 0, s, P, S, ts_out, recs);
}
void launch_window_restore(const CP& P, const CS& S, const uint64_t* addr, const uint32_t* meta, const uint64_t* offs,
                           const uint8_t* fin, const uint64_t* recs, int phase, uint32_t* bad, hipStream_t s)
{
  hipLaunchKernelGGL(k_c_window_restore, dim3((P.L + 255) / 256), dim3(256), 0, s, P, S, addr, meta, offs, fin, recs, phase, bad);
}
void launch_window_install(const CP& P, const CS& S, const uint64_t* addr, const uint32_t* meta, const uint64_t* offs,
                           const uint8_t* fin, int mode, uint32_t* bad, hipStream_t s)
{
  hipLaunchKernelGGL(k_c_window_install, dim3((P.L + 255) / 256), dim3(256), 0, s, P, S, addr, meta, offs, fin, mode, bad);
}
void launch_window_state(const CP& P, const CS& S, uint64_t* consumed, uint64_t* min_records, hipStream_t s)
{
  hipLaunchKernelGGL(k_c_window_state, dim3((P.L + 255) / 256), dim3(256), 0, s, P, S, consumed, min_records);
}

}  // namespace ggc

using namespace ggc;
using namespace gg;

// ---- the host side: gg_coherent_begin_window / _next_window / _window_state ----
// the backstop of a windowed run (qend_window): the safe-quantum rule let a
// tile run off a window that is not the end of its trace
gg_status coh_window_exhausted()
{
  return gg_fail(GG_ERR_STATE, "coherent mode: window exhausted (a tile reached the end of a window that is not the "
                               "end of its trace; the run's results are void)");
}

// a window's offsets and final flags onto the device; the host-side checks
// both entries share
static gg_status win_upload(gg_ctx* ctx, const char* what, const gg_trace* win, const uint8_t* final_tiles, hipStream_t s)
{
  gg_coh_state* C = ctx->coh;
  const uint32_t T = C->P.T;
  if (gg_status st = coh_trace_check(win, T, what)) return st;
  if (!C->win_dev) {
    if (gg_status st = C->mem.alloc(&C->win_dev, (uint64_t)WN_HDR + (uint64_t)C->P.L * WN_TILE)) return st;
    if (gg_status st = C->mem.alloc(&C->win_fin_dev, (uint64_t)T)) return st;
    if (gg_status st = C->mem.alloc(&C->win_bad_dev, 2)) return st;
    if (gg_status st = C->mem.alloc(&C->win_state_dev, 2 * (uint64_t)T)) return st;
    if (gg_status st = C->mem.alloc(&C->win_rec_dev, 4 * (uint64_t)T)) return st;
    if (gg_status st = C->mem.alloc(&C->win_ts_dev, (uint64_t)C->P.L)) return st;
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

// ---- a windowed run's snapshot and restore: the device parts (host side: gg_snapshot.hip) ----
gg_status coh_window_gather(gg_ctx* ctx, std::vector<TileSt>& ts, std::vector<uint64_t>& recs)
{
  gg_coh_state* C = ctx->coh;
  hipStream_t s = ctx->last_stream;
  const uint32_t T = C->P.T, L = C->P.L;
  ts.resize(L); recs.resize((size_t)4 * T);
  launch_window_gather(C->P, C->S, C->win_ts_dev, C->win_rec_dev, s);
  GG_HIP(hipGetLastError());
  GG_HIP(hipMemcpyAsync(ts.data(), C->win_ts_dev, sizeof(TileSt) * L, hipMemcpyDeviceToHost, s));
  GG_HIP(hipMemcpyAsync(recs.data(), C->win_rec_dev, sizeof(uint64_t) * 4 * T, hipMemcpyDeviceToHost, s));
  GG_HIP(hipStreamSynchronize(s));
  return GG_OK;
}

gg_status coh_window_restore_check(gg_ctx* ctx, const char* what, const gg_trace* win, const uint8_t* final_tiles,
                                   const uint8_t* recs, hipStream_t s)
{
  gg_coh_state* C = ctx->coh;
  const uint32_t T = C->P.T;
  if (gg_status st = win_upload(ctx, what, win, final_tiles, s)) return st;
  GG_HIP(hipMemcpyAsync(C->win_rec_dev, recs, sizeof(uint64_t) * 4 * T, hipMemcpyHostToDevice, s));
  launch_window_restore(C->P, C->S, win->addr_dev, win->meta_dev, C->offs_dev, C->win_fin_dev, C->win_rec_dev, 0,
                        C->win_bad_dev, s);
  GG_HIP(hipGetLastError());
  uint32_t bad[2] = {0, 0};
  GG_HIP(hipMemcpyAsync(bad, C->win_bad_dev, sizeof(bad), hipMemcpyDeviceToHost, s));
  GG_HIP(hipStreamSynchronize(s));
  if (bad[0]) {
    const uint32_t t = bad[1] - 1;
    const char* why = (bad[0] & WB_EMPTY)    ? "an unfinished tile's range holds no record"
                    : (bad[0] & WB_RECORD)   ? "a window's first record is not the record its tile stood on (addr or meta)"
                    : (bad[0] & WB_FINISHED) ? "a finished tile's range is not empty"
                                             : "a tile that is not final has an empty window";
    return gg_fail(GG_ERR_INVALID, "%s: %s (first at tile %u); nothing changed", what, why, t);
  }
  return GG_OK;
}

gg_status coh_window_restore_install(gg_ctx* ctx, const gg_trace* win, hipStream_t s)
{
  gg_coh_state* C = ctx->coh;
  cs_set(C->S.win, C->win_dev);
  const uint64_t w0[WN_HDR] = {~0ull, ~0ull};
  GG_HIP(hipMemcpyAsync(C->win_dev, w0, sizeof(w0), hipMemcpyHostToDevice, s));
  GG_HIP(hipMemcpyAsync(C->Sd, &C->S, sizeof(CS), hipMemcpyHostToDevice, s));
  // (offs_dev holds win's offsets since the reset, win_fin_dev and win_rec_dev their values since the check)
  launch_window_restore(C->P, C->S, win->addr_dev, win->meta_dev, C->offs_dev, C->win_fin_dev, C->win_rec_dev, 1,
                        C->win_bad_dev, s);
  GG_HIP(hipGetLastError());
  GG_HIP(hipStreamSynchronize(s));
  C->windowed = true;
  C->drv = gg_coh_state::DRV_DEVICE;
  return GG_OK;
}
