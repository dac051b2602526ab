// gg_coh_window.hip — a coherent run fed its trace in windows (DESIGN.md
// §4j), the device side of the hand-over: one thread per owned tile rebases
// the tile's trace position to the new window's arrays, checks that the
// window continues where the tile stands, and works out the guard and the
// horizon the quantum end's safe-quantum rule reads (qend_window, gg_coh_dev.h).
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
