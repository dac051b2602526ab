// gg_coh_host.h — the host side of the coherent mode, shared by its units:
// gg_coherent.hip (allocation, begin, the single-run drivers, the getters),
// gg_coh_many.hip (ensembles), gg_coh_window.hip (windows), gg_snapshot.hip
// (snapshot / restore) and gg_coh_diag.hip (the diagnostics dumps).
#pragma once
#include "gg_coh_dev.h"

#include <vector>

struct gg_coh_state {
  ggc::CP P{};
  ggc::CS S{};
  ggc::CP* Pd = nullptr;             // device copies of P / S (k_c_step reads its launch state through them)
  ggc::CS* Sd = nullptr;
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
  // a windowed run's snapshot (gg_coherent_window_snapshot / _window_restore):
  // the win records [T] on the device, the canonical copy of S.ts [L]
  uint64_t* win_rec_dev = nullptr;
  ggc::TileSt* win_ts_dev = nullptr;
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
constexpr uint32_t kPersistTiles = 64;        // owned tiles up to which gg_coherent_run uses k_c_persist
constexpr uint32_t kPersistLaunches = 16384;  // launch indices per k_c_persist launch

// What a snapshot does with an array of the list.  SN_DENSE: copied whole.
// SN_PACKED: the directory arrays, the miss-type tables and the caches' tag
// arrays (~0 = an invalid line; their meta bytes carry LRU ages and stay
// dense), as records of the slots in use.  SN_PREFIX: record pools and lists, up to their live counts.
// SN_NONE: scratch that holds nothing at a quantum boundary.
enum { SN_DENSE = 0, SN_PACKED, SN_PREFIX, SN_NONE };

inline bool coh_cfg_owns_all(const gg_config& c)      // the config owns every shard (what the device loop's entries ask)
{
  const uint32_t K = c.num_shards ? c.num_shards : 1;
  return c.shard_begin == 0 && (c.shard_end == 0 || c.shard_end == K);
}

#pragma GCC visibility push(hidden)   // (between the library's units only; gg_coh_check: gg_internal.h)
int snap_policy(const char* name);                      // gg_snapshot.hip
gg_status coh_alloc(gg_ctx* ctx);                       // the launch state, on first use
gg_status coh_owns_all(const gg_ctx* ctx, gg_status code, const char* what);
// a whole trace's or a window's offsets and pointers against T tiles; what: the messages' prefix, or null
gg_status coh_trace_check(const gg_trace* tr, uint32_t T, const char* what);
gg_status coh_window_exhausted();                       // gg_coh_window.hip
// A windowed run's snapshot and restore, the parts on the device (gg_coh_window.hip).
// gather: the tiles' win records (by tile number, ggsnap::WinRec words) and
// S.ts in canonical form (rec = consumed count, rec_end = 0) onto the host;
// the run's state is only read.  restore_check: win's ranges against the
// records of a snapshot (host, [T]), before anything is changed.
// restore_install: after the reset and the state are in place, the tiles onto
// win's arrays as gg_coherent_next_window would; the run is windowed after it.
gg_status coh_window_gather(gg_ctx* ctx, std::vector<ggc::TileSt>& ts, std::vector<uint64_t>& recs);
gg_status coh_window_restore_check(gg_ctx* ctx, const char* what, const gg_trace* win, const uint8_t* final_tiles,
                                   const uint8_t* recs, hipStream_t s);
gg_status coh_window_restore_install(gg_ctx* ctx, const gg_trace* win, hipStream_t s);
gg_status coh_deadlocked(int instance = -1);            // QS_DONE == 2 (instance: of an ensemble)
// A leg of the device loop (gg_coherent_advance, _advance_many).  look: the
// run's stream synchronised, its quantum words in qs[QS_N], *next_quantum and
// *done out of them.  resume, unless the run is over or already at stop: the
// launch index restarts at 0, so the quantum's step 0 is launch 0 (k = L -
// QS_START) and no slot of the live ring is a step; the rest, QS_REL (a barrier
// release for step 0) included, stays.  On s, which becomes the context's stream.
gg_status coh_leg_look(gg_ctx* ctx, uint64_t* qs, uint64_t* next_quantum, int* done);
gg_status coh_leg_resume(gg_ctx* ctx, uint64_t* qs, uint64_t stop_quantum, hipStream_t s);
gg_status coh_diag_dump(gg_ctx* ctx);                   // gg_coh_diag.hip: GG_COH_TRACE_OUT, GG_COH_PROFILE
#pragma GCC visibility pop
