// gg_internal.h — shared definitions of the MI355X backend (host + device).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string>
#include <vector>

#include "../../include/graphite_gpu.h"
#include "gg_devmem.h"

#define GG_WAVE 64
#define GG_NUM_XCD 8          // MI355X: 8 XCDs, workgroups dealt round-robin by blockIdx

// Packed meta byte of one cache line in the device-resident state:
//   bits 0-1 state (0 I, 1 S, 2 M), bit 2 cached_loc == L1-D (L2 only),
//   bits 3-7 replacement age (LRUReplacementPolicy::_lru_bits_vec entry).
#define GG_MS_I 0u
#define GG_MS_S 1u
#define GG_MS_M 2u
#define GG_M_STATE(b) ((b) & 3u)
#define GG_M_LOC(b) (((b) >> 2) & 1u)
#define GG_M_AGE(b) ((b) >> 3)
#define GG_M_MAKE(st, loc, age) ((uint32_t)(st) | ((uint32_t)(loc) << 2) | ((uint32_t)(age) << 3))

#define GG_L1_INV_TAG (~0ull)     // CacheLineInfo invalid tag (cache_line_info.h:21-22)
#define GG_L2_INV_TAG 0xFFFFFFFFu // compressed L2 tag (line >> log2(L2 sets)); 2^32-1 is out of range

// Error bits of the device-side error word (ctx->err_dev).
#define GG_DERR_RANGE 1u   // address beyond the compressed-tag range
#define GG_DERR_STATE 2u   // the reference would LOG_ASSERT_ERROR on this state
#define GG_DERR_CAP 4u     // a device-side capacity (messages, queues, inbox) was exceeded
#define GG_DERR_BARRIER 8u // a BARRIER record (GG_META_BARRIER) reached a path that has no barriers (Mode P)
#define GG_DERR_SAMPLES 16u // the statistics trace's sample buffer is full (gg_stats.hip)
#define GG_DERR_SHARERS 32u // the statistics trace's scan met a directory entry with more sharers than tiles
#define GG_DERR_MT_CAP 64u  // Mode P miss-type tracking: a (tile, L1-D set) slice of the address table is full (gg_modep_mt.h)
#define GG_DERR_WINDOW 128u // a windowed coherent run: a tile reached the end of a window that is not the end of its trace

// Geometry derived from gg_config (cache.cc:44, cache_hash_fn.h:11).
struct gg_geom {
  uint32_t tiles;
  uint32_t log_line;
  uint32_t u1;        // L1-D sets = units per tile
  uint32_t log_u1;
  uint32_t a1;        // L1-D ways
  uint32_t l2_sets;
  uint32_t log_l2;
  uint32_t s2;        // L2 sets per unit (l2_sets / u1)
  uint32_t a2;        // L2 ways
  uint32_t mw;        // u64 meta words per L2 set ((a2 + 7) / 8)
  uint32_t pol1, pol2;
  uint64_t units;     // tiles * u1
  uint64_t addr_limit;  // first byte address whose L2 tag no longer fits 32 bits
};

// Device-resident cache state, structure of arrays indexed [field][unit] so a
// wave of 64 consecutive units loads/stores it coalesced.
struct gg_cache_state {
  uint64_t* l1_tag;   // [a1][units]      line address or ~0
  uint64_t* l1_meta;  // [units]          byte w = meta of way w
  uint8_t*  l1_rr;    // [units]          RoundRobin index
  uint32_t* l2_tag;   // [s2*a2][units]   line >> log2(l2_sets) or 2^32-1
  uint64_t* l2_meta;  // [s2*mw][units]   byte (w%8) of word w/8
  uint8_t*  l2_rr;    // [s2][units]
  uint64_t* counters; // [tiles][2][GG_NUM_CACHE_COUNTERS]
};

// Mode P miss-type tracking (gg_cache_track_miss_types; the device side is
// gg_modep_mt.h): the address table [tile][tracked cache][L1-D set][slot] and
// the counts, as the kernels see them.  tab == nullptr: not opted in.
struct gg_mt_view {
  uint64_t* tab;
  unsigned long long* cnt;   // [tiles][2][GG_NUM_MISS_TYPES]
  uint32_t log_spu;          // log2(slots per (tile, cache, L1-D set))
  uint32_t on1, on2;         // L1-D / L2 tracked
};

struct gg_timer {
  std::string name;
  hipEvent_t start = nullptr, stop = nullptr;
  bool valid = false;
};

struct gg_noc_state;
struct gg_coh_state;
struct gg_stats_state;
struct gg_atac_state;
struct gg_synth_state;
struct gg_memsynth_state;

struct gg_ctx {
  gg_config cfg;
  gg_geom g;
  int device = 0;
  int num_cus = 256;
  hipStream_t last_stream = nullptr;
  gg_arena mem;                  // owns what lives as long as the context: cs, err_dev, unit_*, total_dev, tile_off_dev
                                 // (raw pointers below; gg_devmem.h)
  gg_cache_state cs{};
  uint32_t* err_dev = nullptr;
  // batch scratch (grown on demand)
  gg_dbuf<uint64_t> sh_key;      // sharded records (slot order): line address | write bit
  gg_dbuf<uint32_t> sh_res;      // replay results in slot order
  gg_dbuf<uint64_t> sh_ev;       // evicted L2 line addresses in slot order (only when requested)
  gg_dbuf<uint32_t> rec_slot;    // [records] slot of each program-order record (written by the scatter)
  gg_dbuf<uint32_t> chunk_cnt;   // [chunks][u1]
  gg_dbuf<uint32_t> chunk_tile;  // the chunk tables share one capacity (in chunks)
  gg_dbuf<uint64_t> chunk_start;
  gg_dbuf<uint32_t> chunk_len;
  uint32_t* unit_len = nullptr;  // [units]
  uint64_t* unit_base = nullptr; // [units] slot of the unit's record 0 (records contiguous, padded to 8)
  uint64_t* total_dev = nullptr; // slots of the sharded layout
  uint64_t* tile_off_dev = nullptr; // [tiles+1]
  std::vector<uint32_t> h_chunk_tile, h_chunk_len;
  std::vector<uint64_t> h_chunk_start;
  // NoC
  gg_noc_state* noc = nullptr;
  gg_atac_state* atac = nullptr;  // net_model GG_NET_ATAC (gg_noc_atac.hip)
  // coherent mode (gg_coherent.hip), allocated on first use
  gg_coh_state* coh = nullptr;
  // replay kernel choice: 0 = lean when instantiated (default), 1 = generic
  int replay_variant = 0;
  // Mode P miss-type tracking (gg_cache_track_miss_types): the table, its
  // capacity per (tile, cache) in lines, and whether the private cache state
  // has been touched since gg_create / gg_reset (the opt-in needs it fresh)
  gg_mt_view mt{};
  gg_dbuf<uint64_t> mt_tab;                // mt.tab / mt.cnt
  gg_dbuf<unsigned long long> mt_cnt;
  uint64_t mt_lines = 0;
  bool cache_dirty = false;
  // timing
  int timing = 0;                // gg_set_timing: 0 off, 1 sampled coherent launches, 2 every launch
  std::vector<gg_timer> timers;
  // core timing (gg_core.hip): [tiles][GG_NUM_CORE_STATS] and its task list
  gg_dbuf<uint64_t> core_dev;
  gg_dbuf<uint8_t> core_tasks;   // CoreTask records
  bool core_valid = false;
  // the iocoom core model (gg_core.hip): [tiles][GG_NUM_IOCOOM_STATS], the
  // two offset lists [2][tiles + 1] and the stream-check word
  gg_dbuf<uint64_t> io_stats;
  gg_dbuf<uint64_t> io_offs;
  gg_dbuf<uint32_t> io_err;
  bool io_valid = false;
  // multi-rank round buffers (gg_round.hip), deleted by gg_destroy through round_free
  void* round = nullptr;
  void (*round_free)(void*) = nullptr;
  // statistics trace (gg_stats.hip), allocated by gg_stats_trace_configure
  gg_stats_state* stats = nullptr;
  // packet arrays of gg_noc_synthetic_run (gg_noc_synth.hip), allocated on first use
  gg_synth_state* synth = nullptr;
  // trace and results of gg_mem_synthetic_run (gg_mem_synth.hip), allocated on first use
  gg_memsynth_state* memsynth = nullptr;
};
inline void* gg_round_state(gg_ctx* ctx) { return ctx->round; }
inline void gg_round_state_set(gg_ctx* ctx, void* p, void (*f)(void*)) { ctx->round = p; ctx->round_free = f; }

// error reporting (gg_capi.hip)
gg_status gg_fail(gg_status code, const char* fmt, ...);
gg_status gg_hip_check(hipError_t e, const char* what);
#define GG_HIP(x) do { hipError_t _e = (x); if (_e != hipSuccess) return gg_hip_check(_e, #x); } while (0)

// ATAC (GG_NET_ATAC) is built for the NoC batch API only: the coherent entry points refuse such a context
#define GG_NOT_ATAC(ctx, what) \
  do { if ((ctx) && (ctx)->cfg.net_model == GG_NET_ATAC) \
         return gg_fail(GG_ERR_UNSUPPORTED, "%s: the ATAC network model is built for the NoC batch API only " \
                        "(gg_noc_route_batch / gg_noc_route_tree)", what); } while (0)

// timing helpers (gg_capi.hip)
void gg_timer_begin(gg_ctx* ctx, const char* name, hipStream_t s);
void gg_timer_end(gg_ctx* ctx, const char* name, hipStream_t s);

// cache path (gg_cache.hip)
gg_status gg_cache_state_alloc(gg_ctx* ctx);
gg_status gg_cache_state_reset(gg_ctx* ctx, hipStream_t s);
gg_status gg_cache_run_batch(gg_ctx* ctx, const gg_trace* tr, uint32_t* result, uint64_t* evicted, hipStream_t s);
gg_status gg_cache_quartet(gg_ctx* ctx, int op, uint32_t tile, int level, uint64_t addr,
                           const gg_line_info* in, gg_line_info* out, int* eviction, uint64_t* ev_addr);
gg_status gg_cache_mt_alloc(gg_ctx* ctx, uint64_t lines);      // gg_cache_track_miss_types, after its checks
gg_status gg_cache_mt_counts(gg_ctx* ctx, uint64_t* out);      // [tiles][2][GG_NUM_MISS_TYPES]

// NoC path (gg_noc.hip)
gg_status gg_noc_alloc(gg_ctx* ctx);
void      gg_noc_free(gg_ctx* ctx);
gg_status gg_noc_reset(gg_ctx* ctx, hipStream_t s);
gg_status gg_noc_run(gg_ctx* ctx, const gg_packets* pk, const gg_packet_out* out, hipStream_t s);
gg_status gg_noc_tree(gg_ctx* ctx, const gg_packets* pk, const gg_packet_out* out, const gg_packet_out* bout,
                      uint64_t nb, hipStream_t s);
gg_status gg_noc_counters(gg_ctx* ctx, uint64_t* out);
// coherent path (gg_coherent.hip)
void      gg_coh_free(gg_ctx* ctx);
gg_status gg_htree_run(gg_ctx* ctx, uint64_t min_proc, const uint64_t* t, const uint64_t* p, uint64_t n, uint64_t* d);
gg_status gg_coh_kernel_stats(gg_ctx* ctx, const char* name, double* total_ms, uint64_t* launches);
uint64_t  gg_coherent_msg_cap(gg_ctx* ctx);     // records a quantum boundary can hold (after gg_coherent_begin)
// the quantum steps and the per-rank slot exchange of gg_round_exchange (gg_coherent.hip)
gg_status gg_coh_steps_async(gg_ctx* ctx, uint64_t q, uint32_t k0, uint32_t n);
gg_status gg_coh_round_tail(gg_ctx* ctx, gg_cmsg* slots, uint32_t world, uint32_t per_rank, uint64_t region,
                            uint32_t host_err, uint64_t* dv_own);
gg_status gg_coh_round_import(gg_ctx* ctx, uint64_t q, const gg_cmsg* send, const gg_cmsg* recv, uint32_t world,
                              uint32_t self, uint64_t region, uint64_t slot, const uint64_t* dv_all, uint64_t* counts);
void      gg_coh_harvest(gg_ctx* ctx);
// A rank's round status words (written by k_c_round_tail, gathered over the
// ranks, reduced by k_c_round_commit on the device and by round_decide on the
// host; internal: the transport moves them as GG_ROUND_WORDS opaque words).
//   RW_SENT     records held for other shards at the quantum's end (all slots)
//   RW_ACTIVE   owned tiles with an unfinished trace
//   RW_BLOCKED  of those, blocked on a miss (not at a BARRIER record)
//   RW_FLAGS    bits 0..31 the rank's error flags (GG_DERR_*), bit 32 not-done
//               (the step batch ended before the quantum), bits 33.. the steps
//               the quantum took
//   RW_MAXSLOT  the largest record count of one send slot
//   RW_MINNEXT  least next start (ps) of the tiles neither blocked nor waiting
//   RW_BWAIT    of the active tiles, waiting at a BARRIER record
//   RW_BMAX     their latest arrival: max clock (ps, 64 bits), 0 with no waiter
enum { RW_SENT = 0, RW_ACTIVE, RW_BLOCKED, RW_FLAGS, RW_MAXSLOT, RW_MINNEXT, RW_BWAIT, RW_BMAX, RW_N };
constexpr int kRoundWords = RW_N;
constexpr uint64_t kRwErrMask = 0xFFFFFFFFull, kRwNotDone = 1ull << 32;
constexpr int kRwStepsShift = 33;
gg_status gg_coh_import_slots(gg_ctx* ctx, const gg_cmsg* slots, uint32_t world, uint64_t region, uint64_t lo,
                              uint64_t hi, bool first, const uint64_t* skip_if_dev);
gg_status gg_coh_check(gg_ctx* ctx);
// statistics trace (gg_stats.hip; its view of the coherent state: gg_stats.h)
void      gg_stats_free(gg_ctx* ctx);
bool      gg_stats_on(const gg_ctx* ctx);                 // a trace is configured for the runs begun from now on
gg_status gg_stats_begin(gg_ctx* ctx, hipStream_t s);     // gg_coherent_begin: the configured trace, no samples
gg_status gg_stats_slot(gg_ctx* ctx, hipStream_t s, uint32_t L);   // gg_coherent_run: the scan launch of slot L
uint64_t  gg_coh_generation(gg_ctx* ctx);    // bumped by every gg_coherent_begin (0: none yet)
bool      gg_coh_windowed(const gg_ctx* ctx); // the begun run is fed its trace in windows (gg_coherent_begin_window)
// synthetic network traffic (gg_noc_synth.hip)
void      gg_synth_free(gg_ctx* ctx);
// synthetic memory traffic (gg_mem_synth.hip)
void      gg_memsynth_free(gg_ctx* ctx);
