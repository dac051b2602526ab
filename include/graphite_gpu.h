/*
 * graphite_gpu.h — C ABI of the MI355X batch backend for Graphite's
 * memory-subsystem hot path (private L1-D/L2 cache simulation and EMesh NoC
 * packet latency).
 *
 * This is the drop-in boundary.  Every entry point below replaces one
 * in-process C++ interface of the reference simulator (paths relative to
 * nmtrmail/Graphite):
 *
 *   gg_cache_access_batch      batched Cache line access: the per-access state
 *                              machine L1CacheCntlr::processMemOpFromCore
 *                              (common/tile/memory_subsystem/
 *                              pr_l1_pr_l2_dram_directory_msi/l1_cache_cntlr.cc:89-180)
 *                              + L2CacheCntlr (l2_cache_cntlr.cc:74-527) driving
 *                              Cache::accessCacheLine / insertCacheLine /
 *                              getCacheLineInfo / setCacheLineInfo
 *                              (common/tile/memory_subsystem/cache/cache.h:87-92),
 *                              i.e. the "accessSingleLine" entry of the north star
 *                              applied to a whole trace batch.
 *   gg_cache_access_line       Cache::accessCacheLine            (cache.cc:84-112)
 *   gg_cache_insert_line       Cache::insertCacheLine            (cache.cc:114-184)
 *   gg_cache_get_line_info     Cache::getCacheLineInfo           (cache.cc:187-205)
 *   gg_cache_set_line_info     Cache::setCacheLineInfo           (cache.cc:218-241)
 *   gg_cache_get_counters      the counters printed by Cache::outputSummary
 *                              (cache.cc:419-477)
 *   gg_noc_route_batch         NetworkModel::__routePacket -> routePacket
 *                              (common/network/network_model.cc:87-116,
 *                              network_model.h:188) for every hop of each packet,
 *                              plus NetworkModel::__processReceivedPacket
 *                              (network_model.cc:118-150) at the receiver:
 *                              emesh_hop_counter (models/network_model_emesh_hop_counter.cc:143-157)
 *                              and emesh_hop_by_hop (models/network_model_emesh_hop_by_hop.cc:146-264)
 *   gg_noc_route_tree          the same with broadcast packets (receiver GG_BROADCAST):
 *                              the emesh_hop_by_hop broadcast tree
 *                              (network_model_emesh_hop_by_hop.cc:163-221,
 *                              network/emesh_hop_by_hop/broadcast_tree_enabled)
 *   gg_noc_get_counters        NetworkModel / RouterModel counters
 *                              (network_model.cc:228-316, router_model.cc:120-145)
 *   gg_queue_delay_batch       QueueModelHistoryTree::computeQueueDelay
 *                              (common/shared_models/queue_models/queue_model_history_tree.cc:44-126)
 *   gg_gen_network_traffic     the send loop and the six traffic patterns of
 *                              tests/benchmarks/synthetic_network/synthetic_network.cc:140-359
 *   gg_noc_latency_stats       its result: packets, latency and contention of a batch
 *   gg_noc_synthetic_run       the benchmark in one call on a context
 *   gg_noc_route_batch_many    many independent batches, each on its own context,
 *   gg_noc_synthetic_run_many  in one set of launches (a load-latency sweep)
 *   gg_gen_memory_traffic      the instruction stream of
 *                              tests/benchmarks/synthetic_memory/synthetic_memory.cc:135-399
 *                              as a coherent trace
 *   gg_mem_latency_stats       accesses, levels and latency of a coherent run
 *   gg_mem_synthetic_run       the benchmark in one call on a context
 *
 * Conventions: every function returns a gg_status (0 = OK, negative = error);
 * no exception crosses the ABI; pointers named *_dev are HIP device pointers,
 * all others are host pointers owned by the caller; one host thread per
 * context, one context per GPU.  The reference reports misuse with
 * LOG_ASSERT_ERROR (aborting, common/misc/log.h:112-135); this ABI returns
 * GG_ERR_* instead and records a message retrievable with gg_last_error().
 */
#ifndef GRAPHITE_GPU_H
#define GRAPHITE_GPU_H

#include <stdint.h>
#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GG_ABI_VERSION 10

typedef int gg_status;
enum {
  GG_OK = 0,
  GG_ERR_INVALID = -1,      /* bad argument / inconsistent config            */
  GG_ERR_HIP = -2,          /* HIP runtime error                             */
  GG_ERR_UNSUPPORTED = -3,  /* configuration outside what the backend builds */
  GG_ERR_RANGE = -4,        /* address / time outside the encodable range    */
  GG_ERR_STATE = -5         /* reference would LOG_ASSERT_ERROR here          */
};

/* Replacement policies: CacheReplacementPolicy::parse (cache_replacement_policy.cc:33-46) */
enum { GG_POLICY_LRU = 0, GG_POLICY_ROUND_ROBIN = 1 };

/* Network models: NetworkModel::parseNetworkType (network_model.cc:318-335) */
enum { GG_NET_MAGIC = 0, GG_NET_EMESH_HOP_COUNTER = 1, GG_NET_EMESH_HOP_BY_HOP = 2,
       GG_NET_ATAC = 3 /* batch API only: gg_noc_route_batch / gg_noc_route_tree, see gg_atac_params */ };

/* Cache levels (pr_l1_pr_l2_dram_directory_msi/cache_level.h) */
enum { GG_L1D = 0, GG_L2 = 1 };

/* Cache line states, numerically identical to CacheState::Type (cache_state.h:11-21) */
enum { GG_CSTATE_INVALID = 0, GG_CSTATE_SHARED = 1, GG_CSTATE_OWNED = 2 /* MOSI */, GG_CSTATE_EXCLUSIVE = 3 /* MESI */,
       GG_CSTATE_MODIFIED = 4 };

/* Cached-location values of a private L2 line, MemComponent::Type subset
 * (PrL2CacheLineInfo::_cached_loc, pr_l1_pr_l2_dram_directory_msi/cache_line_info.h) */
enum { GG_LOC_INVALID = 0, GG_LOC_L1I = 2, GG_LOC_L1D = 3 };

/* Access trace record metadata word (gg_trace.meta[i]):
 *   bit 0      : 1 = WRITE (Core::WRITE), 0 = READ (Core::READ)
 *   bits 1..30 : gap in core cycles before this access (coherent/timing modes;
 *                ignored by the private-cache mode)
 *   bit 31     : GG_META_CONT — a later line of a multi-line access
 *                (gg_split_accesses): coherent mode issues it at the previous
 *                record's completion and never cuts it at the lax barrier (the
 *                access is one instruction, core.cc:139-266); gap must be 0.
 *                The private-cache mode ignores it.                          */
#define GG_META_WRITE 1u
#define GG_META_CONT 0x80000000u
/* A BARRIER record (CarbonBarrierWait / SPLASH BARRIER, sync_client.cc:265-316;
 * a CONT code with a nonzero gap, which no access carries; addr ignored):
 * the tile waits until every tile with an unfinished trace waits at a
 * barrier (SimBarrier::wait, sync_server.cc:133-170 with the count = those
 * tiles), then all continue at the latest arrival time (SyncServer::
 * barrierWait replies max_time, :357-383; the MCP is a system tile, so the
 * messages cost no network time).  The release is applied at the quantum
 * boundary after the last arrival and the record's access word written as
 * (stall_ps << 2) | GG_LVL_SYNC.  Traces with barriers are taken by
 * gg_coherent_run (one context) and by the multi-rank round: gg_round_pack /
 * _unpack / _finish, gg_round_exchange, gg_coherent_run_ranks — the ranks'
 * status words carry their waiters and latest arrival, and every rank
 * releases alike, bit-identical to one context.  They are not taken by
 * gg_coherent_quantum / _export / _import (gg_coherent_quantum returns
 * GG_ERR_UNSUPPORTED: its caller picks the next quantum from a
 * gg_coherent_status that has no barrier fields) nor by the private-cache
 * batch (it flags one in the device error word, so the next
 * gg_cache_get_counters returns GG_ERR_UNSUPPORTED); gg_split_accesses
 * rejects one in its access trace: insert barriers into the line records it
 * writes.  Barriers carry no id or count: one global
 * barrier whose count is "every tile with an unfinished trace", released at
 * the quantum boundary after its last arrival.                 */
#define GG_META_BARRIER 0xFFFFFFFFu

/* Per-access result word written by gg_cache_access_batch: one flag per 4-bit
 * field, so result words of up to 15 accesses can be summed field-wise (the
 * replay kernel derives its counters that way).  Where the access was served:
 * L1-D hit = !L1_MISS; L2 hit = L1_MISS && !L2_MISS; directory = L2_MISS.   */
#define GG_RES_L1_MISS         (1u << 0)  /* not an L1-D hit (operationPermissibleinL1Cache, l1:207-243): request to the L2 */
#define GG_RES_L2_MISS         (1u << 4)  /* not an L2 hit either (l2:180-224): SH_REQ / EX_REQ to the home directory */
#define GG_RES_L1_INVAL        (1u << 8)  /* the L1-D held the line without the needed permission: invalidated first (l1:135-137) */
#define GG_RES_L1_EVICT        (1u << 12) /* the L1-D insert evicted a line (insertCacheLineInL1, l2:133-165) */
#define GG_RES_L2_EVICT        (1u << 16) /* the L2 insert evicted a line (l2:74-116) */
#define GG_RES_L2_EVICT_DIRTY  (1u << 20) /* ... in MODIFIED: FLUSH_REP + data (else INV_REP) */
#define GG_RES_L2_EVICT_INV_L1 (1u << 24) /* ... and invalidated its copy in L1-D (invalidateCacheLineInL1, l2:124-131) */
#define GG_RES_UPGRADE         (1u << 28) /* WRITE to a SHARED L2 line: INV_REP + EX_REQ (l2:260-282) */

/* Cache counters, one vector per (tile, level).  Index = what Cache::outputSummary prints. */
enum {
  GG_CC_ACCESSES = 0, GG_CC_MISSES, GG_CC_READ_ACCESSES, GG_CC_READ_MISSES,
  GG_CC_WRITE_ACCESSES, GG_CC_WRITE_MISSES, GG_CC_EVICTIONS, GG_CC_DIRTY_EVICTIONS,
  GG_CC_TAG_READS, GG_CC_TAG_WRITES, GG_CC_DATA_READS, GG_CC_DATA_WRITES,
  GG_NUM_CACHE_COUNTERS
};

/* Network counters per tile (NetworkModel::outputSummary + model event counters). */
enum {
  GG_NC_PACKETS_SENT = 0, GG_NC_FLITS_SENT, GG_NC_BITS_SENT,
  GG_NC_PACKETS_RECEIVED, GG_NC_FLITS_RECEIVED, GG_NC_BITS_RECEIVED,
  GG_NC_TOTAL_LATENCY_PS, GG_NC_TOTAL_CONTENTION_PS,
  /* emesh_hop_counter: updateEventCounters (network_model_emesh_hop_counter.cc:120-127)
   * emesh_hop_by_hop : mesh RouterModel event counters + link traversals    */
  GG_NC_BUFFER_WRITES, GG_NC_BUFFER_READS, GG_NC_SWITCH_ALLOC, GG_NC_CROSSBAR,
  GG_NC_LINK_TRAVERSALS,
  GG_NC_ROUTER_CONTENTION_CYCLES, GG_NC_ROUTER_PACKETS, GG_NC_ANALYTICAL_REQUESTS,
  /* emesh_hop_by_hop with contention: QueueModel utilization counters of the 5
   * mesh output-port queues (queue_model.cc:49-55), + port (SELF, LEFT, RIGHT,
   * DOWN, UP), for RouterModel::getAverageLinkUtilization (router_model.cc:168-182) */
  GG_NC_PORT_UTILIZED_CYCLES,
  GG_NC_PORT_LAST_CYCLES = GG_NC_PORT_UTILIZED_CYCLES + 5,
  /* broadcasts (gg_noc_route_tree): updateSendCounters' broadcast totals
   * (network_model.cc:244-250) and RouterModel::updateEventCounters'
   * Crossbar[2..5] traversals (router_model.cc:126; GG_NC_CROSSBAR = Crossbar[1]) */
  GG_NC_PACKETS_BROADCASTED = GG_NC_PORT_LAST_CYCLES + 5,
  GG_NC_FLITS_BROADCASTED, GG_NC_BITS_BROADCASTED,
  GG_NC_CROSSBAR_MULTI,                 /* + (ports - 2), ports = 2..5 */
  GG_NUM_NET_COUNTERS = GG_NC_CROSSBAR_MULTI + 4
};

/* Queue model types (the type strings of QueueModel::create) and the
 * moving averages of queue_model/basic (MovingAverage::createAvgType,
 * common/misc/moving_average.h).  history_list uses max_list_size and
 * analytical_enabled below (queue_model/history_list, same defaults).    */
enum { GG_QM_HISTORY_TREE = 0, GG_QM_HISTORY_LIST = 1, GG_QM_BASIC = 2 };
enum { GG_MAVG_ARITHMETIC_MEAN = 0, GG_MAVG_MEDIAN = 1, GG_MAVG_NONE = 2 /* moving_avg_enabled = false */,
       GG_MAVG_GEOMETRIC_MEAN = 3 /* not supported: GG_ERR_UNSUPPORTED */ };

typedef struct gg_config {
  uint32_t num_tiles;          /* application tiles (general/total_cores)          */
  uint32_t line_size;          /* bytes, l1_dcache/T1/cache_line_size (64)          */
  uint32_t l1d_size_kb;        /* l1_dcache/T1/cache_size (32)                      */
  uint32_t l1d_assoc;          /* l1_dcache/T1/associativity (4)                    */
  uint32_t l1d_policy;         /* GG_POLICY_*                                        */
  uint32_t l2_size_kb;         /* l2_cache/T1/cache_size (512)                      */
  uint32_t l2_assoc;           /* l2_cache/T1/associativity (8)                     */
  uint32_t l2_policy;
  uint32_t net_model;          /* GG_NET_* for network/memory                        */
  uint32_t flit_width;         /* bits (64)                                          */
  uint32_t router_delay;       /* cycles (1)                                         */
  uint32_t link_delay;         /* cycles (1)                                         */
  uint32_t queue_model_enabled;/* network/emesh_hop_by_hop/queue_model/enabled       */
  uint32_t max_list_size;      /* queue_model/history_tree/max_list_size (100)      */
  uint32_t analytical_enabled; /* queue_model/history_tree/analytical_model_enabled */
  uint32_t total_tiles;        /* app tiles + MCP + spawners (config.cc:77-82); 0 = num_tiles+2 */
  double   frequency_ghz;      /* single DVFS domain (carbon_sim.cfg:147-155)        */
  int32_t  device;             /* HIP device ordinal                                 */
  uint32_t replay_kernel;      /* 0 = single-pass streaming replay where instantiated (else 2),
                                  1 = sharded generic replay, 2 = sharded lean replay */
  /* ---- coherent mode (pr_l1_pr_l2_dram_directory_msi with directory, DRAM, NoC) ---- */
  uint32_t l1d_data_cycles;    /* l1_dcache/T1/data_access_time (1)                 */
  uint32_t l1d_tags_cycles;    /* l1_dcache/T1/tags_access_time (1)                 */
  uint32_t l2_data_cycles;     /* l2_cache/T1/data_access_time (8)                  */
  uint32_t l2_tags_cycles;     /* l2_cache/T1/tags_access_time (3)                  */
  uint32_t dir_assoc;          /* dram_directory/associativity (16)                 */
  uint32_t dir_total_entries;  /* dram_directory/total_entries, 0 = "auto"          */
  uint32_t dir_access_cycles;  /* dram_directory/access_time, 0 = "auto"            */
  uint32_t dram_latency_ns;    /* dram/latency (100)                                */
  float    dram_bandwidth;     /* dram/per_controller_bandwidth, GB/s (5.0)         */
  uint32_t dram_queue_model_enabled; /* dram/queue_model/enabled (history_tree)     */
  uint32_t quantum_ns;         /* clock_skew_management/lax_barrier/quantum (1000)  */
  uint32_t num_shards;         /* logical shards (canonical schedule); 0 = 1 */
  uint32_t shard_begin;        /* shards owned by this context: [shard_begin, shard_end) */
  uint32_t shard_end;          /* 0 = all                                            */
  /* ---- queue models (QueueModel::create, shared_models/queue_model.cc:19-39) ---- */
  uint32_t queue_model_type;   /* network/emesh_hop_by_hop/queue_model/type: GG_QM_* (0 = history_tree) */
  uint32_t dram_queue_model_type; /* dram/queue_model/type: GG_QM_*                 */
  uint32_t basic_moving_avg;   /* queue_model/basic: moving_avg_window_size in bits 0..15
                                  (0 = 64) | GG_MAVG_* << 16 (0 = arithmetic_mean)  */
  uint32_t history_list_no_interleaving; /* queue_model/history_list/interleaving_enabled = false */
  /* ---- miss-type classification (Cache track_miss_types, cache.cc:321-405) ---- */
  uint32_t l1i_track_miss_types; /* l1_icache/T1/track_miss_types (false): the L1-D takes THIS flag
                                    (L1CacheCntlr passes the L1-I one to both, l1_cache_cntlr.cc:69) */
  uint32_t l2_track_miss_types;  /* l2_cache/T1/track_miss_types (false)               */
  uint32_t miss_track_lines;     /* coherent mode, when tracking: address-set capacity per
                                    (tile, cache) in lines, a power of two; 0 = 65536.
                                    The sets keep every line ever fetched, evicted or
                                    invalidated, so size it from the trace's per-tile
                                    footprint; allocated when tracking is on:
                                    tiles x 2 x lines x 8 B (65536: 1 GiB at 1024 tiles,
                                    4 GiB at 4096).  A full table stops the run with
                                    GG_ERR_UNSUPPORTED (no set entry is overwritten).
                                    Also the default capacity of the private replay's
                                    table (gg_cache_track_miss_types with lines = 0). */
  /* ---- caching protocol (caching_protocol/type, carbon_sim.cfg:184) ---- */
  uint32_t protocol;             /* GG_PROTO_*: pr_l1_pr_l2_dram_directory_msi (0) / _mosi (1) /
                                    pr_l1_sh_l2_msi (2) / pr_l1_sh_l2_mesi (3)                */
  uint32_t l1d_track_miss_types; /* l1_dcache/T1/track_miss_types (false): read by the MOSI
                                    protocol only, whose L1CacheCntlr passes the L1-D flag to the
                                    L1-D (…mosi/l1_cache_cntlr.cc:68; MSI passes the L1-I one) */
} gg_config;

/* Caching protocols of the coherent mode (MemoryManager::createMMU,
 * memory_manager.cc:22-60).  pr_l1_sh_l2_msi: private L1s, the L2 a shared
 * slice per tile (home = line % tiles) whose lines hold the full-map
 * directory entries, a DRAM controller per tile reached by DRAM_FETCH /
 * DRAM_STORE messages; the l2_* geometry is one slice's, the dir_* fields are
 * not used.  pr_l1_sh_l2_mesi adds EXCLUSIVE L1 lines: a read of an uncached
 * line is answered SH_REP_EX, the exclusive owner is invalidated (INV_REQ,
 * answered FLUSH_REP when modified) or downgraded (DOWNGRADE_REQ, answered
 * WB_REP when modified, else DOWNGRADE_REP); its own message types count in
 * GG_CT_MSGS_SENT only.  MOSI's DramDirectoryCntlr picks "one sharer"
 * with the directory entry's own drand48 stream (DirectoryEntryFullMap::
 * getOneSharer, directory_entry_full_map.cc:67-74; misc/random.h), which the
 * reference seeds with time(NULL) when the entry is created: the canonical
 * schedule seeds every entry with GG_MOSI_RNG_SEED (one fixed second).      */
enum { GG_PROTO_MSI = 0, GG_PROTO_MOSI = 1, GG_PROTO_SHL2_MSI = 2, GG_PROTO_SHL2_MESI = 3 };
#define GG_MOSI_RNG_SEED 1

/* Miss types (Cache::MissType, cache.h:45-52), counted per (tile, cache). */
enum { GG_MT_COLD = 0, GG_MT_CAPACITY, GG_MT_SHARING, GG_NUM_MISS_TYPES = 3 };

/* Fill cfg with the reference defaults of carbon_sim.cfg for num_tiles tiles. */
void gg_config_default(gg_config* cfg, uint32_t num_tiles);

/* A batch of line accesses in tile-major program order (structure of arrays).
 * Records of tile t are [tile_offsets[t], tile_offsets[t+1]).  addr[i] is the
 * byte address of the accessed line (the low log2(line_size) bits are ignored,
 * as Cache::getTag does, cache.cc:495-498).  Addresses must be < 2^48.        */
typedef struct gg_trace {
  const uint64_t* addr_dev;
  const uint32_t* meta_dev;
  const uint64_t* tile_offsets;   /* host, num_tiles + 1 entries */
  uint64_t        num_records;
} gg_trace;

/* A batch of NoC packets.  Packet k: sender/receiver tile ids, modeled length
 * in bits (NetworkModel::getModeledLength, network_model.cc:185-200) and its
 * send time in picoseconds (NetPacket::time).                                 */
typedef struct gg_packets {
  const uint32_t* src_dev;
  const uint32_t* dst_dev;
  const uint32_t* length_bits_dev;
  const uint64_t* time_ps_dev;
  uint64_t        num_packets;
} gg_packets;

/* Per-packet result: time the packet is handed to the receiving tile
 * (after serialization, network_model.cc:142-150) and the zero-load /
 * contention split (Hop, network_model.cc:556-563).                            */
typedef struct gg_packet_out {
  uint64_t* arrival_ps_dev;
  uint64_t* zero_load_ps_dev;
  uint64_t* contention_ps_dev;
} gg_packet_out;

typedef struct gg_line_info {    /* CacheLineInfo / PrL2CacheLineInfo            */
  uint64_t tag;                  /* line address (addr >> log2 line); ~0 = invalid */
  uint32_t cstate;               /* GG_CSTATE_*                                   */
  uint32_t cached_loc;           /* GG_LOC_* (L2 only)                            */
} gg_line_info;

/* ------------------------------------------------------------------------
 * Coherent mode ("Mode C"): the full pr_l1_pr_l2_dram_directory_msi protocol —
 * L1CacheCntlr / L2CacheCntlr (l1_cache_cntlr.cc, l2_cache_cntlr.cc),
 * DramDirectoryCntlr with DirectoryCache + full-map entries
 * (dram_directory_cntlr.cc, cache/directory_cache.cc,
 * directory_schemes/directory_entry_full_map.cc), DramCntlr + DramPerfModel
 * (dram_cntlr.cc, performance_models/dram_perf_model.cc), the ShmemPerfModel
 * clock (performance_models/shmem_perf_model.cc), the memory network
 * (NetworkModel::routePacket) and the lax-barrier quantum
 * (clock_skew_management_schemes/lax_barrier_sync_*.cc) — driven in the
 * canonical schedule of DESIGN.md §Mode C.
 * ------------------------------------------------------------------------ */

/* ShmemMsg::Type (pr_l1_pr_l2_dram_directory_msi/shmem_msg.h:12-30); MOSI's
 * INV_FLUSH_COMBINED_REQ (…mosi/shmem_msg.h:20, numbered after WB_REQ there)
 * is 13 here so the MSI numbering stays as it is; pr_l1_sh_l2_msi's DRAM
 * messages (…sh_l2_msi/shmem_msg.h:26-30) follow it */
enum {
  GG_MSG_EX_REQ = 1, GG_MSG_SH_REQ, GG_MSG_INV_REQ, GG_MSG_FLUSH_REQ, GG_MSG_WB_REQ,
  GG_MSG_EX_REP, GG_MSG_SH_REP, GG_MSG_UPGRADE_REP, GG_MSG_INV_REP, GG_MSG_FLUSH_REP,
  GG_MSG_WB_REP, GG_MSG_NULLIFY_REQ, GG_MSG_INV_FLUSH_COMBINED_REQ,
  GG_MSG_DRAM_FETCH_REQ, GG_MSG_DRAM_STORE_REQ, GG_MSG_DRAM_FETCH_REP,
  GG_MSG_DOWNGRADE_REQ, GG_MSG_SH_REP_EX, GG_MSG_DOWNGRADE_REP   /* pr_l1_sh_l2_mesi (…sh_l2_mesi/shmem_msg.h:14-39) */
};

/* One ShmemMsg in flight (64 bytes).  The per-sender sequence number keeps
 * the per-channel FIFO order of the reference transports
 * (socktransport.cc:225,366).  A record is either a message for dst's inbox
 * (hop == GG_HOP_NONE) or, under emesh_hop_by_hop with several logical
 * shards, a packet still in the mesh, held at a shard edge: it has left the
 * output port of a router in one shard and continues at router `hop` of
 * another shard after the quantum boundary (arrival_ps = its time at `hop`,
 * contention so far = arrival_ps - send_ps - zero_load_ps).                 */
#define GG_HOP_NONE 0xFFFFFFFFu
typedef struct gg_cmsg {
  uint64_t addr;         /* line byte address                                   */
  uint64_t send_ps;      /* NetPacket::time when sent (MemoryManager::sendMsg)  */
  uint64_t arrival_ps;   /* time handed to the receiver, after the network      */
  uint64_t zero_load_ps; /* zero-load part of the network time so far           */
  uint32_t src, dst;     /* sender / receiver tile                              */
  uint32_t requester;    /* ShmemMsg::_requester                                */
  uint32_t seq;          /* per-sender sequence number                          */
  uint32_t type;         /* GG_MSG_*                                            */
  uint32_t link;         /* backend-private (ignored on import)                 */
  uint32_t hop;          /* GG_HOP_NONE, or the router tile of a held packet    */
  uint32_t single_rx;    /* ShmemMsg::_single_receiver of an INV_FLUSH_COMBINED_REQ
                            (…mosi/shmem_msg.h), else 0                          */
} gg_cmsg;

/* Logical shards: on a full W x H mesh (W = floor(sqrt
 * num_tiles)) the tiles of shard k are the 2-D block the reference gives
 * process k of num_shards under emesh_hop_by_hop
 * (NetworkModelEMeshHopByHop::computeProcessToTileMapping,
 * network_model_emesh_hop_by_hop.cc:367-433); otherwise contiguous tile
 * ranges.  Writes tile_shard[num_tiles]; GG_ERR_INVALID if a shard is empty. */
gg_status gg_shard_map(uint32_t num_tiles, uint32_t num_shards, uint32_t* tile_shard);

/* Per-access output word of the coherent mode: (latency_ps << 2) | level,
 * latency = Core::initiateMemoryAccess final - initial time (core.cc:245-251). */
enum { GG_LVL_L1 = 0, GG_LVL_L2 = 1, GG_LVL_DIR = 2, GG_LVL_SYNC = 3 /* a BARRIER record: latency = sync stall */ };

/* Per-tile statistics of the coherent mode, [tile][GG_NUM_TILE_STATS]. */
enum {
  GG_CT_CLOCK_PS = 0,        /* core clock after the tile's last access / barrier release */
  GG_CT_ACCESSES, GG_CT_L1_HITS, GG_CT_L2_HITS, GG_CT_L2_MISSES, GG_CT_LATENCY_PS,
  GG_CT_DIR_ACCESSES,        /* DirectoryCache::_total_directory_accesses (directory_cache.cc:97-100) */
  GG_CT_DIR_EVICTIONS,       /* _total_evictions                                      */
  GG_CT_DIR_BACK_INVALIDATIONS,
  GG_CT_DRAM_ACCESSES,       /* DramPerfModel::m_num_accesses (dram_perf_model.cc:110)  */
  GG_CT_DRAM_LATENCY_NS,     /* m_total_access_latency                                */
  GG_CT_DRAM_QUEUE_DELAY_NS, /* m_total_queueing_delay                                */
  GG_CT_DRAM_QUEUE_REQUESTS, /* QueueModel::_total_requests of the DRAM queue          */
  GG_CT_DRAM_QUEUE_ANALYTICAL,
  GG_CT_MSGS_SENT,           /* ShmemMsgs sent over the network (self-sends included)  */
  GG_CT_MSGS_RECEIVED,
  GG_CT_SENT_BY_TYPE,        /* + (type - 1), 11 entries                               */
  /* QueueModel utilization counters of the DRAM queue (queue_model.cc:49-55),
   * for DramPerfModel::outputSummary's "Queue Utilization" (dram_perf_model.cc:141-163) */
  GG_CT_DRAM_QUEUE_UTILIZED_NS = GG_CT_SENT_BY_TYPE + 11, /* _total_utilized_cycles */
  GG_CT_DRAM_QUEUE_LAST_NS,                               /* _last_request_time     */
  GG_CT_SENT_INV_FLUSH_COMBINED = 29,                     /* MOSI INV_FLUSH_COMBINED_REQs sent */
  /* pr_l1_sh_l2_msi (no INV_FLUSH_COMBINED_REQ there): its DRAM messages sent */
  GG_CT_SENT_DRAM_FETCH_REQ = 29, GG_CT_SENT_DRAM_STORE_REQ = 30, GG_CT_SENT_DRAM_FETCH_REP = 31,
  GG_NUM_TILE_STATS = 32
};

/* Per-tile protocol event counters of the MOSI controllers, [tile][GG_NUM_PROTO_STATS]
 * (DramDirectoryCntlr::updateShmemReqEventCounters / updateShmemReqLatencyCounters /
 * updateInvalidationEventCounters, …mosi/dram_directory_cntlr.cc:842-1023;
 * L2CacheCntlr::updateInvalidationCounters / updateEvictionCounters,
 * …mosi/l2_cache_cntlr.cc:596-636).  Times in picoseconds.  MSI: zeros.       */
enum {
  GG_PS_EXREQ = 0, GG_PS_EXREQ_MODIFIED, GG_PS_EXREQ_SHARED, GG_PS_EXREQ_UPGRADE, GG_PS_EXREQ_UNCACHED,
  GG_PS_EXREQ_SERIALIZATION_PS, GG_PS_EXREQ_PROCESSING_PS,
  GG_PS_SHREQ, GG_PS_SHREQ_MODIFIED, GG_PS_SHREQ_SHARED, GG_PS_SHREQ_UNCACHED,
  GG_PS_SHREQ_SERIALIZATION_PS, GG_PS_SHREQ_PROCESSING_PS,
  GG_PS_NULLIFY, GG_PS_NULLIFY_MODIFIED, GG_PS_NULLIFY_SHARED, GG_PS_NULLIFY_UNCACHED,
  GG_PS_NULLIFY_SERIALIZATION_PS, GG_PS_NULLIFY_PROCESSING_PS,
  GG_PS_INV_UNICAST, GG_PS_INV_BROADCAST, GG_PS_INV_SHARERS_UNICAST, GG_PS_INV_SHARERS_BROADCAST,
  GG_PS_INV_PROCESSING_UNICAST_PS, GG_PS_INV_PROCESSING_BROADCAST_PS,
  GG_PS_L2_INVALIDATIONS, GG_PS_L2_EVICTIONS, GG_PS_L2_DIRTY_EVICTIONS_EXREQ, GG_PS_L2_CLEAN_EVICTIONS_EXREQ,
  GG_PS_L2_DIRTY_EVICTIONS_SHREQ, GG_PS_L2_CLEAN_EVICTIONS_SHREQ,
  GG_NUM_PROTO_STATS = 32
};

/* Whole-run information, [GG_NUM_RUN_INFO]. */
enum { GG_RI_QUANTA = 0, GG_RI_STEPS, GG_RI_NET_MSGS, GG_RI_SELF_MSGS, GG_RI_BOUNDARY_MSGS,
       GG_RI_FINAL_QUANTUM, GG_NUM_RUN_INFO = 8 };

/* Result of one quantum on the shards a context owns. */
typedef struct gg_coherent_status {
  uint64_t steps;           /* steps run                                                */
  uint64_t boundary_msgs;   /* cross-shard records waiting for the quantum boundary      */
                            /* (messages + held hop-by-hop packets)                      */
  uint64_t min_next_ps;     /* earliest next-access start of a gated owned tile, ~0 if none */
  uint32_t active_tiles;    /* owned tiles whose trace is not finished                  */
  uint32_t blocked_tiles;   /* owned tiles waiting for EX_REP / SH_REP                  */
} gg_coherent_status;

typedef struct gg_ctx gg_ctx;

int         gg_abi_version(void);
const char* gg_last_error(void);

/* Create a context on cfg->device: allocates the device-resident cache state of
 * every tile (reset to the constructor state: all lines invalid, LRU ages =
 * way index, lru_replacement_policy.cc:5-18) and the NoC router state.        */
gg_ctx*   gg_create(const gg_config* cfg, gg_status* status);
void      gg_destroy(gg_ctx* ctx);
gg_status gg_reset(gg_ctx* ctx);

/* Private (decoupled) cache replay of a trace batch, continuing from the
 * context's cache state.  result_dev: one word per record (GG_RES_*), may be
 * NULL.  evicted_dev: L2-evicted line byte address per record or ~0, may be
 * NULL.  Asynchronous on stream (hipStream_t, NULL = default).  Counters
 * accumulate in the context (gg_cache_get_counters).                          */
gg_status gg_cache_access_batch(gg_ctx* ctx, const gg_trace* trace,
                                uint32_t* result_dev, uint64_t* evicted_dev,
                                void* stream);

/* Counters: out has num_tiles * 2 * GG_NUM_CACHE_COUNTERS entries laid out
 * [tile][level][counter].  Synchronizes the context's stream.                */
gg_status gg_cache_get_counters(gg_ctx* ctx, uint64_t* out);

/* Opt a context into miss-type tracking (Cache track_miss_types, cache.cc:321-405)
 * for the private replay and the Cache quartet.  Tracked caches, as in the
 * reference: the L1-D takes cfg.l1i_track_miss_types (l1_cache_cntlr.cc:69),
 * the L2 cfg.l2_track_miss_types; GG_ERR_INVALID with neither set.  A context
 * with a flag set that has not made this call keeps refusing
 * gg_cache_access_batch (GG_ERR_UNSUPPORTED).
 * lines: capacity of the address sets per (tile, cache) in lines; 0 means
 * cfg.miss_track_lines, and 65536 if that is 0 too; a power of two, at least
 * 8 x the L1-D sets and at most 2^26, else GG_ERR_INVALID.  Allocates
 * tiles x (tracked caches) x lines x 8 B; gg_reset empties the table and
 * zeroes the counts (the context stays opted in), gg_destroy frees it.
 * Only on a fresh private cache state: after gg_create or gg_reset, before any
 * batch or quartet call; GG_ERR_STATE otherwise (the sets would miss the
 * lines already resident).
 * Capacity rule: the table is partitioned by (tile, L1-D set), lines / L1-D
 * sets slots each, and keeps every distinct line a set ever installed.  A
 * run fails exactly when some (tile, L1-D set) has to hold more distinct lines
 * than lines / L1-D sets (both caches of a tile see the same lines, so one rule
 * covers both): gg_cache_get_counters and gg_cache_get_miss_types then return
 * GG_ERR_UNSUPPORTED, no slot is overwritten, and the miss-type counts are
 * void until gg_reset.  On an opted-in context every replay_kernel value
 * runs a tracking kernel: 0 streams for the default and the 16-way-L2 LRU
 * geometries and takes the sharded generic kernel elsewhere, 1 and 2 take the
 * sharded generic kernel.                                                    */
gg_status gg_cache_track_miss_types(gg_ctx* ctx, uint32_t lines);
/* The miss types of the private replay and the quartet: out
 * [tiles][2][GG_NUM_MISS_TYPES] (L1-D, L2), zeros for an untracked cache.
 * GG_ERR_INVALID on a context that is not opted in.  Synchronizes the
 * context's stream and reports device errors like gg_cache_get_counters.     */
gg_status gg_cache_get_miss_types(gg_ctx* ctx, uint64_t* out);

/* The Cache quartet on one tile's device-resident cache (slow path, one line
 * per call; used by the host mirror classes and the parity tests).           */
gg_status gg_cache_get_line_info(gg_ctx* ctx, uint32_t tile, int level,
                                 uint64_t addr, gg_line_info* out);
gg_status gg_cache_set_line_info(gg_ctx* ctx, uint32_t tile, int level,
                                 uint64_t addr, const gg_line_info* in);
gg_status gg_cache_access_line(gg_ctx* ctx, uint32_t tile, int level,
                               uint64_t addr, int is_store);
gg_status gg_cache_insert_line(gg_ctx* ctx, uint32_t tile, int level,
                               uint64_t addr, const gg_line_info* in,
                               int* eviction, uint64_t* evicted_addr,
                               gg_line_info* evicted_info);

/* NoC: route every packet of the batch through the configured EMesh model in
 * the canonical discrete-event order, continuing from the
 * context's router queue state.  Asynchronous on stream.                      */
gg_status gg_noc_route_batch(gg_ctx* ctx, const gg_packets* pk,
                             const gg_packet_out* out, void* stream);
/* NetPacket::BROADCAST (common/network/network.h:54) as a receiver id.     */
#define GG_BROADCAST 0xDEADBABEu
/* NoC with broadcasts: as gg_noc_route_batch, and packets whose dst is
 * GG_BROADCAST take the emesh_hop_by_hop broadcast tree
 * (network_model_emesh_hop_by_hop.cc:163-221: UP / DOWN by the router's row
 * against the sender's, LEFT / RIGHT in the sender's row, SELF at every
 * router; one RouterModel::processPacket per router over the port list,
 * router_model.cc:71-108, contention = the max over its ports) and are
 * received by every tile, the sender included.  emesh_hop_by_hop only (the
 * other models have no broadcast capability: network.cc:187-195 unrolls such
 * a packet into one unicast per tile, which the caller does with
 * gg_noc_route_batch).  out[k] is written for unicast packets; the deliveries
 * of the b-th broadcast packet of the batch (batch order) land in
 * bcast_out[b * num_tiles + tile], num_broadcasts = their count.  One device
 * walk in global (time, packet index) order: the router ports a broadcast
 * serves together couple the X and Y chains that gg_noc_route_batch runs
 * independently.  Asynchronous on stream.                                   */
gg_status gg_noc_route_tree(gg_ctx* ctx, const gg_packets* pk, const gg_packet_out* out,
                            const gg_packet_out* bcast_out, uint64_t num_broadcasts, void* stream);
/* out: num_tiles * GG_NUM_NET_COUNTERS, [tile][counter].                      */
gg_status gg_noc_get_counters(gg_ctx* ctx, uint64_t* out);

/* Stand-alone queue model of cfg.queue_model_type (QueueModel::create(type,
 * min_processing_time), queue_model.cc:19-39: history_tree by default,
 * history_list, basic) over a sequence of (pkt_time, processing_time)
 * requests; writes the queue delays.  Host pointers; used by the known-answer
 * test (tests/unit/history_tree) and the reference-harness fixtures.         */
gg_status gg_queue_delay_batch(gg_ctx* ctx, uint64_t min_processing_time,
                               const uint64_t* pkt_time, const uint64_t* proc_time,
                               uint64_t n, uint64_t* delay_out);

/* Coherent mode.  gg_coherent_begin resets the coherent state and binds a
 * tile-major trace of ALL tiles (meta bits 1..30 = gap cycles before the
 * access); only the owned shards' tiles replay.  access_out_dev receives one
 * word per record (GG_LVL_*), may be NULL.  gg_coherent_quantum runs quantum
 * q (lax barrier at (q+1) * quantum_ns) on the owned shards until no owned
 * tile can progress.  gg_coherent_export moves the cross-shard messages of the
 * quantum into out_dev (device, grouped by destination shard, ascending;
 * counts per shard into per_shard_counts, host, num_shards entries);
 * gg_coherent_import delivers messages for owned tiles (device pointer).
 * gg_coherent_run does the whole run on a context that owns every shard.   */
gg_status gg_coherent_begin(gg_ctx* ctx, const gg_trace* trace, uint64_t* access_out_dev, void* stream);
gg_status gg_coherent_quantum(gg_ctx* ctx, uint64_t q, gg_coherent_status* st);
gg_status gg_coherent_export(gg_ctx* ctx, gg_cmsg* out_dev, uint64_t cap, uint64_t* per_shard_counts);
gg_status gg_coherent_import(gg_ctx* ctx, const gg_cmsg* in_dev, uint64_t n);
gg_status gg_coherent_run(gg_ctx* ctx, const gg_trace* trace, uint64_t* access_out_dev, void* stream);
/* An ensemble: n independent coherent runs side by side in one set of
 * launches (a sweep over traces or over latency / cache-timing settings; a
 * 16- or 64-tile run alone leaves most of the card empty).  ctxs[i] is an
 * ordinary context of gg_create that owns every shard, traces[i] its trace,
 * access_out_dev[i] its output buffer (an entry, or the array, may be NULL).
 * Each instance does what gg_coherent_run does, bit for bit, and afterwards
 * every per-context getter (gg_coherent_get_stats, _get_miss_types,
 * _get_protocol_stats, gg_noc_get_counters, gg_dump_summary,
 * gg_core_model_run) works on each context as after a single run.
 * statuses[i] (may be NULL) receives instance i's status; the return value is
 * the first non-zero one, or GG_OK.  A device error in one instance (a
 * capacity, a deadlock) fails that instance alone, with gg_coherent_run's
 * status; the others run to their end.  Instances that finish or fail leave
 * the launches at the next batch boundary, so short runs do not pay for long
 * ones.
 * Launch-compatible contexts.  The contexts must derive the same launch
 * shape: device; num_tiles, num_shards, protocol and network model; the step
 * kernel variant (register-held history-tree queues with no miss-type
 * tracking, or the general form; MOSI; shared L2) and, under
 * emesh_hop_by_hop, the walker variant (pipeline or sweep, register queues
 * or not) with its block sizes and run counts.  The rule is applied to the
 * derived launch state, not to config fields: whatever leaves that state
 * alike may differ — the trace and its length (BARRIER records included),
 * frequency_ghz, every *_cycles latency, dram_latency_ns, dram_bandwidth,
 * router_delay, link_delay, quantum_ns, miss_track_lines, and max_list_size
 * as long as the queue form stays the same.  Dynamic LDS sizes need not
 * match: each instance lays out its own, the launch takes the largest.
 * GG_ERR_INVALID, with gg_last_error naming the first offending index and
 * field, for: n == 0, n > GG_MANY_MAX, a NULL context, a context listed
 * twice, a context that does not own every shard, an incompatible context
 * (compared with context 0).  These are found before any launch or any
 * change to a context's run state (a context that has never run gets its
 * coherent state allocated for the comparison, nothing more).
 * The persistent small-mesh kernel is never used here: its grid barrier
 * needs every workgroup of every instance resident at once, and a mistake
 * there hangs the device.  The per-step launches give bit-identical results
 * (gg_coherent_run has both forms).  Launches are not timed per kernel; the
 * "coherent_run" timer of gg_set_timing covers the whole call on ctxs[0].
 * One stream, one host thread; synchronous.
 * A context with a statistics trace configured is refused
 * (GG_ERR_UNSUPPORTED, naming the index).  A traced sweep is
 * gg_coherent_begin per context, then gg_coherent_advance_many (below),
 * which samples.                                                            */
#define GG_MANY_MAX 4096u
gg_status gg_coherent_run_many(gg_ctx* const* ctxs, uint32_t n, const gg_trace* traces,
                               uint64_t* const* access_out_dev, gg_status* statuses, void* stream);
/* An ensemble in legs, and with statistics traces: gg_coherent_advance_many
 * is to gg_coherent_run_many what gg_coherent_advance (below) is to
 * gg_coherent_run.  Every context has a begun run driven by the device loop
 * (gg_coherent_begin or gg_coherent_restore); the call drives all of them in
 * one set of launches on stream.  Instance i stops when its run is over or
 * when the quantum the device picked next is >= stop_quanta[i] (stop_quanta
 * NULL: ~0, never, for all).  next_quanta[i] and dones[i] (0 paused, 1 over,
 * 2 deadlock) receive what gg_coherent_advance(ctxs[i], stop_quanta[i], ...)
 * would return, statuses[i] (may be NULL) its status; for one instance the
 * call is indistinguishable from that one, whatever company it has:
 *  - An instance that is already over, or whose stop is <= its current next
 *    quantum, gets no launch and no change of state, reports its current
 *    (next, done) and never enters the launches.
 *  - Every other instance is resumed as gg_coherent_advance resumes it (the
 *    stop stored, the launch index restarted at 0 — for all of them together
 *    — a pending BARRIER release kept) and runs in the per-step launches, the
 *    only form an ensemble has, under every stop value.  Instances that
 *    finish, pause or fail leave the launches at the next batch boundary.
 *  - A device capacity error gives GG_ERR_UNSUPPORTED, a deadlock
 *    GG_ERR_STATE, a full sample buffer GG_ERR_UNSUPPORTED ("sample buffer");
 *    a failed instance ends alone, the others run on.  The return value is
 *    the first non-zero status, or GG_OK.
 *  - Each context's own last stream is synchronised before the first launch;
 *    afterwards the getters of a driven context wait on stream.
 * Statistics traces.  A context whose begun run has a trace
 * (gg_stats_trace_configure before gg_coherent_begin) is accepted.  The
 * launches of a slot are followed by one scan launch for all live instances
 * (k_stats_scan_many, grid (tiles, live instances)) while at least one of
 * them has a trace, none otherwise.  Traced and untraced instances, different
 * statistics bits, intervals and max_samples go together; each instance's
 * samples are those of a lone gg_coherent_run, bit for bit, and a full buffer
 * fails that instance only.  A sample due at a pause boundary is taken with
 * its real time_ns and repeat (section 4i's rule).
 * Snapshots stay per context: gg_coherent_snapshot on a paused instance gives
 * the bytes a lone context paused at the same quantum gives.
 * Rejections, all before any launch or any write to any context's state, each
 * naming the context index.  GG_ERR_INVALID: n == 0, n > GG_MANY_MAX, NULL
 * ctxs / next_quanta / dones, a NULL or repeated context, a context with no
 * begun run or one driven by gg_coherent_quantum / the round, a set that is
 * not launch-compatible (gg_coherent_run_many's rule, naming the field).
 * GG_ERR_UNSUPPORTED: a context that does not own every shard, an ATAC
 * context ("batch API only").
 * Not in scope: a multi-rank sweep, a snapshot holding several instances.
 * One stream, one host thread; synchronous.                                 */
gg_status gg_coherent_advance_many(gg_ctx* const* ctxs, uint32_t n, const uint64_t* stop_quanta,
                                   uint64_t* next_quanta, int* dones, gg_status* statuses, void* stream);
/* A coherent run in legs: pause at a quantum boundary, snapshot, restore
 * (DESIGN.md section 4i).
 * gg_coherent_advance runs the device-driven loop of gg_coherent_run from the
 * context's current state (after gg_coherent_begin or gg_coherent_restore, on
 * a context that owns every shard; else GG_ERR_UNSUPPORTED) until the run is
 * over (*done = 1; a deadlock: *done = 2 and gg_coherent_run's GG_ERR_STATE)
 * or the quantum the device picked to run next is >= stop_quantum (*done = 0,
 * *next_quantum = that quantum).  Quanta skipped as empty count: a stop
 * inside a skipped span returns the first quantum chosen, which is larger.
 * stop_quantum <= the current next quantum returns at once, with no launch
 * and no change of state.  stop_quantum = ~0 never pauses: begin +
 * advance(~0) is gg_coherent_run, bit for bit.  Traces with BARRIER records
 * are accepted (a pending release is carried across the pause).  A leg with a
 * finite stop takes the per-step launches on every mesh size; a leg with
 * stop = ~0 takes what gg_coherent_run takes.  The results do not depend on
 * where, or whether, a run was paused.  One begun run is driven either by
 * gg_coherent_advance or by gg_coherent_quantum / gg_round_*: the other
 * family returns GG_ERR_INVALID.  The getters (gg_coherent_get_stats,
 * gg_noc_get_counters, gg_stats_trace_get, ...) work on a paused run.
 *
 * gg_coherent_snapshot copies everything the continuation depends on into
 * host_buf: caches, directory and replaced entries with their sharer words,
 * request FIFOs, DRAM and router queues, tile step state, statistics and
 * counters, the quantum state, the record pools and lists as far as they are
 * live, the error words and, when configured, the miss-type tables and the
 * statistics trace with its configuration and samples.  The directory arrays
 * and the miss-type tables are packed on the device to the slots in use.  It
 * is valid at the device loop's clean point only: after gg_coherent_begin,
 * after a gg_coherent_advance (paused or over) or gg_coherent_run, after a
 * gg_coherent_restore; else GG_ERR_INVALID.  cap too small: GG_ERR_RANGE
 * with *bytes = the need (gg_coherent_snapshot_size returns it alone).
 * The trace and the access-word buffer are the caller's: words of records a
 * tile has passed are final, gg_coherent_restore binds access_out_dev and
 * writes only later records, so a caller who wants the whole array carries
 * its buffer across.
 * gg_coherent_restore resets the context as gg_coherent_begin does, then puts
 * the state back (the snapshot's statistics-trace configuration included).
 * The snapshot carries a format version, the gg_config bytes, the derived
 * launch state (environment knobs included) and tile_offsets;
 * GG_ERR_INVALID, with nothing changed and the context good for a fresh run,
 * for a different config, launch state or tile_offsets, a truncated or
 * corrupted buffer, a section past the buffer or of another size than the
 * context's own.
 * An ensemble in legs: gg_coherent_advance_many (above) pauses and resumes
 * many begun runs in one set of launches; snapshot and restore stay per
 * context.
 * Not in scope: the multi-rank round, a context that does not own every
 * shard (GG_ERR_UNSUPPORTED), changing any setting across a restore.        */
gg_status gg_coherent_advance(gg_ctx* ctx, uint64_t stop_quantum, uint64_t* next_quantum, int* done);
gg_status gg_coherent_snapshot_size(gg_ctx* ctx, uint64_t* bytes);
gg_status gg_coherent_snapshot(gg_ctx* ctx, void* host_buf, uint64_t cap, uint64_t* bytes);
gg_status gg_coherent_restore(gg_ctx* ctx, const gg_trace* trace, uint64_t* access_out_dev,
                              const void* host_buf, uint64_t bytes, void* stream);
/* A coherent run fed its trace in windows: the trace
 * and the access words need not be resident, or exist, before the first
 * launch.  Each tile is given a window of its records that starts at its
 * first unconsumed record and holds at least that one; a tile is final once
 * its window runs to the end of its trace.  The run pauses at a quantum
 * boundary before any quantum in which a tile that is not final could consume
 * the last record of its window; the caller installs the next windows and the
 * run goes on.  The results (access words, tile statistics, cache, NoC and
 * protocol counters, run info, miss types, statistics-trace samples) do not
 * depend on where the windows were cut, or on whether the trace was windowed.
 *
 * gg_coherent_begin_window is gg_coherent_begin with a first window: win's
 * tile_offsets index its own arrays, access_out_dev has win->num_records
 * words (or NULL).  final_tiles[num_tiles] (host): != 0 where the tile's
 * window runs to the end of its trace; NULL: no tile is final.  A tile with an
 * empty window must be final (GG_ERR_INVALID).  The context must own every
 * shard (GG_ERR_UNSUPPORTED); with cfg.l1d_data_cycles == 0 a record can cost
 * no time and no window bounds a quantum: GG_ERR_UNSUPPORTED.  Only
 * gg_coherent_advance drives the run; it takes the per-step launches on every
 * mesh size.
 *
 * gg_coherent_advance on a windowed run can return *done =
 * GG_ADV_NEED_WINDOW: paused at the device loop's clean point because the
 * quantum picked to run next (*next_quantum, as at a pause) is not safe for
 * some tile that is not final.  Windows already too short for the next
 * quantum give it at once, with no launch.  A stop_quantum reached at the same
 * boundary returns *done = 0 as ever, and the next advance asks for the
 * windows.  A run that is not windowed never sees the value.
 *
 * gg_coherent_window_state: consumed[t] = the records tile t has consumed
 * since begin (the caller's index of the tile's first unconsumed record);
 * min_records[t] = the records the next window of a tile that is not final
 * must hold, counted from the first unconsumed record up to the window's last
 * record that is neither a GG_META_CONT line nor a BARRIER record, for the
 * next quantum to run at all (0 for final and finished tiles).  CONT lines and
 * BARRIER records after that record may follow in the window; they do not
 * count.  Both arrays are [num_tiles] on the host; either may be NULL.
 * Synchronizes.
 *
 * gg_coherent_next_window hands the next windows over.  It is valid only at
 * the clean point of a windowed run that is paused (*done 0 or
 * GG_ADV_NEED_WINDOW) or not yet advanced.  Tile t's records in win begin at
 * the tile's first unconsumed record, the record consumed[t] of its trace; a
 * tile that was final and has finished has an empty range.  A device kernel
 * rebases every tile's position to the new arrays, checks that the first
 * record of every unfinished tile equals, in addr and meta, the record the
 * tile stands on (a blocked tile's pending record, whose access word is
 * still to be written, goes to the new access_out_dev), and stores the final
 * flags.  GG_ERR_INVALID with nothing changed: a first record that differs,
 * an unfinished tile with an empty range, a final tile made non-final or
 * given another number of remaining records, a finished tile with records, a
 * run that is over or has failed, a run that is not windowed.  After the call
 * returns the old arrays belong to the caller again; their access words for
 * consumed records are final, and the word of record consumed[t] + i of tile t
 * is word i of the tile's range in the buffer bound while it was consumed.
 *
 * The backstop: should a tile that is not final ever reach the end of its
 * window, the run ends with GG_ERR_STATE ("window exhausted"), never with
 * *done = 1 and never with a result.
 * On a windowed run gg_coherent_snapshot / _snapshot_size (their snapshot
 * names positions in a resident trace: use gg_coherent_window_snapshot /
 * _window_restore below), gg_coherent_advance_many, gg_coherent_run_many and
 * gg_core_model_run (it needs the whole trace) return GG_ERR_UNSUPPORTED;
 * gg_coherent_quantum and gg_round_* return GG_ERR_INVALID as for any
 * advance-driven run.  A later gg_coherent_begin, _run or _restore on the
 * context starts an ordinary run. */
#define GG_ADV_NEED_WINDOW 3
gg_status gg_coherent_begin_window(gg_ctx* ctx, const gg_trace* win, uint64_t* access_out_dev,
                                   const uint8_t* final_tiles, void* stream);
gg_status gg_coherent_next_window(gg_ctx* ctx, const gg_trace* win, uint64_t* access_out_dev,
                                  const uint8_t* final_tiles, void* stream);
gg_status gg_coherent_window_state(gg_ctx* ctx, uint64_t* consumed, uint64_t* min_records);
/* A windowed run in legs: its snapshot and restore (DESIGN.md sections 4i, 4j).
 *
 * gg_coherent_window_snapshot / _size are gg_coherent_snapshot / _size for a
 * run fed in windows, valid at its clean point: after
 * gg_coherent_begin_window, after a gg_coherent_advance that returned *done 0,
 * GG_ADV_NEED_WINDOW or 1, after gg_coherent_next_window, after
 * gg_coherent_window_restore.  The container is the same with one more
 * section, `win`: per tile the records consumed since begin, a finished flag
 * and, for an unfinished tile, addr and meta of the record it stands on.
 * Positions are stored as counts of consumed records, so the bytes do not
 * depend on where the windows were cut: the final flags, the guards, the
 * horizon and the bound arrays are not part of it.  The run is left exactly as
 * it was.  GG_ERR_INVALID: a run that is not windowed (gg_coherent_snapshot
 * takes it), a run that has failed (error word set, "window exhausted").
 * GG_ERR_RANGE with *bytes = the need when cap is too small.
 *
 * gg_coherent_window_restore resets the context as gg_coherent_begin does,
 * puts the state back (the statistics-trace configuration and the miss-type
 * tables included) and installs win as gg_coherent_next_window would: tile
 * t's range begins at record consumed[t] of its trace, final_tiles as in
 * gg_coherent_begin_window, a blocked tile's pending record goes to the new
 * access_out_dev.  Afterwards the run is windowed and driven by
 * gg_coherent_advance; windows too short for the next quantum are no error
 * (the next advance returns GG_ADV_NEED_WINDOW with no launch).
 * GG_ERR_INVALID, with nothing changed and the context good for a fresh run:
 * whatever gg_coherent_restore refuses (config, launch state, section sizes,
 * a truncated or corrupted buffer), a snapshot without a `win` section
 * (gg_coherent_restore takes it), a first record that differs in addr or meta
 * from the stored one, an unfinished tile with an empty range, a finished
 * tile with records, a tile that is not final with an empty window.
 * GG_ERR_UNSUPPORTED as for gg_coherent_begin_window.  gg_coherent_restore
 * given a snapshot with a `win` section returns GG_ERR_INVALID.
 *
 * gg_window_snapshot_state reads consumed[num_tiles] and finished[num_tiles]
 * (host; either may be NULL) out of such a snapshot, with no context and no
 * device: a fresh process cuts its first windows from the file alone.
 * GG_ERR_INVALID with the parser's reason otherwise.                        */
gg_status gg_coherent_window_snapshot_size(gg_ctx* ctx, uint64_t* bytes);
gg_status gg_coherent_window_snapshot(gg_ctx* ctx, void* host_buf, uint64_t cap, uint64_t* bytes);
gg_status gg_coherent_window_restore(gg_ctx* ctx, const gg_trace* win, uint64_t* access_out_dev,
                                     const uint8_t* final_tiles, const void* host_buf, uint64_t bytes, void* stream);
gg_status gg_window_snapshot_state(const void* host_buf, uint64_t bytes, uint32_t num_tiles, uint64_t* consumed,
                                   uint8_t* finished);
/* The coherent mode over ranks (one process per GPU), RCCL over xGMI.
 * nccl_comm is an ncclComm_t (RCCL) of W ranks; rank r's context must own
 * logical shards [r*K/W, (r+1)*K/W) (cfg.shard_begin / shard_end, K =
 * num_shards).  gg_round_exchange runs quantum q's steps on the context,
 * sends the held cross-shard records to the ranks that own their shards and
 * receives this rank's (grouped ncclSend / ncclRecv on stream), all-gathers
 * the ranks' status words and imports the records, with one host sync (a
 * rank whose step batch was short repeats the round); *next_q is the quantum
 * every rank runs next and *done 1 when the run is over (GG_ERR_STATE on a
 * deadlock).  BARRIER records are released by the round: when the gathered
 * words show nothing in flight, no tile blocked on a miss and every
 * unfinished tile of every rank waiting at a barrier, each rank's commit
 * kernel stores the latest arrival and step 0 of quantum q + 1 continues the
 * waiters there (no further host sync; *next_q = q + 1).  While only some
 * tiles wait, the others run on; tiles that finish leave the count.
 * It replaces the reference's per-message transport
 * (common/transport/socktransport.cc) plus its lax barrier round
 * (lax_barrier_sync_client.cc:31-69, lax_barrier_sync_server.cc:57-160).
 * gg_coherent_run_ranks = gg_coherent_begin + rounds from quantum 0 until done. */
gg_status gg_round_exchange(gg_ctx* ctx, void* nccl_comm, void* stream, uint64_t q, uint64_t* next_q, int* done);
gg_status gg_coherent_run_ranks(gg_ctx* ctx, void* nccl_comm, const gg_trace* trace, uint64_t* access_out_dev,
                                void* stream);
/* The round of gg_round_exchange split at its transport, for a caller that
 * moves the bytes itself (another transport, or several contexts on one GPU
 * with device copies).  gg_round_exchange is exactly: pack -> transport ->
 * unpack, again while unpack says GG_ROUND_AGAIN, and on GG_ROUND_OVERFLOW a
 * second transport of the remainder -> gg_round_finish.
 *   gg_round_pack: quantum q's steps (a batch sized from the quanta before,
 *     doubled on each repeat) and the tail kernel: the held cross-rank
 *     records into per-peer send slots and this rank's status words; enqueued
 *     on the context's stream (gg_coherent_begin's), not synced.  Fills io.
 *     The checks of world / rank / shard ownership fail before anything is
 *     enqueued (they fail alike on every rank); a failure of the steps or the
 *     tail becomes the error flag of this rank's status words instead, so the
 *     transport still runs and every rank's unpack returns the error.
 *   transport 1: once the context's stream has finished the pack, for every
 *     r != rank: records [0, 1 + slot) of send + r * stride into rank r's
 *     recv + rank * stride; and words_own into words_all + rank *
 *     GG_ROUND_WORDS of every rank (this rank's too: an all-gather).  The
 *     words are opaque to the transport (their layout is internal: records
 *     sent, active / blocked tiles, flags + steps, largest slot, least next
 *     start, barrier waiters, their latest arrival).
 *   gg_round_unpack: commit (with the barrier release for the next quantum's
 *     step 0, decided from every rank's words) + import on the stream, the
 *     gathered words to the
 *     host, one sync; io->state = GG_ROUND_AGAIN (some rank's quantum had not
 *     finished: pack again with the same q), GG_ROUND_OVERFLOW (a slot held
 *     more than `slot` records: send_count[r] / recv_count[r] records are in
 *     send slot r / receive slot r; transport 2 moves records [1 + slot,
 *     1 + send_count[r]) of send slot r into rank r's receive slot `rank`,
 *     then gg_round_finish) or GG_ROUND_DONE (next_q / done as in
 *     gg_round_exchange).  Record 0 of a slot is a header whose addr is the
 *     slot's record count.
 *   A failure unpack or finish meets after the transport (commit / import)
 *   cannot reach the words the peers already hold: the rank decides that
 *   round like its peers (GG_OK, same state) and its next pack raises its
 *   error flag, so every rank's unpack of the next round returns the error
 *   (the failing rank its own message).  If that round ended the run there
 *   is no next round: the failing rank alone returns its error.  A new
 *   gg_coherent_begin drops a round left in progress (after AGAIN or an
 *   error): the next pack starts at step 0 of its quantum.                  */
enum { GG_ROUND_WORDS = 8, GG_ROUND_DONE = 0, GG_ROUND_AGAIN = 1, GG_ROUND_OVERFLOW = 2 };
typedef struct {
  gg_cmsg* send;                 /* device: [world][stride] records, the slots this rank sends */
  gg_cmsg* recv;                 /* device: [world][stride] records, the slots this rank receives */
  uint64_t* words_own;           /* device: [GG_ROUND_WORDS] this rank's status words */
  uint64_t* words_all;           /* device: [world][GG_ROUND_WORDS] every rank's (the all-gather's target) */
  uint64_t stride;               /* records per slot region (1 + capacity) */
  uint64_t slot;                 /* records of transport 1 per slot, header excluded */
  const uint64_t* send_count;    /* host [world]: records in send slot r (GG_ROUND_OVERFLOW) */
  const uint64_t* recv_count;    /* host [world]: records in receive slot r (GG_ROUND_OVERFLOW) */
  uint64_t next_q;               /* GG_ROUND_DONE: the quantum every rank runs next */
  int done;                      /* GG_ROUND_DONE: 1 when the run is over */
  int state;                     /* GG_ROUND_* after unpack / finish */
} gg_round_io;
gg_status gg_round_pack(gg_ctx* ctx, uint32_t world, uint32_t rank, uint64_t q, gg_round_io* io);
gg_status gg_round_unpack(gg_ctx* ctx, gg_round_io* io);
gg_status gg_round_finish(gg_ctx* ctx, gg_round_io* io);
/* tile_stats: [tiles][GG_NUM_TILE_STATS]; cache: [tiles][2][GG_NUM_CACHE_COUNTERS]
 * (either may be NULL); run_info: [GG_NUM_RUN_INFO] (may be NULL).  Tiles a
 * context does not own read 0.  Network counters: gg_noc_get_counters.      */
gg_status gg_coherent_get_stats(gg_ctx* ctx, uint64_t* tile_stats, uint64_t* cache, uint64_t* run_info);
/* The miss types of a coherent run with l1i_track_miss_types / l2_track_miss_types
 * set: out [tiles][2][GG_NUM_MISS_TYPES] (L1-D, L2), zeros for an untracked
 * cache.  Cache::getMissType (cache.cc:363-375) over the evicted /
 * invalidated / fetched address sets that insertCacheLine and
 * setCacheLineInfo keep (cache.cc:131-148, 228-230, 398-404).  The private
 * (Mode P) replay tracks them on a context opted in with
 * gg_cache_track_miss_types (counts: gg_cache_get_miss_types); without that
 * call gg_cache_access_batch returns GG_ERR_UNSUPPORTED when either flag is
 * set.                                                                       */
gg_status gg_coherent_get_miss_types(gg_ctx* ctx, uint64_t* out);
/* The MOSI event counters of a coherent run: out [tiles][GG_NUM_PROTO_STATS]
 * (zeros under MSI; tiles a context does not own read 0).                   */
gg_status gg_coherent_get_protocol_stats(gg_ctx* ctx, uint64_t* out);

/* The sim.out text of the context's statistics (replaces the per-tile
 * outputSummary chain: TileManager::outputSummary, tile_manager_summary.cc:
 * 60-244 -> Tile / MemoryManager / Cache / DramPerfModel / DirectoryCache /
 * Network summaries).  GG_SUMMARY_BLOCKS: one "Tile t Summary:" block per
 * tile; GG_SUMMARY_TABLE: TileManager's table (one column per tile).  Coherent
 * mode after gg_coherent_run: memory (L1-D, L2, DRAM, directory) and network
 * blocks; private-cache mode: the cache summaries and the network blocks.
 * *needed = the text's bytes + 1; buf (host, cap bytes) receives the
 * NUL-terminated text when it fits, else GG_ERR_RANGE (buf NULL: size query). */
enum { GG_SUMMARY_BLOCKS = 0, GG_SUMMARY_TABLE = 1 };
gg_status gg_dump_summary(gg_ctx* ctx, int format, char* buf, uint64_t cap, uint64_t* needed);

/* The [statistics_trace] time series of a coherent run (carbon_sim.cfg:396-411;
 * StatisticsThread, statistics_thread.cc:65-75: one sample whenever the lax
 * barrier releases at a multiple of sampling_interval).  Two statistics:
 *   GG_ST_NETWORK_UTILIZATION    network_utilization_memory.dat (network.cc:
 *     608-641): the flits sent, broadcast and received since the previous
 *     sample, summed over the tiles;
 *   GG_ST_CACHE_LINE_REPLICATION cache_line_replication.dat (…mosi/
 *     memory_manager.cc:491-602): the L1-D and L2 lines that are exclusive
 *     (MODIFIED) or shared (OWNED + SHARED) and the directories' histogram
 *     "entries with n sharers" (Directory::updateSharerStats, directory.cc:
 *     58-80; entries on the replaced list count until their NULLIFY ends).
 *     The L1-I is not simulated and contributes 0.
 * gg_stats_trace_configure sets the trace of the runs begun afterwards
 * (gg_coherent_begin / _run); statistics = 0 turns it off.  GG_ERR_INVALID:
 * an unknown statistics bit, an interval of 0 or not a multiple of
 * cfg.quantum_ns (carbon_sim.cfg:399), max_samples = 0 or a sample buffer
 * (max_samples * (GG_NUM_ST_FIELDS + num_tiles + 1) * 8 bytes, allocated whole
 * and zeroed at every begin) above GG_ST_MAX_BUFFER_BYTES.  GG_ERR_UNSUPPORTED:
 * cache_line_replication under the shared-L2 protocols (the reference has it
 * for pr_l1_pr_l2_dram_directory_mosi only, memory_manager.cc:200-212; MSI is
 * an extension here: same private-L2 formula, same data layout).
 * Sampling.  gg_coherent_run samples on the device, with no host round trip:
 * when quantum q ends and the run continues at quantum q' (empty quanta are
 * skipped), the lax barrier has passed the times (q+1)*quantum_ns ...
 * q'*quantum_ns; if multiples of the interval are among them, ONE sample is
 * taken of the state after q's last step: time_ns = the first such multiple,
 * repeat = how many there are (nothing happens in a skipped quantum: the
 * repeats are zero utilisation and the same replication state).  At the
 * run's last quantum only its own barrier counts (a partial last interval is
 * not emitted).  While a trace is configured gg_coherent_run uses the
 * per-step launches on every mesh size (the persistent small-mesh kernel
 * keeps cache state in LDS where a scan cannot see it); results are
 * bit-identical.  With no trace configured nothing changes: the same
 * launches, the same kernels.  gg_coherent_run_many and gg_coherent_run_ranks
 * return GG_ERR_UNSUPPORTED for a context with a trace configured (the counts
 * are additive over contexts: a rank samples its own shards with
 * gg_stats_trace_sample).  An ensemble of traced runs is gg_coherent_begin
 * per context, then gg_coherent_advance_many: one scan launch per slot for
 * all its live instances.
 * gg_stats_trace_sample appends one sample (repeat 1) of the context's
 * current state at barrier_time_ns: between the quanta of a host-driven run
 * (gg_coherent_quantum), or after a finished gg_coherent_run for the
 * end-of-run state.  Synchronizes.
 * A full sample buffer is an error (GG_ERR_UNSUPPORTED from the run or from
 * gg_stats_trace_sample), never a silently dropped sample.
 * gg_stats_trace_get: *count = samples taken; the first min(*count, cap)
 * samples into fields [cap][GG_NUM_ST_FIELDS] and sharer_hist
 * [cap][num_tiles + 1] (bin n = directory entries with n sharers, bin 0
 * unused; either may be NULL).  The integers are the contract: rates and
 * text derive from them on the host.
 * gg_stats_trace_dump: the text of one file (`which` = one GG_ST_* bit), as
 * the reference writes it (default ostream formatting, ", " separators with
 * the trailing ones, a blank line after each replication sample, vectors over
 * total_tiles = cfg.total_tiles or num_tiles + 2, and 2 * total_tiles);
 * buffer protocol as gg_dump_summary.  The replication-degree line is
 * computed from the raw counts in the reference's double arithmetic
 * (memory_manager.cc:563-599); where the reference indexes with an undefined
 * value (no shared L2 line: 0/0; an empty bin is harmless there only by
 * luck) empty bins are skipped and a ratio over zero shared L2 lines is 0. */
enum { GG_ST_NETWORK_UTILIZATION = 1, GG_ST_CACHE_LINE_REPLICATION = 2 };
#define GG_ST_MAX_BUFFER_BYTES (1ull << 30)
enum { GG_STF_TIME_NS = 0, GG_STF_REPEAT, GG_STF_FLITS_SENT, GG_STF_FLITS_BROADCASTED, GG_STF_FLITS_RECEIVED,
       GG_STF_L1_EXCLUSIVE, GG_STF_L1_SHARED, GG_STF_L2_EXCLUSIVE, GG_STF_L2_SHARED, GG_NUM_ST_FIELDS };
gg_status gg_stats_trace_configure(gg_ctx* ctx, uint32_t statistics, uint64_t sampling_interval_ns,
                                   uint64_t max_samples);
gg_status gg_stats_trace_sample(gg_ctx* ctx, uint64_t barrier_time_ns);
gg_status gg_stats_trace_get(gg_ctx* ctx, uint64_t* fields, uint64_t* sharer_hist, uint64_t cap, uint64_t* count);
gg_status gg_stats_trace_dump(gg_ctx* ctx, int which, char* buf, uint64_t cap, uint64_t* needed);

/* Synthetic workload generator (not part of the reference boundary; the
 * reference has no trace capture): fills a tile-major trace of
 * `per_tile` records for tiles [tile_begin, tile_begin + tiles) with the
 * configs[1] generator of DESIGN.md §Workloads — record i of tile t is
 * z = SplitMix64(0x9E3779B97F4A7C15 ^ t) step first+i+1, line = z mod 2^lines_log2
 * at byte base t << base_shift, WRITE iff (z >> 32) % 3 == 0.                */
gg_status gg_gen_uniform_trace(uint64_t* addr_dev, uint32_t* meta_dev, uint32_t tile_begin,
                               uint32_t tiles, uint64_t per_tile, uint64_t first,
                               uint32_t lines_log2, uint32_t base_shift, void* stream);

/* configs[2..4] hotspot generator: record i of tile t,
 * z = SplitMix64(0x9E3779B97F4A7C15 ^ t) step first+i+1; hot iff
 * ((z >> 40) & 0xFF) < hot_frac256 -> line (z & 0xFFFFFFFF) % hot_lines at byte
 * 1 << 44, else line z mod 2^lines_log2 at t << base_shift; WRITE iff
 * ((z >> 32) & 0xFF) % 3 == 0; gap = ctz(((z>>48)&0xFF)|0x100) +
 * ctz(((z>>56)&0xFF)|0x100) core cycles in meta bits 1..30.                 */
/* configs[4] coherent stress trace: record i of tile t
 * is z = SplitMix64(0x9E3779B97F4A7C15 ^ t) step first+i+1; WRITE iff bit 32 of
 * z; with probability pool_frac256/256 (bits 40-47) line
 * g(t) + G * ((z mod 2^32) mod (pool_lines / G)) of the shared pool at byte
 * 2^45, where G = max(1, num_tiles / 64) groups and g(t) the tile's group
 * (lowbias32 hash of t + 0x9E3779B9, mod G), so each pool line has ~64
 * sharers; else line z mod 2^lines_log2 at byte t << base_shift; gap cycles as
 * the hotspot trace.                                                         */
gg_status gg_gen_stress_trace(uint64_t* addr_dev, uint32_t* meta_dev, uint32_t tile_begin, uint32_t tiles,
                              uint64_t per_tile, uint64_t first, uint32_t lines_log2, uint32_t base_shift,
                              uint32_t num_tiles, uint32_t pool_lines, uint32_t pool_frac256, void* stream);
gg_status gg_gen_hotspot_trace(uint64_t* addr_dev, uint32_t* meta_dev, uint32_t tile_begin, uint32_t tiles,
                               uint64_t per_tile, uint64_t first, uint32_t lines_log2, uint32_t base_shift,
                               uint32_t hot_lines, uint32_t hot_frac256, void* stream);

/* Synthetic network traffic: the reference's NoC benchmark
 * tests/benchmarks/synthetic_network/synthetic_network.cc as an open-loop
 * packet batch.  Its sends are never held back by the receive window
 * (:177-208) and the lax barrier changes no timestamp, so the batch API
 * reproduces it once the packets exist; Random<double> (seeded with time() in
 * the reference) is SplitMix64 here.                                        */
enum { GG_TP_UNIFORM_RANDOM = 0, GG_TP_BIT_COMPLEMENT, GG_TP_SHUFFLE, GG_TP_TRANSPOSE,
       GG_TP_TORNADO, GG_TP_NEAREST_NEIGHBOR, GG_NUM_TRAFFIC_PATTERNS };
#define GG_NETPACKET_BYTES 64u   /* sizeof(NetPacket), network.h:27-55, x86-64 */
typedef struct gg_traffic_params {
  uint32_t pattern;          /* GG_TP_*                         (-p) */
  uint32_t packet_bytes;     /* payload bytes, default 8        (-s) */
  double   offered_load;     /* packets / tile / cycle, (0, 1]  (-l) */
  uint64_t packets_per_tile; /* default 10000                   (-N) */
  uint64_t seed;
} gg_traffic_params;
/* pattern uniform_random, 8 bytes, load 0.1, 10000 packets, seed 0. */
void      gg_traffic_params_default(gg_traffic_params* p);
/* Fills a tile-major batch: packet k of tile t at index t * N + k, N =
 * packets_per_tile; the four arrays hold num_tiles * N entries.
 *  - Destinations (synthetic_network.cc:232-359).  The mesh is w =
 *    floor(sqrt(T)), h = ceil(T / w); w * h != T is GG_ERR_INVALID (:347).
 *    bit_complement and shuffle need a power-of-two T (:290, :299), else
 *    GG_ERR_INVALID.  transpose, tornado and nearest_neighbor as written,
 *    non-square meshes included.  uniform_random: the LCG matrix
 *    send_matrix[i][j] (:238-252) equals orbit[i + j] with orbit[0] = T / 2,
 *    orbit[k + 1] = (13 * orbit[k] + 5) % T, so tile t sends packet k to
 *    orbit[(k % T) + t]; where a row or column is no permutation (:255-279
 *    asserts; T = 100 is such a count) GG_ERR_INVALID.
 *  - Injection (:180, :215-218).  s_t = SplitMix64(seed) step t + 1; at cycle
 *    c = 0, 1, ... the draw is z = SplitMix64(s_t) step c + 1, and the tile
 *    sends iff (z >> 11) < ceil(offered_load * 2^53), until it has sent N.
 *  - Fields.  time = c * Latency(1, frequency) ps (:206-207 adds ONE_CYCLE per
 *    iteration); length = (GG_NETPACKET_BYTES + packet_bytes) * 8 bits
 *    (network_model.cc:196-199, network.cc:705-708); a destination equal to
 *    the sender is kept.  last_cycle_dev[t] (may be NULL): the cycle of tile
 *    t's last packet.
 * GG_ERR_INVALID: a NULL array, a load outside (0, 1], an unknown pattern,
 * N = 0.  GG_ERR_RANGE: T * N >= 2^32 (the batch limit), N / offered_load >
 * 2^28 expected cycles.  GG_ERR_UNSUPPORTED: uniform_random beyond 2^20 tiles
 * (its table).  All before any launch.  A tile that reaches cycle 2^32 - 64
 * stops: GG_ERR_RANGE.  Synchronizes the stream.                            */
gg_status gg_gen_network_traffic(const gg_traffic_params* p, uint32_t num_tiles, double frequency_ghz,
                                 uint32_t* src_dev, uint32_t* dst_dev, uint32_t* length_bits_dev,
                                 uint64_t* time_ps_dev, uint64_t* last_cycle_dev /* [tiles], may be NULL */,
                                 void* stream);
/* One pass over a routed batch (the arrays of gg_noc_route_batch): what
 * the benchmark's users read off Network::outputSummary (network.cc:79-89),
 * per batch instead of per tile.  A packet with src == dst counts in
 * GG_NLS_SELF_PACKETS only.  stats: host, GG_NUM_NLS words (word 7 is 0).
 * Synchronizes the stream.                                                  */
enum { GG_NLS_PACKETS = 0 /* src != dst */, GG_NLS_SELF_PACKETS, GG_NLS_LATENCY_PS /* sum of arrival - time */,
       GG_NLS_ZERO_LOAD_PS, GG_NLS_CONTENTION_PS, GG_NLS_MAX_LATENCY_PS, GG_NLS_LAST_ARRIVAL_PS,
       GG_NLS_HIST = 8 /* + bit length of latency_ps: 0 for 0, else 64 - clz; 65 bins */,
       GG_NUM_NLS = GG_NLS_HIST + 65 };
gg_status gg_noc_latency_stats(const gg_packets* pk, const gg_packet_out* out,
                               uint64_t* stats /* host, GG_NUM_NLS */, void* stream);
/* The benchmark in one call: generates the packets of p for cfg.num_tiles
 * tiles at cfg.frequency_ghz, routes them with gg_noc_route_batch (continuing
 * from the context's queue state, under any network model the batch API
 * takes) and reduces the batch to stats.  The packet arrays are scratch of
 * the context, grown on demand.  Synchronizes the stream.                   */
gg_status gg_noc_synthetic_run(gg_ctx* ctx, const gg_traffic_params* p, uint64_t* stats, void* stream);

/* Many NoC batches side by side: a load-latency sweep is a
 * set of independent batches on independent contexts.  Instance i does what
 * gg_noc_route_batch(ctxs[i], &pks[i], &outs[i], stream) does, bit for bit —
 * the three output arrays, the context's NoC counters, the port-queue state a
 * later batch (single or _many) continues from, the deferred GG_ERR_RANGE of
 * gg_noc_get_counters for a packet naming no tile — but all instances share
 * one set of launches on stream (grid y = instance), about two dozen enqueues
 * for the whole set, with no host synchronisation.  Each instance uses the
 * state and scratch of its own context.  Not synchronised: as the single call.
 * Network models: emesh_hop_by_hop (with or without the queue model, any
 * queue-model type), emesh_hop_counter, magic.  An ATAC context:
 * GG_ERR_UNSUPPORTED for the whole call, naming the index.
 * Launch-compatible contexts.  The contexts must share the device, num_tiles
 * (hence the mesh w x h) and the network model, and under emesh_hop_by_hop the
 * stage-kernel form derived from the configuration, per X and Y stage: the
 * slab pipeline (max(w, h) <= 32), the position sweep, or the chain walk with
 * queues in HBM (side x queue image of max_list_size beyond the LDS budget).
 * The rule is applied to the derived state, not to config fields: everything
 * else may differ — the batch and its length, frequency_ghz, router_delay,
 * link_delay, flit_width, queue_model_enabled, the queue-model type and its
 * parameter, and max_list_size as long as the form stays the same.  The
 * fall-backs a stage kernel takes per chain or port (a long chain, a packet
 * of 2^16 flits or more, a non-tree queue model) depend on traffic and stay
 * per-instance decisions inside the kernel.
 * GG_ERR_INVALID (GG_ERR_UNSUPPORTED for ATAC), with gg_last_error naming the
 * first offending index and field, for: n == 0, n > GG_MANY_MAX, a NULL array
 * argument, a NULL or repeated context, an incompatible context (compared with
 * context 0), an ATAC context — before any launch and any change of a
 * context's state.  What gg_noc_route_batch would return for one instance's
 * own batch (a NULL packet or output pointer with num_packets > 0, 2^32
 * packets or more, a failed allocation) fails that instance alone, with that
 * status in statuses[i] (may be NULL); the others run.  num_packets == 0 is
 * GG_OK and leaves the context untouched.  Returns the first non-zero status,
 * or GG_OK.  Launches are not timed per kernel: the "noc_route_many" timer of
 * gg_set_timing covers the call on ctxs[0].                                  */
gg_status gg_noc_route_batch_many(gg_ctx* const* ctxs, uint32_t n, const gg_packets* pks, const gg_packet_out* outs,
                                  gg_status* statuses /* may be NULL */, void* stream);
/* gg_noc_synthetic_run for a set: instance i equals gg_noc_synthetic_run(
 * ctxs[i], &params[i], stats + i * GG_NUM_NLS, stream) — the same packets and
 * routed results in the context's scratch arrays, the same 73 words.  One
 * generator launch over (instance, tile), the routing of
 * gg_noc_route_batch_many, one reduction launch over the instances, one
 * device-to-host copy and one synchronisation for the whole call.  The
 * parameters of instance i are checked as gg_noc_synthetic_run checks them,
 * before any launch; a failure is that instance's status and the others run.
 * A generator that stops at cycle 2^32 - 64 is that instance's GG_ERR_RANGE
 * (it is not routed).  stats of a failed instance are not written.  Set-level
 * rejections as gg_noc_route_batch_many.                                     */
gg_status gg_noc_synthetic_run_many(gg_ctx* const* ctxs, uint32_t n, const gg_traffic_params* params,
                                    uint64_t* stats /* host, n * GG_NUM_NLS */,
                                    gg_status* statuses /* may be NULL */, void* stream);

/* Synthetic memory traffic: the instruction stream of the
 * reference's tests/benchmarks/synthetic_memory/synthetic_memory.cc as a
 * gg_trace that every coherent driver takes.  The benchmark seeds every Random
 * with the tile id and the address map with srandom(1), and its stream depends
 * on no simulated time, so a run is a function of its input file and the trace
 * is generated up front, bit for bit.
 *  - Input (:235-260): the eleven numbers of an input file; -ns overrides
 *    degree_of_sharing.  probability[]: NON_MEMORY, RD_ONLY_SHARED_READ,
 *    RD_WR_SHARED_READ, RD_WR_SHARED_WRITE, PRIVATE_READ, PRIVATE_WRITE.
 *    num_threads is the file's first number: 0 or the tile count of the call,
 *    else GG_ERR_INVALID.  T below is the tile count of the call.
 *  - Derived (:266-272): frac_ro = p[1] / (p[1] + p[2] + p[3]) in float; the
 *    cumulative probabilities by sequential float adds.
 *  - Address map (:314-334): srandom(map_seed); for shared address i in order
 *    and j < degree, tid = (int)((((float)random()) / RAND_MAX) * T) in float;
 *    line i goes on tid's read-only list if i < (int)(frac_ro * num_shared),
 *    else on its read-write list.  Duplicates stay, list order is push order.
 *    Drawn with random_r on a state of its own: random()'s state is untouched.
 *  - Per tile t (:285-296): three drand48_r streams (X' = (0x5DEECE66D X + 0xB)
 *    mod 2^48, X0 = (seed << 16) | 0x330E, u = X' 2^-48), all seeded with
 *    seed_base + t (its low 32 bits, as srand48_r keeps them): instruction
 *    type, read-only index, read-write index.
 *  - Per instruction (:143-228, :357-399): the type is the first i with
 *    (float)u < cum[i].  NON_MEMORY costs one cycle (the gap of the tile's
 *    next record).  A shared type whose list is empty on the tile does
 *    nothing: no draw, no time, no record.  Otherwise the address is list[(int)
 *    (u * size)] from the matching stream (reads and writes of read-write data
 *    share one).  Private access k of the tile (reads and writes counted
 *    together) goes to (1 << (log2(num_shared) + log2(line))) + ((t *
 *    num_private + k mod num_private) << log2(line)).  Every access is 4 bytes
 *    at a line-aligned address: one record.
 * Departures from the reference.  (1) It reads the key
 * l1_dcache/T1/cache_block_size, which no configuration has, and so shifts by
 * floorLog2(0) = -1; here the line size is line_bytes.  (2) frac_ro with a zero
 * denominator is 0.  (3) The final CarbonBarrierWait is left out: a BARRIER
 * record carries no gap, so the tile's trailing non-memory cycles could not
 * precede it, and the reported clock does not depend on it.                   */
enum { GG_MI_NON_MEMORY = 0, GG_MI_RD_ONLY_SHARED_READ, GG_MI_RD_WR_SHARED_READ, GG_MI_RD_WR_SHARED_WRITE,
       GG_MI_PRIVATE_READ, GG_MI_PRIVATE_WRITE, GG_NUM_MEM_INS_TYPES };
typedef struct gg_mem_traffic_params {
  uint32_t num_threads;            /* the file's thread count: 0, or the tile count of the call */
  uint32_t degree_of_sharing;      /* tiles drawn per shared address           (-ns) */
  uint32_t num_shared_addresses;   /* lines, a power of two                          */
  uint32_t num_private_addresses;  /* lines per tile, a power of two (or 0: none)    */
  uint64_t instructions_per_tile;  /* N                                              */
  float    probability[GG_NUM_MEM_INS_TYPES];
  uint64_t seed_base;              /* tile t seeds its three streams with seed_base + t; the reference: 0 */
  uint32_t map_seed;               /* srandom() seed of the address map; the reference: 1 */
  uint32_t reserved;               /* 0 */
} gg_mem_traffic_params;
/* The values of inputs/input.64: 64 threads, degree 1, 1024 shared and 256
 * private lines, 10000 instructions, 0.7 / 0.025 / 0.06 / 0.015 / 0.14 / 0.06,
 * seed_base 0, map_seed 1.                                                   */
void      gg_mem_traffic_params_default(gg_mem_traffic_params* p);
/* One function, called twice, because a tile's record count is only known
 * after a pass over its instructions.
 *  - Plan: addr_dev == NULL and meta_dev == NULL.  Draws the map, runs the
 *    count pass and writes tile_offsets[num_tiles + 1] (host) and *num_records.
 *  - Fill: addr_dev and meta_dev hold `capacity` records, capacity >= the
 *    plan's total (else GG_ERR_INVALID).  Repeats the plan (it keeps no state
 *    between calls; the count pass reads no memory but the lists) and writes
 *    addr_dev, meta_dev (WRITE bit; gap in bits 1..30 = NON_MEMORY instructions
 *    since the tile's previous access), tail_cycles_dev[T] (NON_MEMORY
 *    instructions after the tile's last access; u64) and type_counts_dev[T][6]
 *    (u64; every instruction counted, the skipped ones included).  The last
 *    two may be NULL, as may tile_offsets and num_records.
 * GG_ERR_INVALID: NULL p, one of addr_dev / meta_dev NULL, num_tiles == 0,
 * num_shared not a power of two (0 included), num_private not a power of two
 * and not 0, num_private == 0 with p[4] + p[5] > 0, degree > T, a probability
 * outside [0, 1] or not finite, N == 0, line_bytes not a power of two.
 * GG_ERR_RANGE: log2(num_shared) + log2(line) > 30 (the reference shifts an
 * int), T * num_private >= 2^31, N >= 2^31; and two limits of this
 * implementation: num_shared * degree >= 2^31 map entries, and (after the count
 * pass) a tile with 2^30 NON_MEMORY instructions or more, whose gap might not
 * fit 30 bits.  GG_ERR_STATE, where the reference
 * would assert or index out of range: a map draw gives tid == T ((float)
 * random() can round to 2^31); a tile draws from a list of more than 32768
 * entries; a type draw with (float)u >= cum[5] — found by the count pass and
 * reported after it, gg_last_error naming the lowest (tile, instruction).  All
 * but the last two before any launch.  Synchronizes the stream.            */
gg_status gg_gen_memory_traffic(const gg_mem_traffic_params* p, uint32_t num_tiles, uint32_t line_bytes,
                                uint64_t* tile_offsets /* host, num_tiles + 1; may be NULL */,
                                uint64_t* num_records /* may be NULL */,
                                uint64_t* addr_dev, uint32_t* meta_dev, uint64_t capacity,
                                uint64_t* tail_cycles_dev /* [tiles], may be NULL */,
                                uint64_t* type_counts_dev /* [tiles][6], may be NULL */, void* stream);
/* One pass over the access words (latency_ps << 2) | level of any coherent run
 * of trace (its meta_dev and num_records are read; tile_offsets is not).  A
 * BARRIER record is skipped; a GG_META_CONT record counts as an access of its
 * own line.  stats: host, GG_NUM_MLS words; words GG_MLS_TYPE_COUNTS ..
 * GG_MLS_HIST - 1 are 0.  Synchronizes the stream.                           */
enum { GG_MLS_RECORDS = 0, GG_MLS_READS, GG_MLS_WRITES,
       GG_MLS_L1_HITS, GG_MLS_L1_LATENCY_PS, GG_MLS_L2_HITS, GG_MLS_L2_LATENCY_PS,
       GG_MLS_L2_MISSES, GG_MLS_L2_MISS_LATENCY_PS, GG_MLS_MAX_LATENCY_PS,
       GG_MLS_TYPE_COUNTS = 10 /* + GG_MI_*: instructions of each type over all tiles (gg_mem_synthetic_run) */,
       GG_MLS_MAX_TILE_CLOCK_PS = 16 /* the benchmark's "Max Tile Clock" (gg_mem_synthetic_run) */,
       GG_MLS_HIST = 18 /* + bit length of latency_ps: 0 for 0, else 64 - clz; 65 bins */,
       GG_NUM_MLS = GG_MLS_HIST + 65 };
gg_status gg_mem_latency_stats(const gg_trace* trace, const uint64_t* access_out_dev,
                               uint64_t* stats /* host, GG_NUM_MLS */, void* stream);
/* The benchmark in one call: generates p's trace for cfg.num_tiles tiles and
 * the context's line size, runs it with gg_coherent_run and reduces the access
 * words.  Beyond the words of gg_mem_latency_stats: the total of each
 * instruction type, and GG_MLS_MAX_TILE_CLOCK_PS = max over tiles of
 * GG_CT_CLOCK_PS[t] + tail[t] * Latency(1, frequency) (:114-129).  The trace,
 * the access words, the tails and the counts are scratch of the context, grown
 * on demand and freed by gg_destroy.  Errors: those of gg_gen_memory_traffic
 * and gg_coherent_run; an ATAC context GG_ERR_UNSUPPORTED.  Synchronizes.    */
gg_status gg_mem_synthetic_run(gg_ctx* ctx, const gg_mem_traffic_params* p, uint64_t* stats /* host, GG_NUM_MLS */,
                               void* stream);
/* The arrays of the context's last gg_mem_synthetic_run, valid until its next
 * one or gg_destroy: the trace (tile_offsets owned by the context) to hand to
 * another driver, and the device arrays of the access words, tails [T] and
 * type counts [T][6] (each may be NULL).  GG_ERR_INVALID without such a run. */
gg_status gg_mem_synthetic_get(gg_ctx* ctx, gg_trace* trace, const uint64_t** access_out_dev,
                               const uint64_t** tail_cycles_dev, const uint64_t** type_counts_dev);
/* The same arrays copied into the caller's device buffers (num_records, T and
 * T * 6 entries; each may be NULL), for a caller that keeps them past the
 * context's next run.  Synchronizes the stream.                             */
gg_status gg_mem_synthetic_copy(gg_ctx* ctx, uint64_t* addr_dev, uint32_t* meta_dev, uint64_t* access_out_dev,
                                uint64_t* tail_cycles_dev, uint64_t* type_counts_dev, void* stream);

/* Multi-line accesses (replaces the line loop of Core::initiateMemoryAccess,
 * common/tile/core/core.cc:139-266, for the coherent mode).  Input: a
 * tile-major trace of accesses, device arrays addr_dev (byte address),
 * size_dev (bytes), meta_dev (WRITE bit, gap cycles), host tile_offsets
 * [tiles + 1].  Access i becomes the line records first_dev[i] ..
 * first_dev[i+1]-1 (first_dev: device, n + 1 entries): lines begin_aligned ..
 * end_aligned with the zero-size tail skipped (core.cc:167-197); the first
 * keeps the access's WRITE bit and gap, the others are WRITE | GG_META_CONT.
 * A zero-size access makes no line (core.cc:145-155); its gap cycles go to
 * the tile's next access.  line_addr_dev / line_meta_dev (capacity cap) may
 * both be NULL: then only *num_lines and first_dev are produced (size the
 * buffers, call again).  line_tile_offsets (host, may be NULL) receives the
 * line trace's tile offsets.  Synchronous on stream.  Errors: GG_ERR_INVALID
 * (bad arguments, more lines than cap, a carried gap >= 2^30 cycles).       */
gg_status gg_split_accesses(const uint64_t* addr_dev, const uint32_t* size_dev, const uint32_t* meta_dev,
                            const uint64_t* tile_offsets, uint32_t tiles, uint32_t line_size, uint64_t* first_dev,
                            uint64_t* line_addr_dev, uint32_t* line_meta_dev, uint64_t cap, uint64_t* num_lines,
                            uint64_t* line_tile_offsets, void* stream);
/* Per-access results of a coherent run of a split trace (core.cc:239-266):
 * latency_ps_dev[i] = final - initial time = the sum of the access's line
 * latencies (back to back); misses_dev[i] = its lines that did not hit the
 * L1-D on the first attempt (MemoryManager::__coreInitiateMemoryAccess's
 * return, l1_cache_cntlr.cc:100-179).  Either output may be NULL.           */
gg_status gg_combine_accesses(const uint64_t* line_out_dev, const uint64_t* first_dev, uint64_t n,
                              uint64_t* latency_ps_dev, uint32_t* misses_dev, void* stream);

/* Core timing of a trace-driven tile: the simple core model
 * (SimpleCoreModel::handleInstruction, common/tile/core/models/
 * simple_core_model.cc:43-96) over a coherent run's per-access results.  Each
 * access (a record without GG_META_CONT plus the CONT records that follow it)
 * is one instruction: static cost = its gap cycles (execution-unit stall),
 * one memory operand, read or write by the access's WRITE bit, whose latency
 * is the sum of its line latencies (Core::initiateMemoryAccess's final -
 * initial time, core.cc:239-256).  curr_time advances by cost + latency, which
 * is the coherent engine's clock rule, so GG_CORE_TIME_PS equals the run's
 * GG_CT_CLOCK_PS.  A BARRIER record whose access word holds a stall > 0 is
 * the SyncInstruction of sync_client.cc:306-314 (a dynamic instruction:
 * curr_time += stall, core_model.cc:237-240 counters).  No L1-I is modeled
 * (its stall is 0).  The iocoom model is
 * not offered: it needs register operands a memory trace does not carry and
 * would move the issue times the engine replays.
 * Per-tile statistics, [tile][GG_NUM_CORE_STATS]:                            */
enum {
  GG_CORE_INSTRUCTIONS = 0,   /* CoreModel::_instruction_count = data memory accesses  */
  GG_CORE_TIME_PS,            /* _curr_time                                             */
  GG_CORE_MEMORY_STALL_PS,    /* _total_memory_stall_time = total data access latency  */
  GG_CORE_EXECUTION_STALL_PS, /* _total_execution_unit_stall_time                      */
  GG_CORE_L1D_READ_STALL_PS,  /* SimpleCoreModel::_total_l1dcache_read_stall_time      */
  GG_CORE_L1D_WRITE_STALL_PS, /* _total_l1dcache_write_stall_time                      */
  GG_CORE_SYNC_INSTRUCTIONS,  /* _total_sync_instructions: released BARRIER records with a stall */
  GG_CORE_SYNC_STALL_PS,      /* _total_sync_instruction_stall_time                    */
  GG_NUM_CORE_STATS = 8
};
/* Runs the model over the tile-major trace (meta words and tile offsets of
 * `trace`; addresses are not read) and the per-record access words of the
 * coherent run (access_out_dev, (latency_ps << 2) | level), from the model's
 * constructor state; the statistics stay in the context (gg_core_get_stats,
 * gg_dump_summary's "Core Summary" block).  Asynchronous on stream.         */
gg_status gg_core_model_run(gg_ctx* ctx, const gg_trace* trace, const uint64_t* access_out_dev, void* stream);
/* out: num_tiles * GG_NUM_CORE_STATS (host).  Synchronizes.  GG_ERR_STATE if
 * gg_core_model_run has not run on the context.                              */
gg_status gg_core_get_stats(gg_ctx* ctx, uint64_t* out);

/* The iocoom core model (IOCOOMCoreModel, common/tile/core/models/
 * iocoom_core_model.cc; carbon_sim.cfg's default core type): an in-order core
 * with a register scoreboard and out-of-order memory through a load queue
 * and a store buffer.  Its time depends on register dependences, so it runs
 * over an INSTRUCTION stream, one gg_ins per instruction the core model
 * handles (CoreModel::iterate, core_model.cc:290-297), whose memory operands
 * take their DynamicMemoryInfo {address, read, latency} from an ACCESS
 * stream in order (Core::initiateMemoryAccess pushes one per access,
 * core.cc:258-263): per tile, the k-th memory operand of the instruction
 * stream (each instruction's reads, then its writes) is the k-th access.
 * The access stream's latencies are a coherent run's (gg_combine_accesses
 * of its line words, or its access words >> 2 for an unsplit trace): the
 * memory system is timed with the engine's issue times, and the core model
 * retimes the core around them (the reference feeds iocoom's curr_time back
 * as the next access's initial time; a trace carries no instructions between
 * its accesses to do that with).  Barriers likewise: a SYNC instruction
 * costs the stall the coherent engine measured (its release time minus the
 * engine's arrival time), taken as it is.  The reference's SyncClient
 * measures the stall on the core's own clock (sync_client.cc:308-313: time -
 * start_time); iocoom overlaps loads, so its arrival can be earlier and that
 * stall longer, and its clock after a barrier need not land on the common
 * release time.  Not recomputed here (nor in the oracle): parity unpinned.  */
typedef struct {
  uint16_t cost;     /* static cost in core cycles (Instruction::getCost: the
                        [core/static_instruction_costs] of its type, or a
                        branch's resolved cost); unused by a SYNC instruction */
  uint8_t  ops;      /* bits 0-1 memory read operands, bits 2-3 memory write
                        operands, GG_INS_SIMPLE_MOV_LOAD, GG_INS_ATOMIC,
                        GG_INS_FENCE_* in bits 6-7                             */
  uint8_t  regs;     /* bits 0-2 read registers, bits 3-5 write registers
                        (reads + writes <= 6), GG_INS_SYNC                     */
  uint16_t reg[6];   /* the read registers, then the write registers (< 512)  */
} gg_ins;
#define GG_INS_SIMPLE_MOV_LOAD 0x10u   /* Instruction::isSimpleMovMemoryLoad            */
#define GG_INS_ATOMIC          0x20u   /* Instruction::isAtomic (implicit MFENCE)        */
#define GG_INS_FENCE_SHIFT     6       /* 1 LFENCE, 2 SFENCE, 3 MFENCE (INST_*FENCE)    */
#define GG_INS_SYNC            0x80u   /* a SyncInstruction (dynamic): consumes the next
                                          access, which must be a BARRIER record, and
                                          costs its stall (sync_client.cc:306-314); a
                                          released barrier without a stall is no
                                          instruction, as in gg_core_model_run        */
#define GG_IOCOOM_NUM_REGISTERS 512    /* IOCOOMCoreModel::_NUM_REGISTERS               */
typedef struct {
  uint32_t num_load_queue_entries;             /* [core/iocoom] (1..64; default 8)    */
  uint32_t num_store_queue_entries;            /* (1..64; default 8)                   */
  uint32_t speculative_loads_enabled;          /* (default true)                       */
  uint32_t multiple_outstanding_RFOs_enabled;  /* (default true)                       */
} gg_iocoom_params;
/* Per-tile statistics, [tile][GG_NUM_IOCOOM_STATS]: */
enum {
  GG_IOCOOM_INSTRUCTIONS = 0,        /* CoreModel::_instruction_count                        */
  GG_IOCOOM_TIME_PS,                 /* _curr_time                                           */
  GG_IOCOOM_MEMORY_STALL_PS,         /* _total_memory_stall_time                             */
  GG_IOCOOM_EXECUTION_STALL_PS,      /* _total_execution_unit_stall_time                     */
  GG_IOCOOM_SYNC_INSTRUCTIONS,       /* _total_sync_instructions                             */
  GG_IOCOOM_SYNC_STALL_PS,           /* _total_sync_instruction_stall_time                   */
  GG_IOCOOM_LOAD_QUEUE_STALL_PS,     /* IOCOOMCoreModel::_total_load_queue_stall_time        */
  GG_IOCOOM_STORE_QUEUE_STALL_PS,    /* _total_store_queue_stall_time                        */
  GG_IOCOOM_L1I_STALL_PS,            /* _total_l1icache_stall_time (0: no L1-I)              */
  GG_IOCOOM_INTRA_L1D_STALL_PS,      /* _total_intra_ins_l1dcache_stall_time                 */
  GG_IOCOOM_INTER_L1D_STALL_PS,      /* _total_inter_ins_l1dcache_stall_time                 */
  GG_IOCOOM_INTRA_EXEC_STALL_PS,     /* _total_intra_ins_execution_unit_stall_time           */
  GG_IOCOOM_INTER_EXEC_STALL_PS,     /* _total_inter_ins_execution_unit_stall_time           */
  GG_IOCOOM_EXPLICIT_FENCES,         /* lfence + sfence + explicit mfence instructions       */
  GG_IOCOOM_IMPLICIT_MFENCES,        /* atomic instructions                                  */
  GG_IOCOOM_DATA_ACCESSES,           /* memory operands (Core's data memory accesses)        */
  GG_IOCOOM_DATA_LATENCY_PS,         /* their summed latency (Core::incrTotalMemoryAccessLatency) */
  GG_NUM_IOCOOM_STATS = 17
};
/* Runs IOCOOMCoreModel::handleInstruction over each tile's instructions
 * (ins_dev, host ins_tile_offsets[num_tiles + 1]) and accesses (acc_addr_dev
 * u64 address, acc_meta_dev u32 meta word — GG_META_WRITE or GG_META_BARRIER
 * — acc_lat_dev u64 latency in ps or a barrier's stall, host
 * acc_tile_offsets[num_tiles + 1]) from the model's constructor state.  A
 * memory read operand met by a write access (or the reverse), a SYNC met by
 * a non-BARRIER access, a register >= 512, a tile whose instructions leave
 * accesses unconsumed or run out of them, a register time of 2^62 ps or more
 * (the scoreboard keeps the unit in an entry's top two bits): the run's
 * error, reported by gg_iocoom_get_stats (GG_ERR_STATE).  GG_ERR_RANGE up
 * front for a tile of more than 2^28 instructions or 2^31 accesses.
 * Asynchronous on stream.                                                    */
gg_status gg_iocoom_run(gg_ctx* ctx, const gg_iocoom_params* params, const gg_ins* ins_dev,
                        const uint64_t* ins_tile_offsets, const uint64_t* acc_addr_dev, const uint32_t* acc_meta_dev,
                        const uint64_t* acc_lat_dev, const uint64_t* acc_tile_offsets, void* stream);
/* out: num_tiles * GG_NUM_IOCOOM_STATS (host).  Synchronizes.  GG_ERR_STATE
 * if gg_iocoom_run has not run on the context or its streams disagreed.    */
gg_status gg_iocoom_get_stats(gg_ctx* ctx, uint64_t* out);

/* ------------------------------------------------------------------------
 * ATAC (network/memory = atac; models/network_model_atac.cc): an electrical
 * mesh inside a cluster (ENet), an optical ring between the clusters' hubs
 * (ONet) and a receive network (star or broadcast tree) per cluster.  BATCH
 * API ONLY: gg_noc_route_batch and gg_noc_route_tree take a context whose
 * net_model is GG_NET_ATAC; gg_coherent_*, gg_round_* and
 * gg_coherent_run_many return GG_ERR_UNSUPPORTED on it.
 * The settings live here, apart from gg_config (whose layout is unchanged):
 * carbon_sim.cfg:318-352 and [link_model/optical] laser_modes (:366-370).
 * gg_config's flit_width, queue_model_enabled, queue_model_type,
 * max_list_size, analytical_enabled, basic_moving_avg,
 * history_list_no_interleaving and frequency_ghz are read as the
 * network/atac values.  Link delays are not settings: the reference asserts
 * 1 cycle for the ENet, star and B-tree links and 3 for the optical link
 * (network_model_atac.cc:213,229,250,281).                                  */
enum { GG_ATAC_STAR = 0, GG_ATAC_BTREE = 1 };                       /* receive_network_type */
enum { GG_ATAC_CLUSTER_BASED = 0, GG_ATAC_DISTANCE_BASED = 1 };     /* global_routing_strategy */
enum { GG_ATAC_LASER_UNICAST = 1, GG_ATAC_LASER_BROADCAST = 2 };    /* laser_modes bits */
/* The star stage serves a star router's cluster_size output ports with one
 * wave each in one workgroup of at most 1024 threads: cluster sizes above 16
 * are GG_ERR_UNSUPPORTED (star and B-tree alike).                           */
#define GG_ATAC_MAX_STAR_PORTS 16u
typedef struct gg_atac_params {
  uint32_t cluster_size;                /* network/atac/cluster_size (4)                         */
  uint32_t num_access_points;           /* num_optical_access_points_per_cluster (4)             */
  uint32_t receive_net_type;            /* GG_ATAC_STAR / GG_ATAC_BTREE (star)                   */
  uint32_t num_receive_nets;            /* num_receive_networks_per_cluster (2)                  */
  uint32_t global_routing;              /* GG_ATAC_CLUSTER_BASED / _DISTANCE_BASED (cluster)     */
  uint32_t unicast_distance_threshold;  /* (4)                                                   */
  uint32_t enet_router_delay;           /* enet/router/delay (1)                                 */
  uint32_t send_hub_router_delay;       /* onet/send_hub/router/delay (1)                        */
  uint32_t receive_hub_router_delay;    /* onet/receive_hub/router/delay (1)                     */
  uint32_t star_net_router_delay;       /* star_net/router/delay (1)                             */
  uint32_t laser_modes;                 /* bit 0 unicast, bit 1 broadcast (3)                    */
} gg_atac_params;
void gg_atac_params_default(gg_atac_params* p);
/* Validates p against the context's tile count (network_model_atac.cc:104-121),
 * (re)allocates the ATAC queues and resets the NoC state (queues and
 * counters).  A context created with net_model = GG_NET_ATAC starts with the
 * defaults.  GG_ERR_INVALID, the message naming the field: a tile count that
 * is not both a power of two and a perfect square, a cluster size or
 * access-point count that is not a power of two, access points > cluster
 * size, fewer than 2 clusters, num_receive_nets == 0, laser_modes == 0 or
 * above 3, an unknown receive_net_type / global_routing, or a context whose
 * model is not ATAC.  GG_ERR_UNSUPPORTED: cluster_size > GG_ATAC_MAX_STAR_PORTS. */
gg_status gg_noc_set_atac(gg_ctx* ctx, const gg_atac_params* p);
/* Host-only, like gg_shard_map: cluster_of[num_tiles] (getClusterID),
 * access_point_of[num_tiles] (getNearestAccessPoint), hub_of_cluster[num_tiles
 * / cluster_size] (getTileIDWithOpticalHub) and star_index_of[num_tiles] (the
 * tile's index in getTileIDListInCluster: x outer, y inner), any of which may
 * be NULL (network_model_atac.cc:587-745).  The checks of gg_noc_set_atac.   */
gg_status gg_atac_topology(uint32_t num_tiles, const gg_atac_params* p, uint32_t* cluster_of,
                           uint32_t* access_point_of, uint32_t* hub_of_cluster, uint32_t* star_index_of);
/* Event and contention counters of the ATAC components a tile owns
 * (RouterModel::updateEventCounters / updateContentionCounters,
 * router_model.cc:119-144; ElectricalLinkModel / OpticalLinkModel flit counts,
 * optical_link_model.cc:114-135), [tile][GG_NUM_ATAC_COUNTERS].  Per router
 * class R = ENET, SEND_HUB, RECEIVE_HUB, STAR_NET (summed over the receive
 * nets) at GG_AC_R + GG_ACR_*; the hub's components count on the hub's tile.
 * The injection router is not counted (as for the mesh).                     */
enum { GG_ACR_BUFFER_WRITES = 0, GG_ACR_SWITCH_ALLOC, GG_ACR_CROSSBAR_ONE /* flits over one output port */,
       GG_ACR_CROSSBAR_ALL /* flits over all output ports (a router of > 1 ports) */,
       GG_ACR_CONTENTION_CYCLES, GG_ACR_PORT_PACKETS, GG_NUM_ACR = 6 };
enum {
  GG_AC_ENET = 0, GG_AC_SEND_HUB = 6, GG_AC_RECEIVE_HUB = 12, GG_AC_STAR_NET = 18,
  GG_AC_ENET_LINK_FLITS = 24, GG_AC_OPTICAL_UNICAST_FLITS, GG_AC_OPTICAL_BROADCAST_FLITS,
  GG_AC_RECEIVE_NET_LINK_FLITS, GG_NUM_ATAC_COUNTERS
};
/* out: num_tiles * GG_NUM_ATAC_COUNTERS (host).  Synchronizes.  GG_ERR_INVALID
 * on a context whose model is not ATAC.  For such a context gg_noc_get_counters
 * fills packets / flits / bits sent and received, total latency, total
 * contention and the three *_BROADCASTED fields; the mesh router's fields
 * stay zero (they are here, under GG_AC_ENET).                              */
gg_status gg_noc_get_atac_counters(gg_ctx* ctx, uint64_t* out);

/* Device time (ms) of the most recent launch of a named kernel
 * ("cache_hist", "cache_scatter", "cache_replay", "cache_unshard",
 * "noc_hop_counter", ...), measured with HIP
 * events on the stream the kernel ran on; negative if not launched.           */
float     gg_kernel_time_ms(gg_ctx* ctx, const char* kernel);
/* enabled: 0 off; 1 on, coherent-mode launches sampled (an event pair around
 * every 16th launch of each kernel); 2 on, every coherent step / walk launch
 * timed in-kernel (first workgroup start to last workgroup end). */
void      gg_set_timing(gg_ctx* ctx, int enabled);
/* Launches since the last gg_coherent_begin of "coherent_step",
 * "coherent_walk_x", "coherent_walk_y" and their total device time: with
 * timing 1, (mean of the event-timed launches) x launches; with timing 2, the
 * sum of every launch's in-kernel span (s_memrealtime, 100 MHz).           */
gg_status gg_kernel_stats(gg_ctx* ctx, const char* kernel, double* total_ms, uint64_t* launches);

#ifdef __cplusplus
}
#endif
#endif
