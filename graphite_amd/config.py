"""Configuration of the batch backend: the ctypes mirror of ``gg_config``
(include/graphite_gpu.h) and the reference defaults of ``carbon_sim.cfg``.

Reference keys (nmtrmail/Graphite carbon_sim.cfg): l1_dcache/T1 (:219-228),
l2_cache/T1 (:230-239), network/emesh_* (:290-313), queue_model/history_tree
(:388-392), DVFS domain 1 GHz (:147-155).
"""
import ctypes
import math

import numpy as np

POLICY_LRU = 0
POLICY_ROUND_ROBIN = 1
NET_MAGIC = 0
NET_EMESH_HOP_COUNTER = 1
NET_EMESH_HOP_BY_HOP = 2
NET_ATAC = 3
# network/atac (carbon_sim.cfg:318-352): receive_network_type, global_routing_strategy
ATAC_STAR, ATAC_BTREE = 0, 1
ATAC_CLUSTER_BASED, ATAC_DISTANCE_BASED = 0, 1
ATAC_LASER_UNICAST, ATAC_LASER_BROADCAST = 1, 2
ATAC_MAX_STAR_PORTS = 16      # GG_ATAC_MAX_STAR_PORTS: largest cluster_size the star stage holds
# queue model types (QueueModel::create, queue_model.cc:19-39) and queue_model/basic moving averages
QM_HISTORY_TREE = 0
QM_HISTORY_LIST = 1
QM_BASIC = 2
MAVG_ARITHMETIC_MEAN = 0
MAVG_MEDIAN = 1
MAVG_NONE = 2
MAVG_GEOMETRIC_MEAN = 3

L1D = 0
L2 = 1

CSTATE_INVALID = 0
CSTATE_SHARED = 1
CSTATE_OWNED = 2      # MOSI
CSTATE_EXCLUSIVE = 3  # MESI
CSTATE_MODIFIED = 4
PROTO_MSI, PROTO_MOSI, PROTO_SHL2_MSI, PROTO_SHL2_MESI = 0, 1, 2, 3   # GG_PROTO_* (caching_protocol/type)
MOSI_RNG_SEED = 1                     # GG_MOSI_RNG_SEED
LOC_INVALID = 0
LOC_L1D = 3

META_WRITE = 1

RES_L1_MISS = 1 << 0
RES_L2_MISS = 1 << 4
RES_L1_INVAL = 1 << 8
RES_L1_EVICT = 1 << 12
RES_L2_EVICT = 1 << 16
RES_L2_EVICT_DIRTY = 1 << 20
RES_L2_EVICT_INV_L1 = 1 << 24
RES_UPGRADE = 1 << 28

CACHE_COUNTERS = ["accesses", "misses", "read_accesses", "read_misses",
                  "write_accesses", "write_misses", "evictions", "dirty_evictions",
                  "tag_reads", "tag_writes", "data_reads", "data_writes"]
NET_COUNTERS = ["packets_sent", "flits_sent", "bits_sent", "packets_received",
                "flits_received", "bits_received", "total_latency_ps",
                "total_contention_ps", "buffer_writes", "buffer_reads",
                "switch_alloc", "crossbar", "link_traversals",
                "router_contention_cycles", "router_packets", "analytical_requests"] + \
               ["port%d_utilized_cycles" % p for p in range(5)] + ["port%d_last_cycles" % p for p in range(5)] + \
               ["packets_broadcasted", "flits_broadcasted", "bits_broadcasted"] + \
               ["crossbar%d" % m for m in range(2, 6)]
BROADCAST = 0xDEADBABE   # NetPacket::BROADCAST (network.h:54), GG_BROADCAST
# gg_noc_get_atac_counters, [tile][NUM_ATAC_COUNTERS] (GG_AC_*): RouterModel event / contention
# counters (router_model.cc:119-144) per router class, then the link counters
ATAC_COUNTERS = ["%s_%s" % (r, c) for r in ("enet", "send_hub", "receive_hub", "star_net")
                 for c in ("buffer_writes", "switch_alloc", "crossbar_one", "crossbar_all",
                           "contention_cycles", "port_packets")] + \
                ["enet_link_flits", "optical_unicast_flits", "optical_broadcast_flits", "receive_net_link_flits"]
NUM_ATAC_COUNTERS = len(ATAC_COUNTERS)
NUM_CACHE_COUNTERS = len(CACHE_COUNTERS)

# coherent mode (include/graphite_gpu.h)
MSG_TYPES = ["EX_REQ", "SH_REQ", "INV_REQ", "FLUSH_REQ", "WB_REQ", "EX_REP", "SH_REP",
             "UPGRADE_REP", "INV_REP", "FLUSH_REP", "WB_REP"]
MSG = {n: i + 1 for i, n in enumerate(MSG_TYPES)}
MSG["NULLIFY_REQ"], MSG["INV_FLUSH_COMBINED_REQ"] = 12, 13
MSG["DRAM_FETCH_REQ"], MSG["DRAM_STORE_REQ"], MSG["DRAM_FETCH_REP"] = 14, 15, 16   # pr_l1_sh_l2_msi
MSG["DOWNGRADE_REQ"], MSG["SH_REP_EX"], MSG["DOWNGRADE_REP"] = 17, 18, 19            # pr_l1_sh_l2_mesi
CT_SENT_INV_FLUSH_COMBINED = 29       # GG_CT_SENT_INV_FLUSH_COMBINED (MOSI)
CT_SENT_DRAM_FETCH_REQ, CT_SENT_DRAM_STORE_REQ, CT_SENT_DRAM_FETCH_REP = 29, 30, 31   # pr_l1_sh_l2_msi
# MOSI event counters, [tile][NUM_PROTO_STATS] (GG_PS_*)
PROTO_STATS = ["exreq", "exreq_modified", "exreq_shared", "exreq_upgrade", "exreq_uncached",
               "exreq_serialization_ps", "exreq_processing_ps",
               "shreq", "shreq_modified", "shreq_shared", "shreq_uncached",
               "shreq_serialization_ps", "shreq_processing_ps",
               "nullify", "nullify_modified", "nullify_shared", "nullify_uncached",
               "nullify_serialization_ps", "nullify_processing_ps",
               "inv_unicast", "inv_broadcast", "inv_sharers_unicast", "inv_sharers_broadcast",
               "inv_processing_unicast_ps", "inv_processing_broadcast_ps",
               "l2_invalidations", "l2_evictions", "l2_dirty_evictions_exreq", "l2_clean_evictions_exreq",
               "l2_dirty_evictions_shreq", "l2_clean_evictions_shreq"]
NUM_PROTO_STATS = 32
LVL_L1, LVL_L2, LVL_DIR = 0, 1, 2
TILE_STATS = ["clock_ps", "accesses", "l1_hits", "l2_hits", "l2_misses", "latency_ps",
              "dir_accesses", "dir_evictions", "dir_back_invalidations",
              "dram_accesses", "dram_latency_ns", "dram_queue_delay_ns",
              "dram_queue_requests", "dram_queue_analytical", "msgs_sent", "msgs_received"] + \
             ["sent_" + n.lower() for n in MSG_TYPES] + ["dram_queue_utilized_ns", "dram_queue_last_ns"]
NUM_TILE_STATS = 32
RUN_INFO = ["quanta", "steps", "net_msgs", "self_msgs", "boundary_msgs", "final_quantum"]
NUM_RUN_INFO = 8
# gg_core_model_run statistics (include/graphite_gpu.h GG_CORE_*)
CORE_STATS = ["instructions", "time_ps", "memory_stall_ps", "execution_stall_ps", "l1d_read_stall_ps",
              "l1d_write_stall_ps", "sync_instructions", "sync_stall_ps"]
MISS_TYPES = ["cold", "capacity", "sharing"]   # GG_MT_* (Cache::MissType)
META_BARRIER = 0xFFFFFFFF     # GG_META_BARRIER: a BARRIER record of the trace
LVL_SYNC = 3                  # GG_LVL_SYNC: its access word (stall << 2) | 3
NUM_CORE_STATS = 8
# gg_iocoom_run (include/graphite_gpu.h gg_ins, GG_INS_*, GG_IOCOOM_*)
INS_DTYPE = np.dtype([("cost", "<u2"), ("ops", "u1"), ("regs", "u1"), ("reg", "<u2", (6,))])
INS_SIMPLE_MOV_LOAD, INS_ATOMIC, INS_FENCE_SHIFT, INS_SYNC = 0x10, 0x20, 6, 0x80
IOCOOM_NUM_REGISTERS = 512
IOCOOM_STATS = ["instructions", "time_ps", "memory_stall_ps", "execution_stall_ps", "sync_instructions",
                "sync_stall_ps", "load_queue_stall_ps", "store_queue_stall_ps", "l1i_stall_ps",
                "intra_l1d_stall_ps", "inter_l1d_stall_ps", "intra_exec_stall_ps", "inter_exec_stall_ps",
                "explicit_fences", "implicit_mfences", "data_accesses", "data_latency_ps"]
NUM_IOCOOM_STATS = 17


class IocoomParams(ctypes.Structure):
    """gg_iocoom_params; defaults = carbon_sim.cfg [core/iocoom]."""
    _fields_ = [("num_load_queue_entries", ctypes.c_uint32), ("num_store_queue_entries", ctypes.c_uint32),
                ("speculative_loads_enabled", ctypes.c_uint32),
                ("multiple_outstanding_RFOs_enabled", ctypes.c_uint32)]

    def __init__(self, lq=8, sq=8, spec=1, rfo=1):
        super().__init__(lq, sq, spec, rfo)


class AtacParams(ctypes.Structure):
    """gg_atac_params; defaults = carbon_sim.cfg [network/atac] (:318-352) and
    [link_model/optical] laser_modes (:366-370)."""
    _fields_ = [(n, ctypes.c_uint32) for n in (
        "cluster_size", "num_access_points", "receive_net_type", "num_receive_nets", "global_routing",
        "unicast_distance_threshold", "enet_router_delay", "send_hub_router_delay", "receive_hub_router_delay",
        "star_net_router_delay", "laser_modes")]

    def __init__(self, **kw):
        super().__init__(4, 4, ATAC_STAR, 2, ATAC_CLUSTER_BASED, 4, 1, 1, 1, 1, 3)
        for k, v in kw.items():
            if not hasattr(self, k):
                raise KeyError(k)
            setattr(self, k, v)


# synthetic memory traffic (gg_gen_memory_traffic): GG_MI_* instruction types, GG_MLS_* words of the reduction
MEM_INS_TYPES = ["non_memory", "rd_only_shared_read", "rd_wr_shared_read", "rd_wr_shared_write", "private_read",
                 "private_write"]
NUM_MEM_INS_TYPES = 6
MLS_FIELDS = ["records", "reads", "writes", "l1_hits", "l1_latency_ps", "l2_hits", "l2_latency_ps", "l2_misses",
              "l2_miss_latency_ps", "max_latency_ps"]
(MLS_RECORDS, MLS_READS, MLS_WRITES, MLS_L1_HITS, MLS_L1_LATENCY_PS, MLS_L2_HITS, MLS_L2_LATENCY_PS, MLS_L2_MISSES,
 MLS_L2_MISS_LATENCY_PS, MLS_MAX_LATENCY_PS) = range(10)
MLS_TYPE_COUNTS = 10     # + instruction type: totals over the tiles (mem_synthetic_run)
MLS_MAX_TILE_CLOCK_PS = 16
MLS_HIST = 18            # + bit length of the latency in ps, 65 bins
NUM_MLS = MLS_HIST + 65


class MemTrafficParams(ctypes.Structure):
    """gg_mem_traffic_params: the eleven numbers of a synthetic_memory input
    file, the seed of tile 0's streams and the srandom() seed of the address
    map.  Defaults = inputs/input.64."""
    _fields_ = [("num_threads", ctypes.c_uint32), ("degree_of_sharing", ctypes.c_uint32),
                ("num_shared_addresses", ctypes.c_uint32), ("num_private_addresses", ctypes.c_uint32),
                ("instructions_per_tile", ctypes.c_uint64), ("probability", ctypes.c_float * NUM_MEM_INS_TYPES),
                ("seed_base", ctypes.c_uint64), ("map_seed", ctypes.c_uint32), ("reserved", ctypes.c_uint32)]

    def __init__(self, num_threads=64, degree_of_sharing=1, num_shared_addresses=1024, num_private_addresses=256,
                 instructions_per_tile=10000, probability=(0.7, 0.025, 0.060, 0.015, 0.14, 0.06), seed_base=0,
                 map_seed=1):
        if len(probability) != NUM_MEM_INS_TYPES:
            raise ValueError("six probabilities expected")
        super().__init__(num_threads, degree_of_sharing, num_shared_addresses, num_private_addresses,
                         instructions_per_tile, (ctypes.c_float * NUM_MEM_INS_TYPES)(*probability), seed_base,
                         map_seed, 0)

    @classmethod
    def from_input_file(cls, path, ns=None):
        """The reference's input format: eleven whitespace-separated numbers
        (synthetic_memory.cc:235-260); ns overrides the degree of sharing as
        its -ns option does."""
        tok = open(path).read().split()
        if len(tok) < 11:
            raise ValueError("%s: eleven numbers expected, found %d" % (path, len(tok)))
        ints = [int(x) for x in tok[:5]]
        if ns is not None:
            ints[1] = int(ns)
        return cls(*ints, probability=tuple(float(x) for x in tok[5:11]))

    def replace(self, **kw):
        """A copy with some fields changed (probability: a sequence of six)."""
        d = dict(num_threads=self.num_threads, degree_of_sharing=self.degree_of_sharing,
                 num_shared_addresses=self.num_shared_addresses, num_private_addresses=self.num_private_addresses,
                 instructions_per_tile=self.instructions_per_tile, probability=tuple(self.probability),
                 seed_base=self.seed_base, map_seed=self.map_seed)
        for k in kw:
            if k not in d:
                raise KeyError(k)
        d.update(kw)
        return MemTrafficParams(**d)


CMSG_DTYPE = None  # filled below (numpy view of gg_cmsg)
NUM_NET_COUNTERS = len(NET_COUNTERS)


class GGConfig(ctypes.Structure):
    _fields_ = [
        ("num_tiles", ctypes.c_uint32),
        ("line_size", ctypes.c_uint32),
        ("l1d_size_kb", ctypes.c_uint32),
        ("l1d_assoc", ctypes.c_uint32),
        ("l1d_policy", ctypes.c_uint32),
        ("l2_size_kb", ctypes.c_uint32),
        ("l2_assoc", ctypes.c_uint32),
        ("l2_policy", ctypes.c_uint32),
        ("net_model", ctypes.c_uint32),
        ("flit_width", ctypes.c_uint32),
        ("router_delay", ctypes.c_uint32),
        ("link_delay", ctypes.c_uint32),
        ("queue_model_enabled", ctypes.c_uint32),
        ("max_list_size", ctypes.c_uint32),
        ("analytical_enabled", ctypes.c_uint32),
        ("total_tiles", ctypes.c_uint32),
        ("frequency_ghz", ctypes.c_double),
        ("device", ctypes.c_int32),
        ("replay_kernel", ctypes.c_uint32),
        ("l1d_data_cycles", ctypes.c_uint32),
        ("l1d_tags_cycles", ctypes.c_uint32),
        ("l2_data_cycles", ctypes.c_uint32),
        ("l2_tags_cycles", ctypes.c_uint32),
        ("dir_assoc", ctypes.c_uint32),
        ("dir_total_entries", ctypes.c_uint32),
        ("dir_access_cycles", ctypes.c_uint32),
        ("dram_latency_ns", ctypes.c_uint32),
        ("dram_bandwidth", ctypes.c_float),
        ("dram_queue_model_enabled", ctypes.c_uint32),
        ("quantum_ns", ctypes.c_uint32),
        ("num_shards", ctypes.c_uint32),
        ("shard_begin", ctypes.c_uint32),
        ("shard_end", ctypes.c_uint32),
        ("queue_model_type", ctypes.c_uint32),
        ("dram_queue_model_type", ctypes.c_uint32),
        ("basic_moving_avg", ctypes.c_uint32),
        ("history_list_no_interleaving", ctypes.c_uint32),
        ("l1i_track_miss_types", ctypes.c_uint32),
        ("l2_track_miss_types", ctypes.c_uint32),
        ("miss_track_lines", ctypes.c_uint32),
        ("protocol", ctypes.c_uint32),
        ("l1d_track_miss_types", ctypes.c_uint32),
    ]


def default_config(num_tiles, **overrides):
    """The carbon_sim.cfg defaults for ``num_tiles`` application tiles."""
    c = GGConfig()
    c.num_tiles = num_tiles
    c.line_size = 64
    c.l1d_size_kb, c.l1d_assoc, c.l1d_policy = 32, 4, POLICY_LRU
    c.l2_size_kb, c.l2_assoc, c.l2_policy = 512, 8, POLICY_LRU
    c.net_model = NET_EMESH_HOP_COUNTER
    c.flit_width = 64
    c.router_delay = 1
    c.link_delay = 1
    c.queue_model_enabled = 1
    c.max_list_size = 100
    c.analytical_enabled = 1
    c.total_tiles = 0
    c.frequency_ghz = 1.0
    c.device = 0
    c.replay_kernel = 0
    # coherent mode (carbon_sim.cfg:97, 219-273)
    c.l1d_data_cycles, c.l1d_tags_cycles = 1, 1
    c.l2_data_cycles, c.l2_tags_cycles = 8, 3
    c.dir_assoc, c.dir_total_entries, c.dir_access_cycles = 16, 0, 0
    c.dram_latency_ns, c.dram_bandwidth, c.dram_queue_model_enabled = 100, 5.0, 1
    c.quantum_ns = 1000
    c.num_shards = 1
    c.shard_begin, c.shard_end = 0, 0
    for k, v in overrides.items():
        if not hasattr(c, k):
            raise KeyError(k)
        setattr(c, k, v)
    return c


def tile_id_bits(num_tiles):
    """Config::computeTileIDLength = ceilLog2(application tiles) (config.cc:149-152)."""
    return int(math.ceil(math.log2(num_tiles))) if num_tiles > 1 else 0


def shmem_modeled_bits(num_tiles, with_data):
    """Modeled length of an MSI ShmemMsg packet in bits: 2 * tile-id bits
    (network_model.cc:185-200) + 4 msg-type + 48 address bits (+ 64 B of data)
    (pr_l1_pr_l2_dram_directory_msi/shmem_msg.cc:100-125, shmem_msg.h:81)."""
    return 2 * tile_id_bits(num_tiles) + 4 + 48 + (512 if with_data else 0)


def _cmsg_dtype():
    import numpy as np
    return np.dtype([("addr", "<u8"), ("send_ps", "<u8"), ("arrival_ps", "<u8"), ("zero_load_ps", "<u8"),
                     ("src", "<u4"), ("dst", "<u4"), ("requester", "<u4"), ("seq", "<u4"), ("type", "<u4"),
                     ("link", "<u4"), ("hop", "<u4"), ("single_rx", "<u4")])


CMSG_DTYPE = _cmsg_dtype()


HOP_NONE = 0xFFFFFFFF


def shard_map(num_tiles, num_shards):
    """Logical shard of every tile: on a full W x H mesh
    the 2-D block the reference gives process k of num_shards under
    emesh_hop_by_hop (NetworkModelEMeshHopByHop::computeProcessToTileMapping,
    network_model_emesh_hop_by_hop.cc:367-433); contiguous tile ranges
    otherwise.  Same rule as the ABI's gg_shard_map."""
    import numpy as np
    T, K = int(num_tiles), int(num_shards or 1)
    if K < 1 or K > T:
        raise ValueError("num_shards must be in [1, num_tiles]")
    W = int(math.floor(math.sqrt(T)))
    H = int(math.ceil(T / W))
    if W * H != T:
        return (np.arange(T, dtype=np.int64) * K // T).astype(np.uint32)
    out = np.full(T, 0xFFFFFFFF, np.uint32)
    pw = int(math.floor(math.sqrt(K)))
    ph = int(math.floor(K / pw))
    mhl = int((1.0 * H * pw * ph) / K)
    for i in range(pw):
        for j in range(ph):
            sx, sy = W // pw, mhl // ph
            bx, by = i * sx, j * sy
            if i == pw - 1:
                sx = W - (pw - 1) * sx
            if j == ph - 1:
                sy = mhl - (ph - 1) * sy
            for jj in range(sy):
                out[(by + jj) * W + bx:(by + jj) * W + bx + sx] = i + j * pw
    left = K - pw * ph
    for i in range(pw * ph, K):
        sx = W // left
        sy, bx, by = H - mhl, (i - pw * ph) * sx, mhl
        if i == K - 1:
            sx = W - (left - 1) * sx
        for jj in range(sy):
            out[(by + jj) * W + bx:(by + jj) * W + bx + sx] = i
    if (out >= K).any() or len(np.unique(out)) != K:
        raise ValueError("no shard map for %d tiles in %d shards" % (T, K))
    return out


def shard_of_tile(tile, num_tiles, num_shards):
    """Logical shard of a tile (shard_map)."""
    return int(shard_map(num_tiles, num_shards)[tile])


def _isqrt_exact(n):
    r = math.isqrt(n)
    return r if r * r == n else None


def atac_check(num_tiles, params):
    """The checks of NetworkModelAtac::initializeANetTopologyParams
    (network_model_atac.cc:104-121); raises ValueError naming the field."""
    T, cs, ap = int(num_tiles), int(params.cluster_size), int(params.num_access_points)
    p2 = lambda n: n > 0 and n & (n - 1) == 0
    if not p2(T) or _isqrt_exact(T) is None:
        raise ValueError("num_tiles %d must be a power of two and a perfect square" % T)
    if not p2(cs):
        raise ValueError("cluster_size %d must be a power of two" % cs)
    if not p2(ap):
        raise ValueError("num_access_points %d must be a power of two" % ap)
    if ap > cs:
        raise ValueError("num_access_points %d above cluster_size %d" % (ap, cs))
    if T % cs or T // cs < 2:
        raise ValueError("cluster_size %d leaves fewer than 2 clusters of %d tiles" % (cs, T))
    if params.num_receive_nets == 0:
        raise ValueError("num_receive_nets must be at least 1")
    if params.laser_modes == 0 or params.laser_modes > 3:
        raise ValueError("laser_modes must enable unicast (1), broadcast (2) or both")


def atac_topology(num_tiles, params):
    """(cluster_of[T], access_point_of[T], hub_of_cluster[C], star_index_of[T]) of
    the ATAC network (NetworkModelAtac::initializeClusters, getClusterID,
    getNearestAccessPoint, getTileIDWithOpticalHub, getTileIDListInCluster:
    network_model_atac.cc:587-745).  Same rule as the ABI's gg_atac_topology."""
    atac_check(num_tiles, params)
    T, cs, nap = int(num_tiles), int(params.cluster_size), int(params.num_access_points)
    W = math.isqrt(T)
    C = T // cs

    def grid(n, wide):
        # even log2: square; odd: X = sqrt(n/2), Y = sqrt(2n) for clusters (:594-603),
        # the other way round for sub-clusters (:621-630)
        if (n.bit_length() - 1) % 2 == 0:
            return math.isqrt(n), math.isqrt(n)
        a, b = math.isqrt(n // 2), math.isqrt(n * 2)
        return (b, a) if wide else (a, b)

    nx, ny = grid(C, False)
    cw, ch = W // nx, W // ny
    sx, sy = grid(nap, True)
    sw, sh = cw // sx, ch // sy
    if sw == 0 or sh == 0:
        raise ValueError("num_access_points %d does not tile a %d x %d cluster" % (nap, cw, ch))
    cmw = W // cw
    t = np.arange(T)
    x, y = t % W, t // W
    cluster = (y // ch) * cmw + x // cw
    minx, miny = (cluster % cmw) * cw, (cluster // cmw) * ch
    ap = (miny + ((y - miny) // sh) * sh + sh // 2) * W + minx + ((x - minx) // sw) * sw + sw // 2
    c = np.arange(C)
    hub = ((c // cmw) * ch + ch // 2) * W + (c % cmw) * cw + cw // 2
    star = (x - minx) * ch + (y - miny)
    return cluster.astype(np.uint32), ap.astype(np.uint32), hub.astype(np.uint32), star.astype(np.uint32)
