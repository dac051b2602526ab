"""Python binding of the C ABI (include/graphite_gpu.h) over ctypes.

This is host plumbing only: every computation runs in libgraphite_gpu.so's
HIP kernels.  There is no CPU fallback — if the library or a GPU is missing the
calls raise.  Device buffers are torch tensors on the ROCm device (PyTorch is
used for allocation and streams only).
"""
import ctypes
import os

import numpy as np

from .config import (GGConfig, NUM_CACHE_COUNTERS, NUM_NET_COUNTERS, NUM_TILE_STATS, NUM_RUN_INFO, NUM_CORE_STATS,
                     CMSG_DTYPE, AtacParams, NUM_ATAC_COUNTERS, MemTrafficParams, NUM_MEM_INS_TYPES, NUM_MLS)

CMSG_BYTES = CMSG_DTYPE.itemsize

HERE = os.path.dirname(os.path.abspath(__file__))
# GG_LIB (diagnostics only): load an alternative in-tree build for A/B kernel runs
LIB_PATH = os.environ.get("GG_LIB") or os.path.join(HERE, "libgraphite_gpu.so")

GG_OK = 0
_ERR = {-1: "GG_ERR_INVALID", -2: "GG_ERR_HIP", -3: "GG_ERR_UNSUPPORTED", -4: "GG_ERR_RANGE", -5: "GG_ERR_STATE"}


class GGError(RuntimeError):
    def __init__(self, code, msg, statuses=None):
        super().__init__("%s: %s" % (_ERR.get(code, code), msg))
        self.code = code
        self.statuses = statuses     # the *_many calls: the status of every instance


class LineInfo(ctypes.Structure):
    _fields_ = [("tag", ctypes.c_uint64), ("cstate", ctypes.c_uint32), ("cached_loc", ctypes.c_uint32)]


class _Trace(ctypes.Structure):
    _fields_ = [("addr_dev", ctypes.c_void_p), ("meta_dev", ctypes.c_void_p),
                ("tile_offsets", ctypes.POINTER(ctypes.c_uint64)), ("num_records", ctypes.c_uint64)]


class _Packets(ctypes.Structure):
    _fields_ = [("src_dev", ctypes.c_void_p), ("dst_dev", ctypes.c_void_p),
                ("length_bits_dev", ctypes.c_void_p), ("time_ps_dev", ctypes.c_void_p),
                ("num_packets", ctypes.c_uint64)]


class _PacketOut(ctypes.Structure):
    _fields_ = [("arrival_ps_dev", ctypes.c_void_p), ("zero_load_ps_dev", ctypes.c_void_p),
                ("contention_ps_dev", ctypes.c_void_p)]


# every symbol include/graphite_gpu.h declares (checked by tests/test_abi.py)
EXPORTS = ["gg_abi_version", "gg_last_error", "gg_config_default", "gg_create", "gg_destroy", "gg_reset",
           "gg_cache_access_batch", "gg_cache_get_counters", "gg_cache_get_line_info",
           "gg_cache_set_line_info", "gg_cache_access_line", "gg_cache_insert_line",
           "gg_noc_route_batch", "gg_noc_route_tree", "gg_noc_get_counters", "gg_queue_delay_batch",
           "gg_gen_uniform_trace", "gg_kernel_time_ms", "gg_set_timing",
           "gg_coherent_begin", "gg_coherent_quantum", "gg_coherent_export", "gg_coherent_import",
           "gg_coherent_run", "gg_coherent_get_stats", "gg_gen_hotspot_trace", "gg_shard_map",
           "gg_kernel_stats", "gg_round_exchange", "gg_coherent_run_ranks", "gg_gen_stress_trace",
           "gg_split_accesses", "gg_combine_accesses", "gg_dump_summary", "gg_core_model_run", "gg_core_get_stats", "gg_coherent_get_miss_types",
           "gg_coherent_get_protocol_stats", "gg_iocoom_run", "gg_iocoom_get_stats",
           "gg_round_pack", "gg_round_unpack", "gg_round_finish", "gg_coherent_run_many",
           "gg_stats_trace_configure", "gg_stats_trace_sample", "gg_stats_trace_get", "gg_stats_trace_dump",
           "gg_atac_params_default", "gg_noc_set_atac", "gg_atac_topology", "gg_noc_get_atac_counters",
           "gg_cache_track_miss_types", "gg_cache_get_miss_types",
           "gg_coherent_advance", "gg_coherent_snapshot_size", "gg_coherent_snapshot", "gg_coherent_restore",
           "gg_coherent_advance_many",
           "gg_coherent_begin_window", "gg_coherent_next_window", "gg_coherent_window_state",
           "gg_coherent_window_snapshot_size", "gg_coherent_window_snapshot", "gg_coherent_window_restore",
           "gg_window_snapshot_state",
           "gg_traffic_params_default", "gg_gen_network_traffic", "gg_noc_latency_stats", "gg_noc_synthetic_run",
           "gg_noc_route_batch_many", "gg_noc_synthetic_run_many",
           "gg_mem_traffic_params_default", "gg_gen_memory_traffic", "gg_mem_latency_stats", "gg_mem_synthetic_run",
           "gg_mem_synthetic_get", "gg_mem_synthetic_copy"]

# synthetic network traffic (gg_gen_network_traffic): GG_TP_* patterns, GG_NLS_* words of the reduction
TRAFFIC_PATTERNS = ["uniform_random", "bit_complement", "shuffle", "transpose", "tornado", "nearest_neighbor"]
(TP_UNIFORM_RANDOM, TP_BIT_COMPLEMENT, TP_SHUFFLE, TP_TRANSPOSE, TP_TORNADO, TP_NEAREST_NEIGHBOR) = range(6)
NETPACKET_BYTES = 64     # GG_NETPACKET_BYTES
NLS_FIELDS = ["packets", "self_packets", "latency_ps", "zero_load_ps", "contention_ps", "max_latency_ps",
              "last_arrival_ps"]
(NLS_PACKETS, NLS_SELF_PACKETS, NLS_LATENCY_PS, NLS_ZERO_LOAD_PS, NLS_CONTENTION_PS, NLS_MAX_LATENCY_PS,
 NLS_LAST_ARRIVAL_PS) = range(7)
NLS_HIST = 8             # + bit length of the latency in ps, 65 bins
NUM_NLS = NLS_HIST + 65


class TrafficParams(ctypes.Structure):
    """gg_traffic_params: the synthetic_network benchmark's -p / -s / -l / -N and a seed."""
    _fields_ = [("pattern", ctypes.c_uint32), ("packet_bytes", ctypes.c_uint32), ("offered_load", ctypes.c_double),
                ("packets_per_tile", ctypes.c_uint64), ("seed", ctypes.c_uint64)]

    def __init__(self, pattern=TP_UNIFORM_RANDOM, packet_bytes=8, offered_load=0.1, packets_per_tile=10000, seed=0):
        if isinstance(pattern, str):
            pattern = TRAFFIC_PATTERNS.index(pattern)
        super().__init__(pattern, packet_bytes, offered_load, packets_per_tile, seed)

# statistics trace (gg_stats_trace_*): GG_ST_* statistics bits, GG_STF_* sample fields
ST_NETWORK_UTILIZATION, ST_CACHE_LINE_REPLICATION = 1, 2
ST_FIELDS = ["time_ns", "repeat", "flits_sent", "flits_broadcasted", "flits_received",
             "l1_exclusive", "l1_shared", "l2_exclusive", "l2_shared"]

MANY_MAX = 4096          # GG_MANY_MAX


class RoundIO(ctypes.Structure):
    """gg_round_io: the device buffers of one rank's round (gg_round_pack)."""
    _fields_ = [("send", ctypes.c_void_p), ("recv", ctypes.c_void_p), ("words_own", ctypes.c_void_p),
                ("words_all", ctypes.c_void_p), ("stride", ctypes.c_uint64), ("slot", ctypes.c_uint64),
                ("send_count", ctypes.POINTER(ctypes.c_uint64)), ("recv_count", ctypes.POINTER(ctypes.c_uint64)),
                ("next_q", ctypes.c_uint64), ("done", ctypes.c_int32), ("state", ctypes.c_int32)]


ROUND_WORDS = 8
ROUND_DONE, ROUND_AGAIN, ROUND_OVERFLOW = 0, 1, 2
CMSG_RECORD_BYTES = 64


class _CStatus(ctypes.Structure):
    _fields_ = [("steps", ctypes.c_uint64), ("boundary_msgs", ctypes.c_uint64), ("min_next_ps", ctypes.c_uint64),
                ("active_tiles", ctypes.c_uint32), ("blocked_tiles", ctypes.c_uint32)]

_lib = None


def load():
    """Load libgraphite_gpu.so (raises if it has not been built)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RuntimeError("graphite_amd: %s is missing — run __graft_entry__.build() "
                           "(make -C graphite_amd/csrc); there is no CPU fallback" % LIB_PATH)
    L = ctypes.CDLL(LIB_PATH)
    vp, u32, u64, i32 = ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint64, ctypes.c_int
    L.gg_abi_version.restype = i32
    L.gg_last_error.restype = ctypes.c_char_p
    L.gg_config_default.argtypes = [ctypes.POINTER(GGConfig), u32]
    L.gg_create.restype = vp
    L.gg_create.argtypes = [ctypes.POINTER(GGConfig), ctypes.POINTER(i32)]
    L.gg_destroy.argtypes = [vp]
    L.gg_reset.argtypes = [vp]
    L.gg_cache_access_batch.argtypes = [vp, ctypes.POINTER(_Trace), vp, vp, vp]
    L.gg_cache_get_counters.argtypes = [vp, vp]
    L.gg_cache_get_line_info.argtypes = [vp, u32, i32, u64, ctypes.POINTER(LineInfo)]
    L.gg_cache_set_line_info.argtypes = [vp, u32, i32, u64, ctypes.POINTER(LineInfo)]
    L.gg_cache_access_line.argtypes = [vp, u32, i32, u64, i32]
    L.gg_cache_insert_line.argtypes = [vp, u32, i32, u64, ctypes.POINTER(LineInfo), ctypes.POINTER(i32),
                                       ctypes.POINTER(u64), ctypes.POINTER(LineInfo)]
    L.gg_noc_route_batch.argtypes = [vp, ctypes.POINTER(_Packets), ctypes.POINTER(_PacketOut), vp]
    L.gg_noc_route_tree.argtypes = [vp, ctypes.POINTER(_Packets), ctypes.POINTER(_PacketOut),
                                    ctypes.POINTER(_PacketOut), u64, vp]
    L.gg_noc_get_counters.argtypes = [vp, vp]
    L.gg_queue_delay_batch.argtypes = [vp, u64, vp, vp, u64, vp]
    L.gg_gen_uniform_trace.argtypes = [vp, vp, u32, u32, u64, u64, u32, u32, vp]
    L.gg_kernel_time_ms.restype = ctypes.c_float
    L.gg_kernel_time_ms.argtypes = [vp, ctypes.c_char_p]
    L.gg_set_timing.argtypes = [vp, i32]
    L.gg_coherent_begin.argtypes = [vp, ctypes.POINTER(_Trace), vp, vp]
    L.gg_coherent_quantum.argtypes = [vp, u64, ctypes.POINTER(_CStatus)]
    L.gg_coherent_export.argtypes = [vp, vp, u64, vp]
    L.gg_coherent_import.argtypes = [vp, vp, u64]
    L.gg_coherent_run.argtypes = [vp, ctypes.POINTER(_Trace), vp, vp]
    L.gg_coherent_get_stats.argtypes = [vp, vp, vp, vp]
    L.gg_gen_hotspot_trace.argtypes = [vp, vp, u32, u32, u64, u64, u32, u32, u32, u32, vp]
    L.gg_shard_map.argtypes = [u32, u32, vp]
    L.gg_kernel_stats.argtypes = [vp, ctypes.c_char_p, ctypes.POINTER(ctypes.c_double), ctypes.POINTER(u64)]
    L.gg_round_exchange.argtypes = [vp, vp, vp, u64, ctypes.POINTER(u64), ctypes.POINTER(i32)]
    L.gg_gen_stress_trace.argtypes = [vp, vp, u32, u32, u64, u64, u32, u32, u32, u32, u32, vp]
    L.gg_coherent_run_ranks.argtypes = [vp, vp, ctypes.POINTER(_Trace), vp, vp]
    L.gg_split_accesses.argtypes = [vp, vp, vp, vp, u32, u32, vp, vp, vp, u64, ctypes.POINTER(u64), vp, vp]
    L.gg_combine_accesses.argtypes = [vp, vp, u64, vp, vp, vp]
    L.gg_dump_summary.argtypes = [vp, i32, ctypes.c_char_p, u64, ctypes.POINTER(u64)]
    L.gg_core_model_run.argtypes = [vp, ctypes.POINTER(_Trace), vp, vp]
    L.gg_core_get_stats.argtypes = [vp, vp]
    L.gg_iocoom_run.argtypes = [vp, vp, vp, vp, vp, vp, vp, vp, vp]
    L.gg_iocoom_get_stats.argtypes = [vp, vp]
    L.gg_coherent_get_miss_types.argtypes = [vp, vp]
    L.gg_coherent_get_protocol_stats.argtypes = [vp, vp]
    L.gg_round_pack.argtypes = [vp, u32, u32, u64, ctypes.POINTER(RoundIO)]
    L.gg_round_unpack.argtypes = [vp, ctypes.POINTER(RoundIO)]
    L.gg_round_finish.argtypes = [vp, ctypes.POINTER(RoundIO)]
    L.gg_coherent_run_many.argtypes = [ctypes.POINTER(vp), u32, ctypes.POINTER(_Trace), ctypes.POINTER(vp),
                                       ctypes.POINTER(i32), vp]
    L.gg_stats_trace_configure.argtypes = [vp, u32, u64, u64]
    L.gg_stats_trace_sample.argtypes = [vp, u64]
    L.gg_stats_trace_get.argtypes = [vp, vp, vp, u64, ctypes.POINTER(u64)]
    L.gg_stats_trace_dump.argtypes = [vp, i32, ctypes.c_char_p, u64, ctypes.POINTER(u64)]
    for name in ["gg_stats_trace_configure", "gg_stats_trace_sample", "gg_stats_trace_get", "gg_stats_trace_dump"]:
        getattr(L, name).restype = i32
    L.gg_atac_params_default.argtypes = [ctypes.POINTER(AtacParams)]
    L.gg_atac_params_default.restype = None
    L.gg_noc_set_atac.argtypes = [vp, ctypes.POINTER(AtacParams)]
    L.gg_atac_topology.argtypes = [u32, ctypes.POINTER(AtacParams), vp, vp, vp, vp]
    L.gg_noc_get_atac_counters.argtypes = [vp, vp]
    for name in ["gg_noc_set_atac", "gg_atac_topology", "gg_noc_get_atac_counters"]:
        getattr(L, name).restype = i32
    L.gg_cache_track_miss_types.argtypes = [vp, u32]
    L.gg_cache_get_miss_types.argtypes = [vp, vp]
    for name in ["gg_cache_track_miss_types", "gg_cache_get_miss_types"]:
        getattr(L, name).restype = i32
    L.gg_coherent_advance.argtypes = [vp, u64, ctypes.POINTER(u64), ctypes.POINTER(i32)]
    L.gg_coherent_snapshot_size.argtypes = [vp, ctypes.POINTER(u64)]
    L.gg_coherent_snapshot.argtypes = [vp, vp, u64, ctypes.POINTER(u64)]
    L.gg_coherent_restore.argtypes = [vp, ctypes.POINTER(_Trace), vp, vp, u64, vp]
    L.gg_coherent_advance_many.argtypes = [ctypes.POINTER(vp), u32, ctypes.POINTER(u64), ctypes.POINTER(u64),
                                           ctypes.POINTER(i32), ctypes.POINTER(i32), vp]
    for name in ["gg_coherent_advance", "gg_coherent_snapshot_size", "gg_coherent_snapshot", "gg_coherent_restore",
                 "gg_coherent_advance_many"]:
        getattr(L, name).restype = i32
    L.gg_coherent_begin_window.argtypes = [vp, ctypes.POINTER(_Trace), vp, vp, vp]
    L.gg_coherent_next_window.argtypes = [vp, ctypes.POINTER(_Trace), vp, vp, vp]
    L.gg_coherent_window_state.argtypes = [vp, vp, vp]
    L.gg_coherent_window_snapshot_size.argtypes = [vp, ctypes.POINTER(u64)]
    L.gg_coherent_window_snapshot.argtypes = [vp, vp, u64, ctypes.POINTER(u64)]
    L.gg_coherent_window_restore.argtypes = [vp, ctypes.POINTER(_Trace), vp, vp, vp, u64, vp]
    L.gg_window_snapshot_state.argtypes = [vp, u64, u32, vp, vp]
    for name in ["gg_coherent_begin_window", "gg_coherent_next_window", "gg_coherent_window_state",
                 "gg_coherent_window_snapshot_size", "gg_coherent_window_snapshot", "gg_coherent_window_restore",
                 "gg_window_snapshot_state"]:
        getattr(L, name).restype = i32
    L.gg_traffic_params_default.argtypes = [ctypes.POINTER(TrafficParams)]
    L.gg_traffic_params_default.restype = None
    L.gg_gen_network_traffic.argtypes = [ctypes.POINTER(TrafficParams), u32, ctypes.c_double, vp, vp, vp, vp, vp, vp]
    L.gg_noc_latency_stats.argtypes = [ctypes.POINTER(_Packets), ctypes.POINTER(_PacketOut), vp, vp]
    L.gg_noc_synthetic_run.argtypes = [vp, ctypes.POINTER(TrafficParams), vp, vp]
    L.gg_noc_route_batch_many.argtypes = [ctypes.POINTER(vp), u32, ctypes.POINTER(_Packets), ctypes.POINTER(_PacketOut),
                                          ctypes.POINTER(i32), vp]
    L.gg_noc_synthetic_run_many.argtypes = [ctypes.POINTER(vp), u32, ctypes.POINTER(TrafficParams), vp,
                                            ctypes.POINTER(i32), vp]
    for name in ["gg_gen_network_traffic", "gg_noc_latency_stats", "gg_noc_synthetic_run", "gg_noc_route_batch_many",
                 "gg_noc_synthetic_run_many"]:
        getattr(L, name).restype = i32
    L.gg_mem_traffic_params_default.argtypes = [ctypes.POINTER(MemTrafficParams)]
    L.gg_mem_traffic_params_default.restype = None
    L.gg_gen_memory_traffic.argtypes = [ctypes.POINTER(MemTrafficParams), u32, u32, vp, ctypes.POINTER(u64), vp, vp, u64,
                                        vp, vp, vp]
    L.gg_mem_latency_stats.argtypes = [ctypes.POINTER(_Trace), vp, vp, vp]
    L.gg_mem_synthetic_run.argtypes = [vp, ctypes.POINTER(MemTrafficParams), vp, vp]
    L.gg_mem_synthetic_get.argtypes = [vp, ctypes.POINTER(_Trace), ctypes.POINTER(vp), ctypes.POINTER(vp),
                                       ctypes.POINTER(vp)]
    L.gg_mem_synthetic_copy.argtypes = [vp, vp, vp, vp, vp, vp, vp]
    for name in ["gg_gen_memory_traffic", "gg_mem_latency_stats", "gg_mem_synthetic_run", "gg_mem_synthetic_get",
                 "gg_mem_synthetic_copy"]:
        getattr(L, name).restype = i32
    for name in ["gg_kernel_stats", "gg_shard_map", "gg_coherent_begin", "gg_coherent_quantum", "gg_coherent_export",
                 "gg_coherent_import", "gg_coherent_run", "gg_coherent_get_stats", "gg_gen_hotspot_trace",
                 "gg_round_exchange", "gg_coherent_run_ranks", "gg_gen_stress_trace", "gg_split_accesses",
                 "gg_combine_accesses", "gg_dump_summary", "gg_core_model_run", "gg_core_get_stats",
                 "gg_coherent_get_miss_types", "gg_coherent_get_protocol_stats", "gg_iocoom_run",
                 "gg_iocoom_get_stats", "gg_round_pack", "gg_round_unpack", "gg_round_finish",
                 "gg_coherent_run_many"]:
        getattr(L, name).restype = i32
    for name in ["gg_reset", "gg_cache_access_batch", "gg_cache_get_counters", "gg_cache_get_line_info",
                 "gg_cache_set_line_info", "gg_cache_access_line", "gg_cache_insert_line",
                 "gg_noc_route_batch", "gg_noc_route_tree", "gg_noc_get_counters", "gg_queue_delay_batch",
                 "gg_gen_uniform_trace"]:
        getattr(L, name).restype = i32
    _lib = L
    return L


def _check(rc):
    if rc != GG_OK:
        raise GGError(rc, load().gg_last_error().decode(errors="replace"))


def _ptr(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def _stream(stream):
    import torch
    s = stream if stream is not None else torch.cuda.current_stream()
    return ctypes.c_void_p(s.cuda_stream)


def _need_dev(t, dtype, n=None):
    import torch
    if not t.is_cuda:
        raise ValueError("expected a device tensor")
    if t.dtype != dtype or not t.is_contiguous():
        raise ValueError("expected a contiguous %s device tensor" % dtype)
    if n is not None and t.numel() != n:
        raise ValueError("expected %d elements, got %d" % (n, t.numel()))


class Backend:
    """One context per GPU (gg_create): device-resident private caches of
    every tile and the NoC router state."""

    def __init__(self, cfg: GGConfig):
        L = load()
        st = ctypes.c_int(0)
        self.cfg = cfg
        self.h = L.gg_create(ctypes.byref(cfg), ctypes.byref(st))
        if not self.h:
            _check(st.value or -1)

    def close(self):
        if getattr(self, "h", None) and _lib is not None:
            _lib.gg_destroy(self.h)
            self.h = None

    __del__ = close

    def reset(self):
        _check(load().gg_reset(self.h))

    def set_timing(self, on=True, every_launch=False):
        """Kernel timing: off, sampled HIP events (coherent launches: 1 in 16),
        or every_launch=True: every coherent step / walk launch stamps its
        span (first workgroup start, last workgroup end) in-kernel."""
        load().gg_set_timing(self.h, (2 if every_launch else 1) if on else 0)

    def kernel_time_ms(self, name):
        return load().gg_kernel_time_ms(self.h, name.encode())

    def kernel_stats(self, name):
        """(total device ms, launches) of a coherent-mode kernel since the last
        coherent begin (timing must be on): mean over the timed launches (every
        16th, or every one) x launches."""
        ms, n = ctypes.c_double(0), ctypes.c_uint64(0)
        _check(load().gg_kernel_stats(self.h, name.encode(), ctypes.byref(ms), ctypes.byref(n)))
        return ms.value, n.value

    # ---- cache ----------------------------------------------------------
    def cache_access_batch(self, addr, meta, tile_offsets, result=None, evicted=None, stream=None):
        """Replay a tile-major trace batch (device tensors addr: uint64 as
        int64, meta: int32).  tile_offsets: host sequence of num_tiles+1."""
        import torch
        n = addr.numel()
        _need_dev(addr, torch.int64, n)
        _need_dev(meta, torch.int32, n)
        if result is not None:
            _need_dev(result, torch.int32, n)
        if evicted is not None:
            _need_dev(evicted, torch.int64, n)
        offs = np.ascontiguousarray(tile_offsets, dtype=np.uint64)
        if offs.size != self.cfg.num_tiles + 1:
            raise ValueError("tile_offsets needs num_tiles + 1 entries")
        tr = _Trace(addr.data_ptr(), meta.data_ptr(), offs.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64)), n)
        self._keep = offs
        _check(load().gg_cache_access_batch(self.h, ctypes.byref(tr), _ptr(result), _ptr(evicted), _stream(stream)))

    def cache_counters(self):
        out = np.zeros(self.cfg.num_tiles * 2 * NUM_CACHE_COUNTERS, np.uint64)
        _check(load().gg_cache_get_counters(self.h, out.ctypes.data_as(ctypes.c_void_p)))
        return out.reshape(self.cfg.num_tiles, 2, NUM_CACHE_COUNTERS)

    def cache_track_miss_types(self, lines=0):
        """gg_cache_track_miss_types: opt the context into miss-type tracking
        for the private replay and the quartet (fresh cache state only).
        lines: address-set capacity per (tile, cache); 0 = cfg.miss_track_lines
        or 65536."""
        _check(load().gg_cache_track_miss_types(self.h, lines))

    def cache_miss_types(self):
        """gg_cache_get_miss_types: [tile][L1-D, L2][cold, capacity, sharing]."""
        out = np.zeros(self.cfg.num_tiles * 2 * 3, np.uint64)
        _check(load().gg_cache_get_miss_types(self.h, out.ctypes.data_as(ctypes.c_void_p)))
        return out.reshape(self.cfg.num_tiles, 2, 3)

    def get_line_info(self, tile, level, addr, default=None):
        li = default or LineInfo(0xFFFFFFFFFFFFFFFF, 0, 0)
        _check(load().gg_cache_get_line_info(self.h, tile, level, addr, ctypes.byref(li)))
        return li

    def set_line_info(self, tile, level, addr, li):
        return load().gg_cache_set_line_info(self.h, tile, level, addr, ctypes.byref(li))

    def access_line(self, tile, level, addr, is_store):
        return load().gg_cache_access_line(self.h, tile, level, addr, int(is_store))

    def insert_line(self, tile, level, addr, li):
        ev = ctypes.c_int(0)
        ea = ctypes.c_uint64(0)
        evi = LineInfo(0xFFFFFFFFFFFFFFFF, 0, 0)
        rc = load().gg_cache_insert_line(self.h, tile, level, addr, ctypes.byref(li), ctypes.byref(ev),
                                         ctypes.byref(ea), ctypes.byref(evi))
        return rc, ev.value, ea.value, evi

    # ---- NoC ------------------------------------------------------------
    def noc_route_batch(self, src, dst, length_bits, time_ps, arrival, zero_load, contention, stream=None):
        import torch
        n = src.numel()
        for t, dt in ((src, torch.int32), (dst, torch.int32), (length_bits, torch.int32), (time_ps, torch.int64),
                      (arrival, torch.int64), (zero_load, torch.int64), (contention, torch.int64)):
            _need_dev(t, dt, n)
        pk = _Packets(src.data_ptr(), dst.data_ptr(), length_bits.data_ptr(), time_ps.data_ptr(), n)
        out = _PacketOut(arrival.data_ptr(), zero_load.data_ptr(), contention.data_ptr())
        _check(load().gg_noc_route_batch(self.h, ctypes.byref(pk), ctypes.byref(out), _stream(stream)))

    def noc_route_tree(self, src, dst, length_bits, time_ps, arrival, zero_load, contention,
                       b_arrival, b_zero_load, b_contention, num_broadcasts, stream=None):
        """gg_noc_route_tree: dst == config.BROADCAST takes the hop-by-hop broadcast
        tree; b_* hold num_broadcasts x num_tiles deliveries (batch order)."""
        import torch
        n = src.numel()
        for t, dt in ((src, torch.int32), (dst, torch.int32), (length_bits, torch.int32), (time_ps, torch.int64),
                      (arrival, torch.int64), (zero_load, torch.int64), (contention, torch.int64)):
            _need_dev(t, dt, n)
        nbt = num_broadcasts * self.cfg.num_tiles
        for t in (b_arrival, b_zero_load, b_contention):
            _need_dev(t, torch.int64, nbt)
        pk = _Packets(src.data_ptr(), dst.data_ptr(), length_bits.data_ptr(), time_ps.data_ptr(), n)
        out = _PacketOut(arrival.data_ptr(), zero_load.data_ptr(), contention.data_ptr())
        bout = _PacketOut(b_arrival.data_ptr(), b_zero_load.data_ptr(), b_contention.data_ptr())
        _check(load().gg_noc_route_tree(self.h, ctypes.byref(pk), ctypes.byref(out), ctypes.byref(bout),
                                        num_broadcasts, _stream(stream)))

    def noc_counters(self):
        out = np.zeros(self.cfg.num_tiles * NUM_NET_COUNTERS, np.uint64)
        _check(load().gg_noc_get_counters(self.h, out.ctypes.data_as(ctypes.c_void_p)))
        return out.reshape(self.cfg.num_tiles, NUM_NET_COUNTERS)

    def noc_synthetic_run(self, params, stream=None):
        """gg_noc_synthetic_run: generate params' traffic for this context's
        tiles, route it (continuing from the queue state) and reduce it;
        returns the NUM_NLS words (NLS_*)."""
        stats = np.zeros(NUM_NLS, np.uint64)
        _check(load().gg_noc_synthetic_run(self.h, ctypes.byref(params), stats.ctypes.data_as(ctypes.c_void_p),
                                           _stream(stream)))
        return stats

    def mem_synthetic_run(self, params, stream=None):
        """gg_mem_synthetic_run: generate params' (config.MemTrafficParams)
        instruction stream for this context's tiles and line size, run it with
        gg_coherent_run and reduce its access words; returns the NUM_MLS words
        (config.MLS_*), the type totals and the max tile clock among them."""
        stats = np.zeros(NUM_MLS, np.uint64)
        _check(load().gg_mem_synthetic_run(self.h, ctypes.byref(params), stats.ctypes.data_as(ctypes.c_void_p),
                                           _stream(stream)))
        return stats

    def mem_synthetic_trace(self, stream=None):
        """The last mem_synthetic_run's trace and results in fresh device
        tensors (gg_mem_synthetic_get for the sizes and tile offsets,
        gg_mem_synthetic_copy for the arrays): (addr, meta, tile_offsets
        [host], access words, tails [tiles], type counts [tiles][6]) — addr,
        meta and tile_offsets go to any coherent driver as they are."""
        import torch
        tr = _Trace()
        _check(load().gg_mem_synthetic_get(self.h, ctypes.byref(tr), None, None, None))
        T, n = self.cfg.num_tiles, int(tr.num_records)
        offs = np.array([tr.tile_offsets[i] for i in range(T + 1)], np.uint64)
        addr, out = (torch.zeros(n, dtype=torch.int64, device="cuda") for _ in range(2))
        meta = torch.zeros(n, dtype=torch.int32, device="cuda")
        tail = torch.zeros(T, dtype=torch.int64, device="cuda")
        types = torch.zeros((T, NUM_MEM_INS_TYPES), dtype=torch.int64, device="cuda")
        _check(load().gg_mem_synthetic_copy(self.h, _ptr(addr), _ptr(meta), _ptr(out), _ptr(tail), _ptr(types),
                                            _stream(stream)))
        return addr, meta, offs, out, tail, types

    def noc_set_atac(self, params):
        """gg_noc_set_atac: the ATAC settings (config.AtacParams) of a NET_ATAC
        context; reallocates the ATAC queues and resets the NoC state."""
        _check(load().gg_noc_set_atac(self.h, ctypes.byref(params)))

    def noc_atac_counters(self):
        """gg_noc_get_atac_counters: [tile][NUM_ATAC_COUNTERS] (config.ATAC_COUNTERS)."""
        out = np.zeros(self.cfg.num_tiles * NUM_ATAC_COUNTERS, np.uint64)
        _check(load().gg_noc_get_atac_counters(self.h, out.ctypes.data_as(ctypes.c_void_p)))
        return out.reshape(self.cfg.num_tiles, NUM_ATAC_COUNTERS)

    # ---- coherent mode (Mode C) ----------------------------------------
    def _trace(self, addr, meta, tile_offsets):
        import torch
        n = addr.numel()
        _need_dev(addr, torch.int64, n)
        _need_dev(meta, torch.int32, n)
        offs = np.ascontiguousarray(tile_offsets, dtype=np.uint64)
        if offs.size != self.cfg.num_tiles + 1:
            raise ValueError("tile_offsets needs num_tiles + 1 entries")
        self._keep = offs
        return _Trace(addr.data_ptr(), meta.data_ptr(), offs.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64)), n)

    def coherent_run(self, addr, meta, tile_offsets, out=None, stream=None):
        """Whole coherent run (the context must own every shard).  out: int64
        device tensor, one word per record ((latency_ps << 2) | level)."""
        import torch
        if out is not None:
            _need_dev(out, torch.int64, addr.numel())
        tr = self._trace(addr, meta, tile_offsets)
        _check(load().gg_coherent_run(self.h, ctypes.byref(tr), _ptr(out), _stream(stream)))

    def coherent_run_ranks(self, comm_ptr, addr, meta, tile_offsets, out=None, stream=None):
        """The whole coherent run over the ranks of an RCCL communicator
        (gg_coherent_run_ranks; comm_ptr = ncclComm_t as an int, e.g.
        ProcessGroupNCCL._comm_ptr()).  This context owns the rank's shards.
        The trace may hold BARRIER records: the round releases them as
        coherent_run does, bit-identical for any split over ranks."""
        import torch
        if out is not None:
            _need_dev(out, torch.int64, addr.numel())
        tr = self._trace(addr, meta, tile_offsets)
        _check(load().gg_coherent_run_ranks(self.h, ctypes.c_void_p(comm_ptr), ctypes.byref(tr), _ptr(out),
                                            _stream(stream)))

    def coherent_begin(self, addr, meta, tile_offsets, out=None, stream=None):
        import torch
        if out is not None:
            _need_dev(out, torch.int64, addr.numel())
        tr = self._trace(addr, meta, tile_offsets)
        _check(load().gg_coherent_begin(self.h, ctypes.byref(tr), _ptr(out), _stream(stream)))

    # ---- a run in legs: pause, snapshot, restore (gg_coherent_advance / _snapshot / _restore)
    NEVER = 0xFFFFFFFFFFFFFFFF          # stop_quantum that never pauses

    def coherent_advance(self, stop_quantum=NEVER):
        """The device-driven loop from the current state (after coherent_begin
        or coherent_restore) until the run is over or the next quantum is >=
        stop_quantum.  Returns (next_quantum, done): done 0 paused, 1 over
        (a deadlock raises, as coherent_run does), NEED_WINDOW on a windowed
        run whose next quantum needs the next windows (coherent_next_window)."""
        nq, done = ctypes.c_uint64(0), ctypes.c_int(0)
        _check(load().gg_coherent_advance(self.h, stop_quantum, ctypes.byref(nq), ctypes.byref(done)))
        return nq.value, done.value

    def coherent_snapshot_size(self):
        n = ctypes.c_uint64(0)
        _check(load().gg_coherent_snapshot_size(self.h, ctypes.byref(n)))
        return n.value

    def coherent_snapshot(self, cap=None):
        """The run's state at the device loop's clean point as a numpy uint8
        array (the container of gg_snapshot.h).  cap: the buffer's size
        (default: what gg_coherent_snapshot_size asks for)."""
        n = ctypes.c_uint64(self.coherent_snapshot_size() if cap is None else cap)
        buf = np.empty(max(n.value, 1), np.uint8)
        got = ctypes.c_uint64(0)
        rc = load().gg_coherent_snapshot(self.h, buf.ctypes.data_as(ctypes.c_void_p), n.value, ctypes.byref(got))
        if rc != GG_OK:
            e = GGError(rc, load().gg_last_error().decode(errors="replace"))
            e.needed = got.value         # GG_ERR_RANGE: the bytes a snapshot needs
            raise e
        return buf[:got.value]

    def coherent_restore(self, blob, addr, meta, tile_offsets, out=None, stream=None):
        """Reset as coherent_begin does, then put a snapshot's state back; the
        run continues with coherent_advance.  out: the access-word buffer
        (words of records already passed are not rewritten: carry the buffer
        across for the whole array)."""
        import torch
        if out is not None:
            _need_dev(out, torch.int64, addr.numel())
        b = np.ascontiguousarray(np.frombuffer(blob, np.uint8) if isinstance(blob, (bytes, bytearray)) else blob, np.uint8)
        tr = self._trace(addr, meta, tile_offsets)
        _check(load().gg_coherent_restore(self.h, ctypes.byref(tr), _ptr(out), b.ctypes.data_as(ctypes.c_void_p),
                                          b.size, _stream(stream)))

    # ---- a run fed its trace in windows (gg_coherent_begin_window / _next_window / _window_state)
    NEED_WINDOW = 3                     # GG_ADV_NEED_WINDOW: coherent_advance's done on a windowed run

    def _window(self, fn, addr, meta, tile_offsets, out, final_tiles, stream):
        import torch
        if out is not None:
            _need_dev(out, torch.int64, addr.numel())
        fin = None
        if final_tiles is not None:
            fin = np.ascontiguousarray(final_tiles, dtype=np.uint8)
            if fin.size != self.cfg.num_tiles:
                raise ValueError("final_tiles needs num_tiles entries")
        tr = self._trace(addr, meta, tile_offsets)
        _check(fn(self.h, ctypes.byref(tr), _ptr(out), None if fin is None else fin.ctypes.data_as(ctypes.c_void_p),
                  _stream(stream)))

    def coherent_begin_window(self, addr, meta, tile_offsets, out=None, final_tiles=None, stream=None):
        """coherent_begin with a first window of every tile's records
        (tile_offsets index the window's own arrays).  final_tiles[t] != 0:
        tile t's window runs to the end of its trace.  The run is driven by
        coherent_advance, which returns done == NEED_WINDOW when the next
        windows are due."""
        self._window(load().gg_coherent_begin_window, addr, meta, tile_offsets, out, final_tiles, stream)

    def coherent_next_window(self, addr, meta, tile_offsets, out=None, final_tiles=None, stream=None):
        """The next windows of a paused (or not yet advanced) windowed run:
        tile t's records begin at its first unconsumed record
        (coherent_window_state's consumed[t]).  After the call the previous
        arrays are the caller's again."""
        self._window(load().gg_coherent_next_window, addr, meta, tile_offsets, out, final_tiles, stream)

    def coherent_window_state(self):
        """(consumed, min_records), uint64 [num_tiles] each: the records every
        tile has consumed since begin, and what its next window must hold (up
        to its last record that is no CONT line and no BARRIER) for the next
        quantum to run; 0 for final and finished tiles."""
        T = self.cfg.num_tiles
        c, m = np.zeros(T, np.uint64), np.zeros(T, np.uint64)
        _check(load().gg_coherent_window_state(self.h, c.ctypes.data_as(ctypes.c_void_p), m.ctypes.data_as(ctypes.c_void_p)))
        return c, m

    # ---- a windowed run in legs (gg_coherent_window_snapshot / _window_restore)
    def coherent_window_snapshot_size(self):
        n = ctypes.c_uint64(0)
        _check(load().gg_coherent_window_snapshot_size(self.h, ctypes.byref(n)))
        return n.value

    def coherent_window_snapshot(self, cap=None):
        """coherent_snapshot for a run fed in windows, at its clean point (after
        coherent_begin_window, a returned coherent_advance, coherent_next_window
        or coherent_window_restore): the same container plus a `win` section.
        The bytes do not depend on where the windows were cut."""
        n = ctypes.c_uint64(self.coherent_window_snapshot_size() if cap is None else cap)
        buf = np.empty(max(n.value, 1), np.uint8)
        got = ctypes.c_uint64(0)
        rc = load().gg_coherent_window_snapshot(self.h, buf.ctypes.data_as(ctypes.c_void_p), n.value, ctypes.byref(got))
        if rc != GG_OK:
            e = GGError(rc, load().gg_last_error().decode(errors="replace"))
            e.needed = got.value         # GG_ERR_RANGE: the bytes a snapshot needs
            raise e
        return buf[:got.value]

    def coherent_window_restore(self, addr, meta, tile_offsets, out=None, final_tiles=None, blob=None, stream=None):
        """Reset as coherent_begin does, put a windowed snapshot's state back and
        install the windows as coherent_next_window would: tile t's records
        begin at record consumed[t] of its trace (window_snapshot_state(blob)).
        The run continues with coherent_advance and coherent_next_window."""
        if blob is None:
            raise ValueError("coherent_window_restore needs the snapshot (blob=...)")
        b = np.ascontiguousarray(np.frombuffer(blob, np.uint8) if isinstance(blob, (bytes, bytearray)) else blob, np.uint8)
        fn = lambda h, tr, out_p, fin_p, st: load().gg_coherent_window_restore(
            h, tr, out_p, fin_p, b.ctypes.data_as(ctypes.c_void_p), b.size, st)
        self._window(fn, addr, meta, tile_offsets, out, final_tiles, stream)

    def round_pack(self, world, rank, q):
        """gg_round_pack: quantum q's steps + the tail on the context's stream;
        returns the RoundIO with the device slots / words to move.  The
        ROUND_WORDS status words are opaque to the transport (they carry the
        rank's barrier waiters too: round_unpack's commit releases a barrier
        every unfinished tile of every rank has reached)."""
        io = RoundIO()
        _check(load().gg_round_pack(self.h, world, rank, q, ctypes.byref(io)))
        return io

    def round_unpack(self, io):
        _check(load().gg_round_unpack(self.h, ctypes.byref(io)))
        return io

    def round_finish(self, io):
        _check(load().gg_round_finish(self.h, ctypes.byref(io)))
        return io

    def coherent_quantum(self, q):
        st = _CStatus()
        _check(load().gg_coherent_quantum(self.h, q, ctypes.byref(st)))
        return {"steps": st.steps, "boundary_msgs": st.boundary_msgs, "min_next_ps": st.min_next_ps,
                "active_tiles": st.active_tiles, "blocked_tiles": st.blocked_tiles}

    def coherent_export(self, out_buf, cap):
        """Held cross-shard records -> out_buf (uint8 device tensor of cap*CMSG_BYTES
        bytes), grouped by destination shard; returns per-shard counts."""
        K = self.cfg.num_shards or 1
        counts = np.zeros(K, np.uint64)
        _check(load().gg_coherent_export(self.h, _ptr(out_buf), cap, counts.ctypes.data_as(ctypes.c_void_p)))
        return counts

    def coherent_import(self, buf, n):
        _check(load().gg_coherent_import(self.h, _ptr(buf), n))

    def coherent_stats(self):
        T = self.cfg.num_tiles
        st = np.zeros(T * NUM_TILE_STATS, np.uint64)
        cc = np.zeros(T * 2 * NUM_CACHE_COUNTERS, np.uint64)
        ri = np.zeros(NUM_RUN_INFO, np.uint64)
        _check(load().gg_coherent_get_stats(self.h, st.ctypes.data_as(ctypes.c_void_p),
                                            cc.ctypes.data_as(ctypes.c_void_p), ri.ctypes.data_as(ctypes.c_void_p)))
        return st.reshape(T, NUM_TILE_STATS), cc.reshape(T, 2, NUM_CACHE_COUNTERS), ri

    def core_model_run(self, meta, tile_offsets, access_out, stream=None):
        """The simple core model over a coherent run's access words
        (gg_core_model_run): meta (int32/uint32 device tensor of the trace's
        meta words), host tile offsets, access_out (int64 device tensor)."""
        import torch
        self._offs = np.ascontiguousarray(tile_offsets, np.uint64)
        if self._offs.size != self.cfg.num_tiles + 1:
            raise ValueError("tile_offsets needs num_tiles + 1 entries")
        n = int(self._offs[-1])
        _need_dev(meta, torch.int32, n)
        _need_dev(access_out, torch.int64, n)
        tr = _Trace(None, meta.data_ptr(), self._offs.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64)), n)
        _check(load().gg_core_model_run(self.h, ctypes.byref(tr), access_out.data_ptr(), _stream(stream)))

    def iocoom_run(self, params, ins, ins_offsets, addr, meta, lat, acc_offsets, stream=None):
        """The iocoom core model (gg_iocoom_run): params (config.IocoomParams),
        ins (device tensor holding the gg_ins records, 16 B each), host
        instruction tile offsets, the access stream's addr (int64), meta
        (int32) and latency (int64, ps) device tensors, host access tile
        offsets."""
        import torch
        T = self.cfg.num_tiles
        io = np.ascontiguousarray(ins_offsets, np.uint64)
        ao = np.ascontiguousarray(acc_offsets, np.uint64)
        if io.size != T + 1 or ao.size != T + 1:
            raise ValueError("tile offsets need num_tiles + 1 entries")
        if not ins.is_cuda or not ins.is_contiguous() or ins.numel() * ins.element_size() < 16 * int(io[-1]):
            raise ValueError("ins: a contiguous device tensor of %d gg_ins records" % int(io[-1]))
        n = int(ao[-1])
        _need_dev(addr, torch.int64, n)
        _need_dev(meta, torch.int32, n)
        _need_dev(lat, torch.int64, n)
        self._io_offs = (io, ao)
        self._io_params = params
        _check(load().gg_iocoom_run(self.h, ctypes.byref(params), ins.data_ptr(), io.ctypes.data, addr.data_ptr(),
                                    meta.data_ptr(), lat.data_ptr(), ao.ctypes.data, _stream(stream)))

    def iocoom_stats(self):
        """[tiles][NUM_IOCOOM_STATS] (gg_iocoom_get_stats)."""
        from graphite_amd.config import NUM_IOCOOM_STATS
        T = self.cfg.num_tiles
        out = np.zeros(T * NUM_IOCOOM_STATS, np.uint64)
        _check(load().gg_iocoom_get_stats(self.h, out.ctypes.data_as(ctypes.c_void_p)))
        return out.reshape(T, NUM_IOCOOM_STATS)

    def miss_types(self):
        """[tiles][2][3] cold / capacity / sharing misses of the L1-D and L2
        (gg_coherent_get_miss_types; zeros for an untracked cache)."""
        T = self.cfg.num_tiles
        out = np.zeros(T * 2 * 3, np.uint64)
        _check(load().gg_coherent_get_miss_types(self.h, out.ctypes.data_as(ctypes.c_void_p)))
        return out.reshape(T, 2, 3)

    def protocol_stats(self):
        """[tiles][NUM_PROTO_STATS] MOSI event counters (gg_coherent_get_protocol_stats; zeros under MSI)."""
        T = self.cfg.num_tiles
        out = np.zeros(T * 32, np.uint64)
        _check(load().gg_coherent_get_protocol_stats(self.h, out.ctypes.data_as(ctypes.c_void_p)))
        return out.reshape(T, 32)

    def core_stats(self):
        T = self.cfg.num_tiles
        out = np.zeros(T * NUM_CORE_STATS, np.uint64)
        _check(load().gg_core_get_stats(self.h, out.ctypes.data_as(ctypes.c_void_p)))
        return out.reshape(T, NUM_CORE_STATS)

    def dump_summary(self, table=False):
        """The sim.out text of the context's statistics (gg_dump_summary): one
        "Tile t Summary:" block per tile, or TileManager's table."""
        L = load()
        need = ctypes.c_uint64(0)
        fmt = 1 if table else 0
        _check(L.gg_dump_summary(self.h, fmt, None, 0, ctypes.byref(need)))
        buf = ctypes.create_string_buffer(need.value)
        _check(L.gg_dump_summary(self.h, fmt, buf, need.value, ctypes.byref(need)))
        return buf.value.decode()

    # ---- statistics trace ([statistics_trace]: gg_stats_trace_*) ----------
    def stats_trace_configure(self, statistics, sampling_interval_ns=0, max_samples=0):
        """The trace of the coherent runs begun from now on: statistics = a bit
        set of ST_NETWORK_UTILIZATION / ST_CACHE_LINE_REPLICATION (0: off), the
        sampling interval (a multiple of cfg.quantum_ns) and the sample
        buffer's size (a full buffer fails the run)."""
        _check(load().gg_stats_trace_configure(self.h, statistics, sampling_interval_ns, max_samples))

    def stats_trace_sample(self, barrier_time_ns):
        """Append one sample of the context's current state (between
        host-driven quanta, or after a finished run)."""
        _check(load().gg_stats_trace_sample(self.h, barrier_time_ns))

    def stats_trace(self):
        """The samples so far: {field: uint64 [n]} for ST_FIELDS, and
        "sharer_hist": uint64 [n][num_tiles + 1] (bin k = directory entries
        with k sharers)."""
        L = load()
        n = ctypes.c_uint64(0)
        _check(L.gg_stats_trace_get(self.h, None, None, 0, ctypes.byref(n)))
        m, T = n.value, self.cfg.num_tiles
        f = np.zeros((m, len(ST_FIELDS)), np.uint64)
        h = np.zeros((m, T + 1), np.uint64)
        if m:
            _check(L.gg_stats_trace_get(self.h, f.ctypes.data_as(ctypes.c_void_p), h.ctypes.data_as(ctypes.c_void_p),
                                        m, ctypes.byref(n)))
        out = {name: f[:, i].copy() for i, name in enumerate(ST_FIELDS)}
        out["sharer_hist"] = h
        return out

    def stats_trace_text(self, which):
        """The text of network_utilization_memory.dat (ST_NETWORK_UTILIZATION)
        or cache_line_replication.dat (ST_CACHE_LINE_REPLICATION) as the
        reference writes it (gg_stats_trace_dump)."""
        L = load()
        need = ctypes.c_uint64(0)
        _check(L.gg_stats_trace_dump(self.h, which, None, 0, ctypes.byref(need)))
        buf = ctypes.create_string_buffer(need.value)
        _check(L.gg_stats_trace_dump(self.h, which, buf, need.value, ctypes.byref(need)))
        return buf.value.decode()

    def queue_delay_batch(self, pkt_time, proc_time, min_processing_time=1):
        t = np.ascontiguousarray(pkt_time, np.uint64)
        p = np.ascontiguousarray(proc_time, np.uint64)
        d = np.zeros(t.size, np.uint64)
        _check(load().gg_queue_delay_batch(self.h, min_processing_time, t.ctypes.data_as(ctypes.c_void_p),
                                           p.ctypes.data_as(ctypes.c_void_p), t.size,
                                           d.ctypes.data_as(ctypes.c_void_p)))
        return d


def coherent_run_many(backends, addrs, metas, tile_offsets, outs=None, stream=None):
    """An ensemble of independent coherent runs in one set of launches
    (gg_coherent_run_many): backends[i] runs the trace addrs[i] / metas[i] /
    tile_offsets[i] into outs[i] (outs, or an entry, may be None).  The
    backends must be launch-compatible (include/graphite_gpu.h).  Returns the
    list of per-instance statuses; if any is non-zero raises GGError carrying
    that list (e.statuses) — the other instances have run to their end."""
    import torch
    n = len(backends)
    if not (len(addrs) == len(metas) == len(tile_offsets) == n) or (outs is not None and len(outs) != n):
        raise ValueError("one trace (and one output, if any) per backend")
    traces = (_Trace * max(n, 1))()
    keep = []                                       # the host offset arrays, alive for the call
    for i, be in enumerate(backends):
        if outs is not None and outs[i] is not None:
            _need_dev(outs[i], torch.int64, addrs[i].numel())
        traces[i] = be._trace(addrs[i], metas[i], tile_offsets[i])
        keep.append(be._keep)
    hs = (ctypes.c_void_p * max(n, 1))(*[be.h for be in backends])
    op = None
    if outs is not None:
        op = (ctypes.c_void_p * max(n, 1))(*[o.data_ptr() if o is not None else None for o in outs])
    st = (ctypes.c_int * max(n, 1))()
    rc = load().gg_coherent_run_many(hs, n, traces, op, st, _stream(stream))
    del keep
    statuses = [int(st[i]) for i in range(n)]
    if rc != GG_OK:
        raise GGError(rc, load().gg_last_error().decode(errors="replace"), statuses)
    return statuses


def coherent_advance_many(backends, stops=None, stream=None):
    """An ensemble in legs (gg_coherent_advance_many): every backend has a
    begun run (coherent_begin or coherent_restore); all of them are driven in
    one set of launches until each is over or the quantum it would run next
    is >= stops[i] (stops None, or an entry None: never).  Instances with a
    statistics trace sample as a lone coherent_run does.  Returns the list of
    (next_quantum, done) per instance, done 0 paused, 1 over.  If any
    instance fails raises GGError carrying the per-instance statuses
    (e.statuses) and that list (e.results) — the other instances have run to
    their stop."""
    n = len(backends)
    if stops is not None and len(stops) != n:
        raise ValueError("one stop per backend")
    hs = (ctypes.c_void_p * max(n, 1))(*[be.h for be in backends])
    sp = None
    if stops is not None:
        sp = (ctypes.c_uint64 * max(n, 1))(*[Backend.NEVER if q is None else int(q) for q in stops])
    nq = (ctypes.c_uint64 * max(n, 1))()
    dn = (ctypes.c_int * max(n, 1))()
    st = (ctypes.c_int * max(n, 1))()
    rc = load().gg_coherent_advance_many(hs, n, sp, nq, dn, st, _stream(stream))
    results = [(int(nq[i]), int(dn[i])) for i in range(n)]
    if rc != GG_OK:
        e = GGError(rc, load().gg_last_error().decode(errors="replace"), [int(st[i]) for i in range(n)])
        e.results = results
        raise e
    return results


def window_snapshot_state(blob, num_tiles):
    """(consumed, finished) of a windowed run's snapshot
    (gg_window_snapshot_state): uint64 / bool [num_tiles].  No backend and no
    device: a fresh process cuts its first windows from the snapshot alone."""
    b = np.ascontiguousarray(np.frombuffer(blob, np.uint8) if isinstance(blob, (bytes, bytearray)) else blob, np.uint8)
    c, f = np.zeros(max(num_tiles, 1), np.uint64), np.zeros(max(num_tiles, 1), np.uint8)
    _check(load().gg_window_snapshot_state(b.ctypes.data_as(ctypes.c_void_p), b.size, num_tiles,
                                           c.ctypes.data_as(ctypes.c_void_p), f.ctypes.data_as(ctypes.c_void_p)))
    return c[:num_tiles], f[:num_tiles].astype(bool)


def noc_route_batch_many(backends, batches, outs, stream=None):
    """Many NoC batches in one set of launches (gg_noc_route_batch_many):
    backends[i] routes batches[i] = (src, dst, length_bits, time_ps) into
    outs[i] = (arrival, zero_load, contention), exactly as its
    noc_route_batch would.  The backends must be launch-compatible
    (include/graphite_gpu.h).  Returns the list of per-instance statuses; if
    any is non-zero raises GGError carrying that list (e.statuses) — the other
    instances have been routed."""
    import torch
    n = len(backends)
    if not (len(batches) == len(outs) == n):
        raise ValueError("one batch and one output triple per backend")
    pks = (_Packets * max(n, 1))()
    pos = (_PacketOut * max(n, 1))()
    for i in range(n):
        src, dst, length_bits, time_ps = batches[i]
        arrival, zero_load, contention = outs[i]
        m = src.numel()
        for t, dt in ((src, torch.int32), (dst, torch.int32), (length_bits, torch.int32), (time_ps, torch.int64),
                      (arrival, torch.int64), (zero_load, torch.int64), (contention, torch.int64)):
            _need_dev(t, dt, m)
        pks[i] = _Packets(src.data_ptr(), dst.data_ptr(), length_bits.data_ptr(), time_ps.data_ptr(), m)
        pos[i] = _PacketOut(arrival.data_ptr(), zero_load.data_ptr(), contention.data_ptr())
    hs = (ctypes.c_void_p * max(n, 1))(*[be.h for be in backends])
    st = (ctypes.c_int * max(n, 1))()
    rc = load().gg_noc_route_batch_many(hs, n, pks, pos, st, _stream(stream))
    statuses = [int(st[i]) for i in range(n)]
    if rc != GG_OK:
        raise GGError(rc, load().gg_last_error().decode(errors="replace"), statuses)
    return statuses


def noc_synthetic_run_many(backends, params, stream=None):
    """gg_noc_synthetic_run_many: backends[i] generates, routes and reduces
    params[i] (TrafficParams) as its noc_synthetic_run would, all instances in
    one set of launches.  Returns the [n][NUM_NLS] words; if an instance fails
    raises GGError carrying the per-instance statuses (e.statuses) and that
    array (e.stats; the rows of failed instances are zero) — the other
    instances have run."""
    n = len(backends)
    if len(params) != n:
        raise ValueError("one TrafficParams per backend")
    ps = (TrafficParams * max(n, 1))()
    for i, p in enumerate(params):
        ps[i] = p
    stats = np.zeros((n, NUM_NLS), np.uint64)
    hs = (ctypes.c_void_p * max(n, 1))(*[be.h for be in backends])
    st = (ctypes.c_int * max(n, 1))()
    rc = load().gg_noc_synthetic_run_many(hs, n, ps, stats.ctypes.data_as(ctypes.c_void_p), st, _stream(stream))
    if rc != GG_OK:
        e = GGError(rc, load().gg_last_error().decode(errors="replace"), [int(st[i]) for i in range(n)])
        e.stats = stats
        raise e
    return stats


def shard_map(num_tiles, num_shards):
    """tile -> logical shard through the ABI (gg_shard_map)."""
    out = np.zeros(num_tiles, np.uint32)
    _check(load().gg_shard_map(num_tiles, num_shards, out.ctypes.data_as(ctypes.c_void_p)))
    return out


def atac_topology(num_tiles, params):
    """gg_atac_topology: (cluster_of, access_point_of, hub_of_cluster, star_index_of)."""
    T = int(num_tiles)
    _check(load().gg_atac_topology(T, ctypes.byref(params), None, None, None, None))   # the checks, before any buffer
    outs = [np.zeros(n, np.uint32) for n in (T, T, T // params.cluster_size, T)]
    _check(load().gg_atac_topology(T, ctypes.byref(params), *[o.ctypes.data_as(ctypes.c_void_p) for o in outs]))
    return tuple(outs)


def gen_uniform_trace(addr, meta, tile_begin, tiles, per_tile, first=0, lines_log2=15, base_shift=26, stream=None):
    """Fill device tensors with the configs[1] synthetic trace."""
    _check(load().gg_gen_uniform_trace(_ptr(addr), _ptr(meta), tile_begin, tiles, per_tile, first,
                                       lines_log2, base_shift, _stream(stream)))


def gen_hotspot_trace(addr, meta, tile_begin, tiles, per_tile, first=0, lines_log2=15, base_shift=26,
                      hot_lines=64, hot_frac256=51, stream=None):
    """Fill device tensors with the configs[2..4] hotspot trace."""
    _check(load().gg_gen_hotspot_trace(_ptr(addr), _ptr(meta), tile_begin, tiles, per_tile, first, lines_log2,
                                       base_shift, hot_lines, hot_frac256, _stream(stream)))


def gen_stress_trace(addr, meta, tile_begin, tiles, per_tile, num_tiles, first=0, lines_log2=15, base_shift=26,
                     pool_lines=4096, pool_frac256=77, stream=None):
    """Fill device tensors with the configs[4] coherent stress trace."""
    _check(load().gg_gen_stress_trace(_ptr(addr), _ptr(meta), tile_begin, tiles, per_tile, first, lines_log2,
                                      base_shift, num_tiles, pool_lines, pool_frac256, _stream(stream)))


def gen_network_traffic(params, num_tiles, frequency_ghz, src, dst, length_bits, time_ps, last_cycle=None,
                        stream=None):
    """gg_gen_network_traffic: fill device tensors (int32 x 3, int64; num_tiles x
    params.packets_per_tile entries, tile-major) with the synthetic_network
    benchmark's packets; last_cycle (int64, num_tiles) receives the cycle of
    every tile's last packet."""
    import torch
    n = num_tiles * params.packets_per_tile
    for t, dt in ((src, torch.int32), (dst, torch.int32), (length_bits, torch.int32), (time_ps, torch.int64)):
        _need_dev(t, dt, n)
    if last_cycle is not None:
        _need_dev(last_cycle, torch.int64, num_tiles)
    _check(load().gg_gen_network_traffic(ctypes.byref(params), num_tiles, frequency_ghz, _ptr(src), _ptr(dst),
                                         _ptr(length_bits), _ptr(time_ps), _ptr(last_cycle), _stream(stream)))


def noc_latency_stats(src, dst, length_bits, time_ps, arrival, zero_load, contention, stream=None):
    """gg_noc_latency_stats: the NUM_NLS words (NLS_*) of a routed batch, reduced
    on the device (the tensors of Backend.noc_route_batch)."""
    import torch
    n = src.numel()
    for t, dt in ((src, torch.int32), (dst, torch.int32), (length_bits, torch.int32), (time_ps, torch.int64),
                  (arrival, torch.int64), (zero_load, torch.int64), (contention, torch.int64)):
        _need_dev(t, dt, n)
    pk = _Packets(src.data_ptr(), dst.data_ptr(), length_bits.data_ptr(), time_ps.data_ptr(), n)
    out = _PacketOut(arrival.data_ptr(), zero_load.data_ptr(), contention.data_ptr())
    stats = np.zeros(NUM_NLS, np.uint64)
    _check(load().gg_noc_latency_stats(ctypes.byref(pk), ctypes.byref(out), stats.ctypes.data_as(ctypes.c_void_p),
                                       _stream(stream)))
    return stats


def gen_memory_traffic(params, num_tiles, line_bytes=64, stream=None):
    """gg_gen_memory_traffic, both steps: plan (tile offsets and the record
    total), then fill into fresh device tensors.  Returns (addr int64, meta
    int32, tile_offsets [host uint64, num_tiles + 1], tail_cycles int64
    [tiles], type_counts int64 [tiles][6]); addr, meta and tile_offsets are a
    trace for any coherent driver."""
    import torch
    L = load()
    offs = np.zeros(num_tiles + 1, np.uint64)
    total = ctypes.c_uint64(0)
    po = offs.ctypes.data_as(ctypes.c_void_p)
    _check(L.gg_gen_memory_traffic(ctypes.byref(params), num_tiles, line_bytes, po, ctypes.byref(total), None, None, 0,
                                   None, None, _stream(stream)))
    n = int(total.value)
    addr = torch.zeros(max(n, 1), dtype=torch.int64, device="cuda")
    meta = torch.zeros(max(n, 1), dtype=torch.int32, device="cuda")
    tail = torch.zeros(num_tiles, dtype=torch.int64, device="cuda")
    types = torch.zeros((num_tiles, NUM_MEM_INS_TYPES), dtype=torch.int64, device="cuda")
    _check(L.gg_gen_memory_traffic(ctypes.byref(params), num_tiles, line_bytes, po, ctypes.byref(total), _ptr(addr),
                                   _ptr(meta), n, _ptr(tail), _ptr(types), _stream(stream)))
    return addr[:n], meta[:n], offs, tail, types


def mem_latency_stats(meta, access_out, stream=None):
    """gg_mem_latency_stats: the NUM_MLS words (config.MLS_*) of a coherent
    run's access words, reduced on the device; meta is the trace's (BARRIER
    records are skipped, CONT records counted)."""
    import torch
    n = meta.numel()
    _need_dev(meta, torch.int32, n)
    _need_dev(access_out, torch.int64, n)
    tr = _Trace(None, meta.data_ptr() if n else None, None, n)
    stats = np.zeros(NUM_MLS, np.uint64)
    _check(load().gg_mem_latency_stats(ctypes.byref(tr), _ptr(access_out) if n else None,
                                       stats.ctypes.data_as(ctypes.c_void_p), _stream(stream)))
    return stats


def split_accesses(addr, size, meta, tile_offsets, line_size=64, stream=None):
    """Multi-line accesses -> line records (gg_split_accesses, core.cc:139-266).
    addr (int64 byte addresses), size (int32 bytes), meta (int32) are device
    tensors of a tile-major access trace with host tile_offsets [tiles + 1].
    Returns (line_addr, line_meta, first, line_tile_offsets): device tensors
    of the line trace (later lines GG_META_CONT), each access's first line
    (n + 1 entries) and the line trace's host tile offsets."""
    import torch
    offs = np.ascontiguousarray(tile_offsets, dtype=np.uint64)
    tiles = len(offs) - 1
    n = int(offs[-1]) if tiles > 0 else 0
    first = torch.empty(n + 1, dtype=torch.int64, device=addr.device)
    nl = ctypes.c_uint64(0)
    loffs = np.zeros(tiles + 1, np.uint64)
    L = load()
    _check(L.gg_split_accesses(_ptr(addr), _ptr(size), _ptr(meta), offs.ctypes.data_as(ctypes.c_void_p), tiles,
                               line_size, _ptr(first), None, None, 0, ctypes.byref(nl), None, _stream(stream)))
    la = torch.empty(max(nl.value, 1), dtype=torch.int64, device=addr.device)
    lm = torch.empty(max(nl.value, 1), dtype=torch.int32, device=addr.device)
    _check(L.gg_split_accesses(_ptr(addr), _ptr(size), _ptr(meta), offs.ctypes.data_as(ctypes.c_void_p), tiles,
                               line_size, _ptr(first), _ptr(la), _ptr(lm), nl.value, ctypes.byref(nl),
                               loffs.ctypes.data_as(ctypes.c_void_p), _stream(stream)))
    return la[:nl.value], lm[:nl.value], first, loffs


def combine_accesses(line_out, first, stream=None):
    """Per-access (latency_ps, misses) of a coherent run over a split trace
    (gg_combine_accesses, core.cc:239-266): device int64 / int32 tensors."""
    import torch
    n = first.numel() - 1
    lat = torch.empty(max(n, 0), dtype=torch.int64, device=first.device)
    miss = torch.empty(max(n, 0), dtype=torch.int32, device=first.device)
    _check(load().gg_combine_accesses(_ptr(line_out), _ptr(first), max(n, 0), _ptr(lat), _ptr(miss), _stream(stream)))
    return lat, miss


def gen_iocoom_streams(T, per_tile, seed, regs=24, addrs=24, p_sync=0.01, max_lat=300000):
    """Tile-major instructions (random read / write registers from `regs`
    registers, 0-2 memory reads and 0-1 memory writes, simple-mov loads,
    atomics, fences, SyncInstructions) and the access stream their memory
    operands consume in order (addresses from `addrs` per tile, so loads hit
    the store buffer; 0xFFFFFFFF records with and without a stall)."""
    from . import config as C_
    rng = np.random.default_rng(seed)
    n = T * per_tile
    ins = np.zeros(n, C_.INS_DTYPE)
    sync = rng.random(n) < p_sync
    nr = rng.integers(0, 4, n)
    nw = np.minimum(rng.integers(0, 3, n), 6 - nr)
    nrd = rng.choice(3, n, p=[0.55, 0.35, 0.10])
    nwm = (rng.random(n) < 0.25).astype(np.int64)
    smov = (nrd == 1) & (nwm == 0) & (nw == 1) & (rng.random(n) < 0.6)
    fence = np.where(rng.random(n) < 0.03, rng.integers(1, 4, n), 0)
    atomic = rng.random(n) < 0.02
    nr[sync] = 0; nw[sync] = 0; nrd[sync] = 0; nwm[sync] = 0; smov[sync] = False; fence[sync] = 0; atomic[sync] = False
    ins["cost"] = rng.choice(np.array([0, 1, 1, 1, 3, 5, 6, 18]), n)
    ins["ops"] = (nrd | (nwm << 2) | np.where(smov, C_.INS_SIMPLE_MOV_LOAD, 0) |
                  np.where(atomic, C_.INS_ATOMIC, 0) | (fence << C_.INS_FENCE_SHIFT)).astype(np.uint8)
    ins["regs"] = (nr | (nw << 3) | np.where(sync, C_.INS_SYNC, 0)).astype(np.uint8)
    ins["reg"] = rng.integers(0, regs, (n, 6)).astype(np.uint16)
    ins_offs = np.arange(T + 1, dtype=np.uint64) * np.uint64(per_tile)
    cnt = np.where(sync, 1, nrd + nwm)
    tot = int(cnt.sum())
    owner = np.repeat(np.arange(n), cnt)
    pos = np.arange(tot) - np.repeat(np.cumsum(cnt) - cnt, cnt)
    is_bar = sync[owner]
    is_wr = ~is_bar & (pos >= nrd[owner])
    meta = np.where(is_bar, np.uint32(0xFFFFFFFF), np.where(is_wr, np.uint32(1), np.uint32(0))).astype(np.uint32)
    meta[~is_bar] |= (rng.integers(0, 8, int((~is_bar).sum())) << 1).astype(np.uint32)   # gap bits: ignored
    tile = owner // per_tile
    addr = (tile.astype(np.uint64) << np.uint64(20)) + rng.integers(0, addrs, tot).astype(np.uint64) * np.uint64(8)
    lat = rng.integers(1000, max_lat, tot).astype(np.uint64)
    lat[is_bar & (rng.random(tot) < 0.3)] = 0
    per = np.bincount(tile, minlength=T)
    acc_offs = np.concatenate([[0], np.cumsum(per)]).astype(np.uint64)
    return ins, ins_offs, addr, meta, lat, acc_offs


class CoherentEngine:
    """A Backend context behind the engine surface of graphite_amd.coherent.run
    (one rank: the shards [cfg.shard_begin, cfg.shard_end))."""

    def __init__(self, backend, addr, meta, tile_offsets, out=None):
        import torch
        self.be = backend
        self.dev = addr.device
        backend.coherent_begin(addr, meta, tile_offsets, out)
        self.cap = 64 * backend.cfg.num_tiles + 65536
        self.buf = torch.empty(self.cap * CMSG_BYTES, dtype=torch.uint8, device=self.dev)

    def quantum(self, q):
        return self.be.coherent_quantum(q)

    def export(self):
        counts = self.be.coherent_export(self.buf, self.cap)
        n = int(counts.sum())
        return self.buf[:n * CMSG_BYTES], counts

    def import_(self, buf):
        n = buf.numel() // CMSG_BYTES
        if n:
            self.be.coherent_import(buf.contiguous(), n)
