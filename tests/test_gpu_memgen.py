"""Synthetic memory traffic on the GPU: the generator
gg_gen_memory_traffic bit for bit against tests/memgen_model.py, its rejections,
gg_mem_synthetic_run against the oracle's run of the model's trace, the
reduction gg_mem_latency_stats against numpy, and a generated trace through
gg_coherent_run_many."""
import ctypes
import functools
import os
import re

import numpy as np
import pytest

from graphite_amd import config as C
from graphite_amd import backend as B
import memgen_model as M
from gpu_util import torch_dev, to_dev, to_np

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "synthetic_memory")
P64 = (0.7, 0.025, 0.060, 0.015, 0.14, 0.06)             # input.64's probabilities
P97 = (0.97, 0.005, 0.005, 0.005, 0.01, 0.005)
P0 = (0.0, 0.1, 0.2, 0.2, 0.3, 0.2)
CHUNK = 1024                                              # instructions of a (tile, chunk) wave


def params(T, degree=1, shared=1024, private=256, N=2000, prob=P64, seed_base=0, map_seed=1):
    return C.MemTrafficParams(T, degree, shared, private, N, prob, seed_base, map_seed)


@functools.lru_cache(maxsize=None)
def model(key, T, line=64):
    """The model's trace of params(*key): computed once per case, shared, never written to."""
    return M.generate(params(*key), T, line)


# ---- A. the generator against the model (B: the model raising ModelError would show a GG_ERR_STATE case) ----
GEN_CASES = {
    "input.64": ((64, 1, 1024, 256, 10000), 64, 64),
    "16_shared_mostly_empty_lists": ((64, 1, 16, 256, 3000), 64, 64),
    "input.test_at_16_tiles": ((16, 16, 128, 0, 5000, (0.0, 1.0, 0.0, 0.0, 0.0, 0.0)), 16, 64),
    "p0_97_no_record_tiles": ((16, 1, 1024, 256, 50, P97), 16, 64),
    "p0_97_gaps_beyond_a_round": ((16, 1, 1024, 256, 3000, P97), 16, 64),
    "p0_0_no_gaps": ((16, 1, 1024, 256, 300, P0), 16, 64),
    "private_1": ((16, 1, 1024, 1, 2000), 16, 64),
    "private_4": ((16, 1, 1024, 4, 2000), 16, 64),
    "36_tiles": ((36, 2, 256, 256, 2000), 36, 64),
    "seed_base_7_map_seed_3": ((16, 1, 1024, 256, 2000, P64, 7, 3), 16, 64),
    "line_128": ((16, 1, 1024, 256, 2000), 16, 128),
}
for _n in (1, 63, 64, 65, CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK + 1):
    GEN_CASES["N_%d" % _n] = ((16, 1, 1024, 256, _n), 16, 64)


@pytest.mark.parametrize("name", sorted(GEN_CASES))
def test_generator_matches_model(name):
    torch_dev()
    key, T, line = GEN_CASES[name]
    ref = model(key, T, line)
    addr, meta, offs, tail, types = B.gen_memory_traffic(params(*key), T, line)
    np.testing.assert_array_equal(offs, ref["tile_offsets"], err_msg="tile_offsets")
    np.testing.assert_array_equal(to_np(types, np.uint64).reshape(T, 6), ref["type_counts"], err_msg="type_counts")
    np.testing.assert_array_equal(to_np(tail, np.uint64), ref["tail"], err_msg="tail_cycles")
    np.testing.assert_array_equal(to_np(meta, np.uint32), ref["meta"], err_msg="meta")
    np.testing.assert_array_equal(to_np(addr, np.uint64), ref["addr"], err_msg="addr")
    if name == "input.64":
        f = C.MemTrafficParams.from_input_file(os.path.join(GOLDEN, "input.64"))
        assert bytes(f) == bytes(params(*key))
    if name == "16_shared_mostly_empty_lists":
        assert int((ref["skipped"] > 0).sum()) >= 49
    if name == "p0_97_no_record_tiles":
        assert (np.diff(ref["tile_offsets"].astype(np.int64)) == 0).any() and (ref["tail"] > 0).any()
    if name == "p0_97_gaps_beyond_a_round":
        assert int((ref["meta"] >> 1).max()) > 64
    if name == "p0_0_no_gaps":
        assert not (ref["meta"] >> 1).any() and not ref["tail"].any()


def test_plan_alone_and_small_capacity():
    torch = torch_dev()
    T, p = 16, params(16)
    ref = model((16,), T)
    offs, total = np.zeros(T + 1, np.uint64), ctypes.c_uint64(0)
    L = B.load()
    B._check(L.gg_gen_memory_traffic(ctypes.byref(p), T, 64, offs.ctypes.data_as(ctypes.c_void_p),
                                     ctypes.byref(total), None, None, 0, None, None, B._stream(None)))
    np.testing.assert_array_equal(offs, ref["tile_offsets"])
    n = int(total.value)
    assert n == int(ref["tile_offsets"][-1])
    addr = torch.zeros(n, dtype=torch.int64, device="cuda")
    meta = torch.zeros(n, dtype=torch.int32, device="cuda")
    rc = L.gg_gen_memory_traffic(ctypes.byref(p), T, 64, None, None, B._ptr(addr), B._ptr(meta), n - 1, None, None,
                                 B._stream(None))
    assert rc == M.INVALID
    assert not to_np(meta, np.uint32).any()                          # nothing was written
    B._check(L.gg_gen_memory_traffic(ctypes.byref(p), T, 64, None, None, B._ptr(addr), B._ptr(meta), n, None, None,
                                     B._stream(None)))
    np.testing.assert_array_equal(to_np(addr, np.uint64), ref["addr"])


# ---- C. errors -----------------------------------------------------------------------------------
BAD = [
    (M.INVALID, dict(shared=24), 64), (M.INVALID, dict(shared=0), 64), (M.INVALID, dict(private=3), 64),
    (M.INVALID, dict(private=0), 64), (M.INVALID, dict(degree=17), 64), (M.INVALID, dict(N=0), 64),
    (M.INVALID, dict(prob=(0.7, -0.1, 0.1, 0.1, 0.1, 0.1)), 64), (M.INVALID, dict(prob=(1.5, 0, 0, 0, 0, 0)), 64),
    (M.INVALID, dict(prob=(float("nan"), 0, 0, 0, 0, 0)), 64), (M.INVALID, dict(prob=(float("inf"), 0, 0, 0, 0, 0)), 64),
    (M.INVALID, dict(), 48), (M.INVALID, dict(), 0),
    (M.RANGE, dict(shared=1 << 25), 64), (M.RANGE, dict(private=1 << 27), 64), (M.RANGE, dict(N=1 << 31), 64),
]


@pytest.mark.parametrize("code,kw,line", BAD)
def test_rejections(code, kw, line):
    torch_dev()
    with pytest.raises(B.GGError) as e:
        B.gen_memory_traffic(params(16, **kw), 16, line)
    assert e.value.code == code
    if line == 64 and not any(isinstance(x, float) and x != x for x in kw.get("prob", ())):
        with pytest.raises(M.ModelError) as me:                      # the model agrees on the kind
            M.check(params(16, **kw), 16, line)
        assert me.value.code == code


def test_null_arguments_and_atac():
    torch = torch_dev()
    L = B.load()
    s = B._stream(None)
    stats = np.zeros(C.NUM_MLS, np.uint64)
    sp = stats.ctypes.data_as(ctypes.c_void_p)
    assert L.gg_gen_memory_traffic(None, 16, 64, None, None, None, None, 0, None, None, s) == M.INVALID
    p = params(16)
    meta = torch.zeros(8, dtype=torch.int32, device="cuda")
    assert L.gg_gen_memory_traffic(ctypes.byref(p), 16, 64, None, None, None, B._ptr(meta), 8, None, None, s) == M.INVALID
    assert L.gg_gen_memory_traffic(ctypes.byref(params(16, N=10)), 8, 64, None, None, None, None, 0, None, None,
                                   s) == M.INVALID             # num_threads 16 on 8 tiles
    assert L.gg_mem_latency_stats(None, None, sp, s) == M.INVALID
    tr = B._Trace(None, None, None, 8)
    assert L.gg_mem_latency_stats(ctypes.byref(tr), None, sp, s) == M.INVALID
    be = B.Backend(C.default_config(16))
    assert L.gg_mem_synthetic_run(be.h, None, sp, s) == M.INVALID
    assert L.gg_mem_synthetic_run(be.h, ctypes.byref(p), None, s) == M.INVALID
    assert L.gg_mem_synthetic_run(None, ctypes.byref(p), sp, s) == M.INVALID
    assert L.gg_mem_synthetic_get(be.h, None, None, None, None) == M.INVALID        # no run yet
    be.close()
    atac = B.Backend(C.default_config(64, net_model=C.NET_ATAC))
    with pytest.raises(B.GGError) as e:
        atac.mem_synthetic_run(params(64))
    assert e.value.code == -3
    atac.close()


def test_a_draw_that_names_no_type_is_reported_after_the_launch():
    """Probabilities summing to 0.5: half the draws lie at or above cum[5]."""
    torch_dev()
    key = (16, 1, 1024, 256, 2 * CHUNK + 1, (0.25, 0.05, 0.05, 0.05, 0.05, 0.05))
    with pytest.raises(M.ModelError) as me:
        M.generate(params(*key), 16)
    assert me.value.code == M.STATE
    with pytest.raises(B.GGError) as e:
        B.gen_memory_traffic(params(*key), 16)
    assert e.value.code == M.STATE
    where = re.search(r"tile (\d+) instruction (\d+)", str(e.value))
    assert where and (int(where.group(1)), int(where.group(2))) == me.value.where


# ---- D. gg_mem_synthetic_run against the oracle ------------------------------------------------------
RUN_CASES = {
    "msi_hop_counter_16": (16, 1, dict(net_model=C.NET_EMESH_HOP_COUNTER)),
    "mosi_16": (16, 1, dict(protocol=C.PROTO_MOSI)),
    "shl2_mesi_16": (16, 1, dict(protocol=C.PROTO_SHL2_MESI)),
    "msi_hop_by_hop_64_degree_8": (64, 8, dict(net_model=C.NET_EMESH_HOP_BY_HOP)),
    "msi_1_5_ghz_16": (16, 1, dict(net_model=C.NET_EMESH_HOP_COUNTER, frequency_ghz=1.5)),
}


@pytest.mark.parametrize("name", sorted(RUN_CASES))
def test_synthetic_run_matches_oracle(name):
    from oracle import pyoracle as po
    from coherent_util import _oracle_run
    torch_dev()
    T, degree, kw = RUN_CASES[name]
    cfg = C.default_config(T, **kw)
    key = (T, degree)
    ref = model(key, T)
    a, m, o = ref["addr"], ref["meta"], ref["tile_offsets"]
    rout, rst, rcc, rnet, _ = _oracle_run(cfg, a, m, o)
    be = B.Backend(cfg)
    stats = be.mem_synthetic_run(params(*key))
    addr, meta, offs, out, tail, types = be.mem_synthetic_trace()
    np.testing.assert_array_equal(offs, o)
    np.testing.assert_array_equal(to_np(addr, np.uint64), a)
    np.testing.assert_array_equal(to_np(meta, np.uint32), m)
    np.testing.assert_array_equal(to_np(tail, np.uint64), ref["tail"])
    np.testing.assert_array_equal(to_np(types, np.uint64).reshape(T, 6), ref["type_counts"])
    gout = to_np(out, np.uint64)
    np.testing.assert_array_equal(gout, rout, err_msg="access words")
    gst, gcc, _ = be.coherent_stats()
    np.testing.assert_array_equal(gst, rst, err_msg="tile stats")
    np.testing.assert_array_equal(gcc, rcc, err_msg="cache counters")
    np.testing.assert_array_equal(be.noc_counters(), rnet, err_msg="noc counters")
    cycle = int(po.lib().oracle_lat_to_ps(1, float(cfg.frequency_ghz)))
    if name == "msi_1_5_ghz_16":
        assert cycle == 667
    want = M.numpy_stats(m, rout, C.NUM_MLS, C.MLS_HIST)
    want[C.MLS_TYPE_COUNTS:C.MLS_TYPE_COUNTS + 6] = ref["type_counts"].sum(axis=0)
    want[C.MLS_MAX_TILE_CLOCK_PS] = (rst[:, 0] + ref["tail"] * np.uint64(cycle)).max()
    np.testing.assert_array_equal(stats, want)
    assert stats[C.MLS_L2_MISSES] > 0 and ref["tail"].any()
    if degree > 1:
        assert gst[:, C.TILE_STATS.index("sent_inv_req")].sum() > 0           # real sharing: invalidations were sent
    be.close()


# ---- E. the reduction alone ----------------------------------------------------------------------------
def _reduce_and_compare(cfg, a, m, o):
    from coherent_util import _oracle_run
    torch = torch_dev()
    be = B.Backend(cfg)
    addr, meta = to_dev(torch, a, torch.int64), to_dev(torch, m, torch.int32)
    out = torch.zeros(len(a), dtype=torch.int64, device="cuda")
    be.coherent_run(addr, meta, o, out)
    torch.cuda.synchronize()
    rout = _oracle_run(cfg, a, m, o)[0]
    np.testing.assert_array_equal(to_np(out, np.uint64), rout)
    np.testing.assert_array_equal(B.mem_latency_stats(meta, out), M.numpy_stats(m, rout, C.NUM_MLS, C.MLS_HIST))
    be.close()


def test_latency_stats_of_a_split_trace():
    from oracle import pyoracle as po
    from tests.access_util import gen_multiline
    addr, size, meta, offs = gen_multiline(16, 300)
    la, lm, _, lo = po.split_accesses(addr, size, meta, offs)
    assert ((lm >> np.uint32(31)) == 1).any() and not (lm == np.uint32(C.META_BARRIER)).any()     # CONT records
    _reduce_and_compare(C.default_config(16, net_model=C.NET_EMESH_HOP_COUNTER), la, lm, lo)


def test_latency_stats_of_a_barrier_trace():
    from oracle import pyoracle as po
    from replication_util import with_barriers
    a, m, o = with_barriers(*po.gen_trace(16, 300, hot_lines=16), 100)
    assert (m == np.uint32(C.META_BARRIER)).sum() == 32
    _reduce_and_compare(C.default_config(16, net_model=C.NET_EMESH_HOP_COUNTER), a, m, o)


def test_latency_stats_of_an_empty_trace():
    torch = torch_dev()
    s = B.mem_latency_stats(torch.zeros(0, dtype=torch.int32, device="cuda"),
                            torch.zeros(0, dtype=torch.int64, device="cuda"))
    assert not s.any()


# ---- F. a generated trace through the ensemble driver ---------------------------------------------------
def test_two_degrees_of_sharing_side_by_side():
    torch = torch_dev()
    T = 16
    cfg = C.default_config(T, net_model=C.NET_EMESH_HOP_BY_HOP)
    traces = [B.gen_memory_traffic(params(T, degree), T) for degree in (1, 4)]
    assert not np.array_equal(to_np(traces[0][0], np.uint64), to_np(traces[1][0], np.uint64))
    single = []
    for addr, meta, offs, _, _ in traces:
        be = B.Backend(cfg)
        out = torch.zeros(addr.numel(), dtype=torch.int64, device="cuda")
        be.coherent_run(addr, meta, offs, out)
        torch.cuda.synchronize()
        single.append((to_np(out, np.uint64), be.coherent_stats()[0], be.noc_counters()))
        be.close()
    bes = [B.Backend(cfg) for _ in traces]
    outs = [torch.zeros(t[0].numel(), dtype=torch.int64, device="cuda") for t in traces]
    assert B.coherent_run_many(bes, [t[0] for t in traces], [t[1] for t in traces], [t[2] for t in traces], outs) == [0, 0]
    torch.cuda.synchronize()
    for be, out, (sout, sst, snet) in zip(bes, outs, single):
        np.testing.assert_array_equal(to_np(out, np.uint64), sout)
        np.testing.assert_array_equal(be.coherent_stats()[0], sst)
        np.testing.assert_array_equal(be.noc_counters(), snet)
        be.close()


# ---- G. the command-line tool ------------------------------------------------------------------------------
def test_gg_replay_prints_the_benchmarks_figures():
    import subprocess
    torch_dev()
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = os.path.join(root, "graphite_amd", "host", "gg_replay")
    r = subprocess.run([exe, "--coherent", "--synthetic-memory", os.path.join(GOLDEN, "input.64"), "-ns", "2",
                        "--tiles", "16"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    lines = r.stdout.splitlines()
    key = (16, 2, 1024, 256, 10000)
    ref = model(key, 16)
    want = ["thread(%d) -> %s" % (t, "".join("%d\t" % c for c in ref["type_counts"][t])) for t in range(16)]
    assert lines[:16] == want
    be = B.Backend(C.default_config(16, net_model=C.NET_EMESH_HOP_COUNTER))       # gg_replay's defaults
    stats = be.mem_synthetic_run(params(*key))
    be.close()
    ns = -(-int(stats[C.MLS_MAX_TILE_CLOCK_PS]) // 1000)                          # Time::toNanosec: the ceiling
    assert lines[16] == "Success: Max Tile Clock(%d ns)" % ns
    assert lines[17].startswith("Synthetic Memory: accesses %d reads %d writes %d " % tuple(stats[:3]))
