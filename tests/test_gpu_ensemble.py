"""gg_coherent_run_many / backend.coherent_run_many: n independent coherent
runs side by side in one set of launches (k_c_step_many / k_c_walk_many, the
instance chosen by blockIdx.y).  Every instance must equal
oracle.pyoracle.OracleCoherent on its own config and trace bit for bit:
access words, tile stats, cache counters, NoC counters and run info.  The
generators take no seed, so the instances differ in per_tile, hot_lines,
hot_frac256 and lines_log2 (and in latency settings where a case says so).

The CPU tests (symbol, the n == 0 rejection, the Python entry point) need no
GPU and fail without the feature."""
import ctypes
import functools

import numpy as np
import pytest

from graphite_amd import backend as B
from graphite_amd import config as C
from tests.gpu_util import torch_dev, to_dev, to_np

HBH, HC = C.NET_EMESH_HOP_BY_HOP, C.NET_EMESH_HOP_COUNTER
GG_ERR_INVALID, GG_ERR_UNSUPPORTED = -1, -3
NAMES = ("access words", "tile stats", "cache counters", "noc counters", "run info")


# ---- CPU: the surface exists (no GPU call) --------------------------------
def test_symbol_and_binding_exist():
    lib = ctypes.CDLL(B.LIB_PATH)
    assert hasattr(lib, "gg_coherent_run_many")
    assert "gg_coherent_run_many" in B.EXPORTS
    assert callable(getattr(B, "coherent_run_many", None))
    assert 0 < B.MANY_MAX <= 65535


def test_n_zero_is_invalid_without_a_gpu():
    L = B.load()
    assert L.gg_coherent_run_many(None, 0, None, None, None, None) == GG_ERR_INVALID
    assert b"n == 0" in L.gg_last_error()


# ---- instances: (config, trace) specs, hashable so the oracle runs once ----
def _spec(T, K, net, per_tile, protocol=C.PROTO_MSI, stress=False, barriers=0, trace=(), cfg=()):
    return (T, K, net, per_tile, protocol, stress, barriers, tuple(sorted(dict(trace).items())),
            tuple(sorted(dict(cfg).items())))


def _cfg(spec):
    T, K, net, _, protocol, _, _, _, cfg = spec
    return C.default_config(T, num_shards=K, net_model=net, protocol=protocol, **dict(cfg))


def _with_barriers(a, m, offs, every):
    """A BARRIER record after every `every` accesses of each tile (as
    tests/test_gpu_round_barriers.py builds its traces)."""
    A, M = [], []
    for t in range(len(offs) - 1):
        s, e = int(offs[t]), int(offs[t + 1])
        pos = np.arange(every, e - s, every)
        A.append(np.insert(a[s:e], pos, np.uint64(0)))
        M.append(np.insert(m[s:e], pos, np.uint32(C.META_BARRIER)))
    o = np.concatenate([[0], np.cumsum([len(x) for x in A])]).astype(np.uint64)
    return np.concatenate(A), np.concatenate(M).astype(np.uint32), o


@functools.lru_cache(maxsize=None)
def _trace(spec):
    from oracle import pyoracle as po
    T, _, _, per_tile, _, stress, barriers, trace, _ = spec
    gen = po.gen_stress_trace if stress else po.gen_trace
    r = gen(T, per_tile, **dict(trace))
    if barriers:
        r = _with_barriers(*r, barriers)
    r = tuple(np.ascontiguousarray(x) for x in r)
    for x in r:
        x.setflags(write=False)
    return r


@functools.lru_cache(maxsize=None)
def _oracle(spec):
    """(access words, tile stats, cache counters, NoC counters, run info,
    miss types, protocol stats) of the oracle, computed once per instance."""
    from oracle import pyoracle as po
    a, m, o = _trace(spec)
    oc = po.OracleCoherent(_cfg(spec))
    r = (oc.run(a, m, o).copy(), oc.tile_stats(), oc.cache_counters(), oc.net_counters(),
         oc.run_info()[:len(C.RUN_INFO)], oc.miss_types(), oc.proto_stats())
    for x in r:
        x.setflags(write=False)
    return r


class _Ensemble:
    """Contexts, device traces and output buffers of a list of specs."""

    def __init__(self, torch, specs):
        self.torch, self.specs = torch, list(specs)
        self.bes = [B.Backend(_cfg(s)) for s in self.specs]
        self.addr, self.meta, self.offs, self.outs = [], [], [], []
        for s in self.specs:
            a, m, o = _trace(s)
            self.addr.append(to_dev(torch, np.array(a), torch.int64))
            self.meta.append(to_dev(torch, np.array(m), torch.int32))
            self.offs.append(o)
            self.outs.append(torch.zeros(len(a), dtype=torch.int64, device="cuda"))

    def run(self, order=None):
        """coherent_run_many over the instances `order` (default: all)."""
        ix = list(range(len(self.specs))) if order is None else list(order)
        for i in ix:
            self.outs[i].zero_()
        pick = lambda xs: [xs[i] for i in ix]
        st = B.coherent_run_many(pick(self.bes), pick(self.addr), pick(self.meta), pick(self.offs), pick(self.outs))
        self.torch.cuda.synchronize()
        return st

    def single(self, i):
        self.outs[i].zero_()
        self.bes[i].coherent_run(self.addr[i], self.meta[i], self.offs[i], self.outs[i])
        self.torch.cuda.synchronize()

    def result(self, i):
        be = self.bes[i]
        st, cc, ri = be.coherent_stats()
        return (to_np(self.outs[i], np.uint64).copy(), st, cc, be.noc_counters(), ri[:len(C.RUN_INFO)],
                be.miss_types(), be.protocol_stats())

    def close(self):
        for be in self.bes:
            be.close()


def _same(got, ref, what, upto=5):
    for name, x, y in zip(NAMES + ("miss types", "protocol stats"), got[:upto], ref[:upto]):
        if not np.array_equal(x, y):
            d = np.argwhere(np.asarray(x) != np.asarray(y))
            raise AssertionError("%s: %s differ at %d places, first %s: %s vs %s"
                                 % (what, name, len(d), d[0], np.asarray(x)[tuple(d[0])], np.asarray(y)[tuple(d[0])]))


def _check_all(specs, upto=5):
    """Run the ensemble once; every instance equals the oracle."""
    torch = torch_dev()
    en = _Ensemble(torch, specs)
    try:
        assert en.run() == [0] * len(specs)
        for i, s in enumerate(specs):
            _same(en.result(i), _oracle(s), "instance %d vs oracle" % i, upto)
    finally:
        en.close()


# ---- GPU cases --------------------------------------------------------------
@pytest.mark.gpu
def test_hop_counter_five_instances():
    """T=16, K=1: five instances of 200-500 records per tile."""
    _check_all([_spec(16, 1, HC, 200, trace=dict(hot_lines=8)),
                _spec(16, 1, HC, 290, trace=dict(hot_lines=16, hot_frac256=90)),
                _spec(16, 1, HC, 350, trace=dict(hot_lines=64, lines_log2=12)),
                _spec(16, 1, HC, 430, trace=dict(hot_lines=32, hot_frac256=20)),
                _spec(16, 1, HC, 500, trace=dict(hot_lines=4, lines_log2=10))])


@pytest.mark.gpu
def test_hop_by_hop_different_settings():
    """T=64, K=8: three instances that also differ in dram_latency_ns,
    router_delay and l2_data_cycles."""
    _check_all([_spec(64, 8, HBH, 200, trace=dict(hot_lines=32)),
                _spec(64, 8, HBH, 260, trace=dict(hot_lines=16, hot_frac256=80),
                      cfg=dict(dram_latency_ns=60, router_delay=2)),
                _spec(64, 8, HBH, 150, trace=dict(hot_lines=64, lines_log2=12),
                      cfg=dict(l2_data_cycles=12, router_delay=2))])


@pytest.mark.gpu
def test_hop_by_hop_different_clocks_and_dram_bandwidths():
    """T=16, K=1: three instances that differ only in frequency_ghz (1.0, 1.5,
    2.66: the exact and the rounding forms of the cycle <-> picosecond
    conversions side by side in one launch set) and dram_bandwidth; each
    equals the oracle and its own lone coherent_run."""
    specs = [_spec(16, 1, HBH, 300, trace=dict(hot_lines=8), cfg=dict(frequency_ghz=f, dram_bandwidth=bw))
             for f, bw in ((1.0, 5.0), (1.5, 3.3), (2.66, 64.0))]
    torch = torch_dev()
    en, lone = _Ensemble(torch, specs), _Ensemble(torch, specs)
    try:
        assert en.run() == [0, 0, 0]
        for i, s in enumerate(specs):
            r = en.result(i)
            _same(r, _oracle(s), "instance %d vs oracle" % i)
            lone.single(i)
            _same(lone.result(i), r, "lone run %d vs ensemble" % i)
        assert not np.array_equal(en.result(0)[0], en.result(1)[0])
    finally:
        en.close()
        lone.close()


@pytest.mark.gpu
def test_hop_by_hop_256_tiles_and_lone_run():
    """T=256, K=8 (the per-step path in a single run too), two instances x 150
    records; each also equals a lone coherent_run on a fresh context."""
    specs = [_spec(256, 8, HBH, 150, trace=dict(hot_lines=64)),
             _spec(256, 8, HBH, 150, trace=dict(hot_lines=16, hot_frac256=100))]
    torch = torch_dev()
    en, lone = _Ensemble(torch, specs), _Ensemble(torch, specs)
    try:
        assert en.run() == [0, 0]
        for i, s in enumerate(specs):
            r = en.result(i)
            _same(r, _oracle(s), "instance %d vs oracle" % i)
            lone.single(i)
            _same(lone.result(i), r, "lone run %d vs ensemble" % i)
    finally:
        en.close()
        lone.close()


@pytest.mark.gpu
@pytest.mark.parametrize("protocol", [C.PROTO_MOSI, C.PROTO_SHL2_MSI, C.PROTO_SHL2_MESI])
def test_other_protocols(protocol):
    """MOSI, pr_l1_sh_l2_msi, pr_l1_sh_l2_mesi: two instances, T=16, 300
    records, all stats and the protocol stats."""
    specs = [_spec(16, 1, HC, 300, protocol, trace=dict(hot_lines=8)),
             _spec(16, 1, HC, 300, protocol, trace=dict(hot_lines=32, hot_frac256=120))]
    torch = torch_dev()
    en = _Ensemble(torch, specs)
    try:
        assert en.run() == [0, 0]
        for i, s in enumerate(specs):
            r, ref = en.result(i), _oracle(s)
            _same(r, ref, "instance %d vs oracle" % i)
            assert np.array_equal(r[6], ref[6]), "instance %d: protocol stats" % i
    finally:
        en.close()


@pytest.mark.gpu
def test_barrier_records():
    """Two instances at T=16 with different barrier counts."""
    specs = [_spec(16, 1, HC, 200, barriers=50, trace=dict(hot_lines=16)),
             _spec(16, 1, HC, 240, barriers=30, trace=dict(hot_lines=8))]
    for s in specs:
        assert int((_trace(s)[1] == C.META_BARRIER).sum()) > 0
    assert len({int((_trace(s)[1] == C.META_BARRIER).sum()) for s in specs}) == 2
    _check_all(specs)
    for s in specs:
        bar = _trace(s)[1] == C.META_BARRIER
        assert np.all((_oracle(s)[0][bar] & np.uint64(3)) == C.LVL_SYNC)


UNEVEN = [_spec(16, 1, HC, 50, trace=dict(hot_lines=8)),
          _spec(16, 1, HC, 400, trace=dict(hot_lines=16, hot_frac256=90)),
          _spec(16, 1, HC, 1500, trace=dict(hot_lines=32, lines_log2=12))]


@pytest.mark.gpu
def test_uneven_lengths_live_list():
    """50, 400 and 1 500 records per tile: the short runs leave the launches
    (the live list is rebuilt after a batch) and the long one runs on."""
    def last_batch(spec):
        """The batch (16, 32, ... 256, 256, ... launches) a run ends in: it
        needs a launch per step and one per quantum end."""
        ri = _oracle(spec)[4]
        need = int(ri[C.RUN_INFO.index("steps")]) + int(ri[C.RUN_INFO.index("quanta")])
        done, size, k = 0, 16, 0
        while done < need:
            done, size, k = done + size, min(2 * size, 256), k + 1
        return k
    ends = [last_batch(s) for s in UNEVEN]
    assert ends[0] < ends[1] < ends[2], ends                 # the live list shrinks twice before the end
    _check_all(UNEVEN)


@pytest.mark.gpu
def test_independence():
    """Order, company and history do not matter: reversed order, each alone
    with n = 1, the same call twice, and a plain coherent_run afterwards."""
    torch = torch_dev()
    en = _Ensemble(torch, UNEVEN)
    try:
        assert en.run() == [0, 0, 0]
        first = [en.result(i) for i in range(3)]
        for i, s in enumerate(UNEVEN):
            _same(first[i], _oracle(s), "instance %d vs oracle" % i)
        assert en.run() == [0, 0, 0]                         # the same contexts again
        for i in range(3):
            _same(en.result(i), first[i], "second call, instance %d" % i)
        assert en.run([2, 1, 0]) == [0, 0, 0]
        for i in range(3):
            _same(en.result(i), first[i], "reversed order, instance %d" % i)
        for i in range(3):
            assert en.run([i]) == [0]
            _same(en.result(i), first[i], "alone, instance %d" % i)
        en.single(1)                                         # a plain run on one of them afterwards
        _same(en.result(1), _oracle(UNEVEN[1]), "plain coherent_run after the ensemble")
    finally:
        en.close()


@pytest.mark.gpu
def test_error_isolation():
    """Three instances with miss tracking on (one kernel variant); one has a
    64-line table on the trace that fills it (test_gpu_miss_types_errors'
    case).  The call raises, that instance has the single-run status, the
    other two are GG_OK and bit-exact, miss types included."""
    track = dict(l1i_track_miss_types=1, l2_track_miss_types=1)
    specs = [_spec(16, 1, HC, 300, trace=dict(hot_lines=32), cfg=track),
             _spec(16, 1, HC, 2000, trace=dict(hot_lines=8), cfg=dict(track, miss_track_lines=64)),
             _spec(16, 1, HC, 450, trace=dict(hot_lines=16, hot_frac256=90), cfg=track)]
    torch = torch_dev()
    en = _Ensemble(torch, specs)
    try:
        with pytest.raises(B.GGError) as single:
            en.single(1)
        with pytest.raises(B.GGError) as ei:
            en.run()
        assert ei.value.code == single.value.code == GG_ERR_UNSUPPORTED
        assert ei.value.statuses == [0, single.value.code, 0]
        for i in (0, 2):
            r, ref = en.result(i), _oracle(specs[i])
            _same(r, ref, "instance %d vs oracle" % i)
            assert np.array_equal(r[5], ref[5]) and r[5].sum() > 0, "instance %d: miss types" % i
    finally:
        en.close()


@pytest.mark.gpu
def test_rejections():
    """Incompatible sets, a context that does not own every shard, a duplicate
    and n above the cap: GG_ERR_INVALID with the index in gg_last_error,
    before anything runs; a following valid call succeeds."""
    torch = torch_dev()
    base = _spec(16, 2, HBH, 120, trace=dict(hot_lines=8))
    other = _spec(16, 2, HBH, 100, trace=dict(hot_lines=16))
    en = _Ensemble(torch, [base, other])
    odd = {"num_tiles": _spec(64, 2, HBH, 20), "protocol": _spec(16, 2, HBH, 20, C.PROTO_MOSI),
           "net_model": _spec(16, 2, HC, 20), "own every shard": _spec(16, 2, HBH, 20, cfg=dict(shard_end=1))}
    extra = _Ensemble(torch, list(odd.values()))
    try:
        def rejected(bes, addrs, metas, offs, index, field):
            with pytest.raises(B.GGError) as ei:
                B.coherent_run_many(bes, addrs, metas, offs)
            assert ei.value.code == GG_ERR_INVALID, ei.value
            assert "context %d" % index in str(ei.value) and field in str(ei.value), ei.value

        for k, (field, _) in enumerate(odd.items()):
            rejected([en.bes[0], en.bes[1], extra.bes[k]], en.addr + [extra.addr[k]], en.meta + [extra.meta[k]],
                     en.offs + [extra.offs[k]], 2, field)
        rejected([en.bes[0], en.bes[1], en.bes[0]], en.addr + en.addr[:1], en.meta + en.meta[:1], en.offs + en.offs[:1],
                 2, "again")
        n = B.MANY_MAX + 1
        with pytest.raises(B.GGError) as ei:
            B.coherent_run_many([en.bes[0]] * n, [en.addr[0]] * n, [en.meta[0]] * n, [en.offs[0]] * n)
        assert ei.value.code == GG_ERR_INVALID and "GG_MANY_MAX" in str(ei.value)
        assert en.run() == [0, 0]                            # the same contexts, now a valid set
        for i, s in enumerate((base, other)):
            _same(en.result(i), _oracle(s), "instance %d after the rejections" % i)
    finally:
        en.close()
        extra.close()
