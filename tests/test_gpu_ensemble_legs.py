"""gg_coherent_advance_many / backend.coherent_advance_many: an ensemble in
legs, and with statistics traces.  Every context has a begun run; one call
drives all of them in one set of launches, each to its own stop quantum
(k_c_step_many / k_c_walk_many as gg_coherent_run_many, plus k_stats_scan_many
after every slot while a live instance has a trace).  For one instance the
call must be indistinguishable from gg_coherent_advance on a lone context:
every comparison here is word for word — access words, tile stats, cache
counters, NoC counters, run info, miss types and protocol stats where they
matter, samples with their time_ns, repeat and histogram — against
oracle.pyoracle.OracleCoherent, against a twin context driven alone, or both.

The helpers are those of tests/test_gpu_ensemble.py (copied: that file stays
as it is), with a gap on every tile's middle record and a statistics trace per
instance added.  The CPU tests need no GPU and fail without the feature."""
import ctypes
import functools

import numpy as np
import pytest

from graphite_amd import backend as B
from graphite_amd import config as C
from tests.gpu_util import torch_dev, to_dev, to_np

HBH, HC = C.NET_EMESH_HOP_BY_HOP, C.NET_EMESH_HOP_COUNTER
MSI, MOSI = C.PROTO_MSI, C.PROTO_MOSI
GG_ERR_INVALID, GG_ERR_UNSUPPORTED = -1, -3
ST_NET, ST_REPL = B.ST_NETWORK_UTILIZATION, B.ST_CACHE_LINE_REPLICATION
NAMES = ("access words", "tile stats", "cache counters", "noc counters", "run info", "miss types", "protocol stats")
ALL = len(NAMES)


# ---- instances: (config, trace) specs, hashable so the oracle runs once ----
def _spec(T, K, net, per_tile, protocol=MSI, barriers=0, gap=0, trace=(), cfg=()):
    return (T, K, net, per_tile, protocol, barriers, gap, tuple(sorted(dict(trace).items())),
            tuple(sorted(dict(cfg).items())))


def _cfg(spec):
    T, K, net, _, protocol, _, _, _, cfg = spec
    return C.default_config(T, num_shards=K, net_model=net, protocol=protocol, **dict(cfg))


def _with_barriers(a, m, offs, every):
    """A BARRIER record after every `every` accesses of each tile."""
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
    T, _, _, per_tile, _, barriers, gap, trace, _ = spec
    a, m, o = po.gen_trace(T, per_tile, **dict(trace))
    if gap:
        # every tile's middle record waits `gap` cycles: all tiles idle at once,
        # the run skips empty quanta (tests/test_stats_trace.py, "skipped_boundaries")
        m = m.copy()
        mid = o[:-1].astype(np.int64) + per_tile // 2
        m[mid] = (np.uint32(gap) << np.uint32(1)) | (m[mid] & np.uint32(1))
    r = (a, m, o)
    if barriers:
        r = _with_barriers(a, m, o, barriers)
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


def _final_quantum(spec):
    return int(_oracle(spec)[4][C.RUN_INFO.index("final_quantum")])


def _max_samples(spec, st):
    """Room for every sample of the run (st = (bits, interval in quanta))."""
    return _final_quantum(spec) // st[1] + 8


class _Ensemble:
    """Contexts, device traces and output buffers of a list of specs.
    stats[i]: None, or (GG_ST_* bits, interval in quanta[, max_samples]) of
    instance i's statistics trace."""

    def __init__(self, torch, specs, stats=None):
        self.torch, self.specs = torch, list(specs)
        self.bes = [B.Backend(_cfg(s)) for s in self.specs]
        self.addr, self.meta, self.offs, self.outs = [], [], [], []
        for i, s in enumerate(self.specs):
            a, m, o = _trace(s)
            self.addr.append(to_dev(torch, np.array(a), torch.int64))
            self.meta.append(to_dev(torch, np.array(m), torch.int32))
            self.offs.append(o)
            self.outs.append(torch.zeros(len(a), dtype=torch.int64, device="cuda"))
            st = stats[i] if stats else None
            if st:
                self.bes[i].stats_trace_configure(st[0], st[1] * self.bes[i].cfg.quantum_ns,
                                                  st[2] if len(st) > 2 else _max_samples(s, st))

    def begin(self, order=None):
        for i in (range(len(self.specs)) if order is None else order):
            self.outs[i].zero_()
            self.bes[i].coherent_begin(self.addr[i], self.meta[i], self.offs[i], self.outs[i])

    def advance(self, stops=None, order=None):
        """coherent_advance_many over the instances `order` (default: all);
        stops follow `order`."""
        ix = list(range(len(self.specs))) if order is None else list(order)
        r = B.coherent_advance_many([self.bes[i] for i in ix], stops)
        self.torch.cuda.synchronize()
        return r

    def lone_advance(self, i, stop=None):
        r = self.bes[i].coherent_advance(B.Backend.NEVER if stop is None else stop)
        self.torch.cuda.synchronize()
        return r

    def run_many(self):
        for o in self.outs:
            o.zero_()
        st = B.coherent_run_many(self.bes, self.addr, self.meta, self.offs, self.outs)
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
            if be is not None:
                be.close()


def _same(got, ref, what, upto=5):
    for name, x, y in zip(NAMES, got[:upto], ref[:upto]):
        if not np.array_equal(x, y):
            d = np.argwhere(np.asarray(x) != np.asarray(y))
            raise AssertionError("%s: %s differ at %d places, first %s: %s vs %s"
                                 % (what, name, len(d), d[0], np.asarray(x)[tuple(d[0])], np.asarray(y)[tuple(d[0])]))


def _same_samples(got, ref, what, upto=None):
    """Two stats_trace() results: count, every field, the histogram (ref cut
    to its first `upto` samples)."""
    n = len(ref["time_ns"]) if upto is None else upto
    assert len(got["time_ns"]) == n, "%s: %d samples, expected %d" % (what, len(got["time_ns"]), n)
    for k in B.ST_FIELDS + ["sharer_hist"]:
        if not np.array_equal(got[k], ref[k][:n]):
            d = np.argwhere(got[k] != ref[k][:n])
            raise AssertionError("%s: %s differ at %d places, first at %s: %s vs %s"
                                 % (what, k, len(d), d[0], got[k][tuple(d[0])], ref[k][:n][tuple(d[0])]))


# ---- 1. whole runs ------------------------------------------------------------
@pytest.mark.gpu
def test_whole_runs():
    """begin per context, then coherent_advance_many() with no stops: three
    instances of 200, 290 and 350 records per tile, each over and exact."""
    specs = [_spec(16, 1, HC, 200, trace=dict(hot_lines=8)),
             _spec(16, 1, HC, 290, trace=dict(hot_lines=16, hot_frac256=90)),
             _spec(16, 1, HC, 350, trace=dict(hot_lines=64, lines_log2=12))]
    torch = torch_dev()
    en = _Ensemble(torch, specs)
    try:
        en.begin()
        r = en.advance()
        assert [d for _, d in r] == [1, 1, 1], r
        for i, s in enumerate(specs):
            assert r[i][0] == _final_quantum(s) + 1
            _same(en.result(i), _oracle(s), "instance %d vs oracle" % i)
    finally:
        en.close()


# ---- 2. different stops, uneven lengths --------------------------------------
UNEVEN = [_spec(16, 1, HC, 50, trace=dict(hot_lines=8)),
          _spec(16, 1, HC, 400, trace=dict(hot_lines=16, hot_frac256=90)),
          _spec(16, 1, HC, 1500, trace=dict(hot_lines=32, lines_log2=12))]


@pytest.mark.gpu
def test_different_stops_and_uneven_lengths():
    """50, 400 and 1 500 records per tile in three legs, the stops at one third
    and two thirds of each instance's own final quantum; after every call
    (next, done) of every instance equals that of a twin context driven alone
    by coherent_advance with the same stop, and the final states equal the
    oracle.  Under those stops the short instance pauses like the others, so
    the same contexts then run a second time with the short one unstopped: it
    is over after the first leg and sits in the later calls as a no-op whose
    getters do not change."""
    torch = torch_dev()
    en, tw = _Ensemble(torch, UNEVEN), _Ensemble(torch, UNEVEN)
    fq = [_final_quantum(s) for s in UNEVEN]
    assert all(f >= 6 for f in fq), fq
    thirds = [[f // 3 for f in fq], [2 * f // 3 for f in fq], [None] * 3]
    try:
        for short_unstopped in (False, True):
            en.begin()
            tw.begin()
            short = None
            for leg, st in enumerate(thirds):
                stops = list(st)
                if short_unstopped and leg == 0:
                    stops[0] = None
                r = en.advance(stops)
                for i in range(3):
                    assert r[i] == tw.lone_advance(i, stops[i]), "leg %d, instance %d: %s" % (leg, i, r[i])
                if short_unstopped:
                    assert r[0] == (fq[0] + 1, 1)            # over after the first leg, a no-op afterwards
                    now = en.result(0)
                    if short is not None:
                        _same(now, short, "the finished instance after leg %d" % leg, ALL)
                    short = now
                elif leg < 2:
                    assert [d for _, d in r] == [0, 0, 0], r
                    assert all(q >= s for (q, _), s in zip(r, stops)), (r, stops)
            assert [d for _, d in r] == [1, 1, 1], r
            for i, s in enumerate(UNEVEN):
                _same(en.result(i), _oracle(s), "instance %d vs oracle" % i)
                _same(tw.result(i), _oracle(s), "twin %d vs oracle" % i)
    finally:
        en.close()
        tw.close()


# ---- 3. hop-by-hop across shards, through the host -----------------------------
@pytest.mark.gpu
def test_hop_by_hop_snapshot_restore():
    """T=64, K=8, two instances that differ in dram_latency_ns and
    router_delay, both paused mid-run in one call.  Each snapshot is byte for
    byte that of a lone context paused at the same quantum; the contexts are
    closed, the blobs restored into fresh ones, and coherent_advance_many runs
    those to the end: the oracle's results."""
    specs = [_spec(64, 8, HBH, 200, trace=dict(hot_lines=32)),
             _spec(64, 8, HBH, 260, trace=dict(hot_lines=16, hot_frac256=80),
                   cfg=dict(dram_latency_ns=60, router_delay=2))]
    torch = torch_dev()
    en, lone = _Ensemble(torch, specs), _Ensemble(torch, specs)
    fresh = []
    try:
        stops = [_final_quantum(s) // 2 for s in specs]
        en.begin()
        r = en.advance(stops)
        assert [d for _, d in r] == [0, 0] and all(q >= s for (q, _), s in zip(r, stops)), r
        blobs = [be.coherent_snapshot().copy() for be in en.bes]
        lone.begin()
        for i in range(2):
            assert lone.lone_advance(i, stops[i]) == r[i]
            b = lone.bes[i].coherent_snapshot()
            assert b.size == blobs[i].size and np.array_equal(b, blobs[i]), "instance %d: snapshot bytes" % i
        for i in range(2):
            en.bes[i].close()
            en.bes[i] = None
        fresh = [B.Backend(_cfg(s)) for s in specs]
        for i, be in enumerate(fresh):
            be.coherent_restore(blobs[i], en.addr[i], en.meta[i], en.offs[i], en.outs[i])   # (the buffer is carried across)
        r = B.coherent_advance_many(fresh)
        torch.cuda.synchronize()
        assert [d for _, d in r] == [1, 1], r
        en.bes = fresh
        fresh = []
        for i, s in enumerate(specs):
            _same(en.result(i), _oracle(s), "restored instance %d vs oracle" % i)
    finally:
        en.close()
        lone.close()
        for be in fresh:
            be.close()


# ---- 4. every boundary, BARRIER records -----------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("protocol", [MSI, MOSI])
def test_every_boundary_with_barriers(protocol):
    """Two instances of 120 records per tile with a BARRIER every 30 and every
    50 records, paused at every quantum boundary (stops = next + 1) until both
    are over.  Every BARRIER round of a trace is released across a boundary
    (qend_pick stores the release for the next quantum's step 0), so that many
    pauses carry a pending release.  The pauses per instance equal a lone
    context's, the results the oracle's, BARRIER words carry LVL_SYNC."""
    specs = [_spec(16, 1, HC, 120, protocol, barriers=30, trace=dict(hot_lines=16)),
             _spec(16, 1, HC, 120, protocol, barriers=50, trace=dict(hot_lines=8))]
    rounds = [int((_trace(s)[1] == C.META_BARRIER).sum()) // 16 for s in specs]
    assert rounds == [3, 2], rounds
    torch = torch_dev()
    en, tw = _Ensemble(torch, specs), _Ensemble(torch, specs)
    try:
        en.begin()
        tw.begin()
        lone = []
        for i in range(2):
            nxt, done, k = 0, 0, 0
            while not done:
                nxt, done = tw.lone_advance(i, nxt + 1)
                k += 1 - done
                assert k < 100000
            lone.append(k)
        nxt, pauses, calls = [0, 0], [0, 0], 0
        while True:
            r = en.advance([q + 1 for q in nxt])
            calls += 1
            assert calls < 100000
            for i, (q, d) in enumerate(r):
                assert q > nxt[i] or d == 1
                pauses[i] += 1 - d
                nxt[i] = q
            if all(d == 1 for _, d in r):
                break
        assert pauses == lone, (pauses, lone)
        assert all(p > n for p, n in zip(pauses, rounds)), (pauses, rounds)   # boundaries with a release pending among them
        for i, s in enumerate(specs):
            _same(en.result(i), _oracle(s), "instance %d vs oracle" % i)
            _same(tw.result(i), _oracle(s), "twin %d vs oracle" % i)
            bar = _trace(s)[1] == C.META_BARRIER
            assert np.all((en.result(i)[0][bar] & np.uint64(3)) == C.LVL_SYNC)
    finally:
        en.close()
        tw.close()


# ---- 5. other step variants ------------------------------------------------------
def _pause_once(specs, upto):
    torch = torch_dev()
    en = _Ensemble(torch, specs)
    try:
        en.begin()
        stops = [_final_quantum(s) // 2 for s in specs]
        r = en.advance(stops)
        assert [d for _, d in r] == [0] * len(specs) and all(q >= s for (q, _), s in zip(r, stops)), r
        r = en.advance()
        assert [d for _, d in r] == [1] * len(specs), r
        for i, s in enumerate(specs):
            _same(en.result(i), _oracle(s), "instance %d vs oracle" % i, upto)
        return [en.result(i) for i in range(len(specs))]
    finally:
        en.close()


@pytest.mark.gpu
@pytest.mark.parametrize("protocol", [C.PROTO_SHL2_MSI, C.PROTO_SHL2_MESI])
def test_shared_l2_variants(protocol):
    """pr_l1_sh_l2_msi / _mesi: two instances, T=16, 300 records, one mid-run
    pause; all stats and the protocol stats."""
    specs = [_spec(16, 1, HC, 300, protocol, trace=dict(hot_lines=8)),
             _spec(16, 1, HC, 300, protocol, trace=dict(hot_lines=32, hot_frac256=120))]
    for i, r in enumerate(_pause_once(specs, 5)):
        assert np.array_equal(r[6], _oracle(specs[i])[6]), "instance %d: protocol stats" % i


@pytest.mark.gpu
def test_general_step_variant_with_miss_types():
    """Miss tracking on (the general step variant): one mid-run pause, the
    miss types compared."""
    track = dict(l1i_track_miss_types=1, l2_track_miss_types=1)
    res = _pause_once([_spec(16, 1, HC, 300, trace=dict(hot_lines=32), cfg=track),
                       _spec(16, 1, HC, 450, trace=dict(hot_lines=16, hot_frac256=90), cfg=track)], 6)
    assert all(r[5].sum() > 0 for r in res)


# ---- 6. - 8. statistics traces -------------------------------------------------
# T=16, K=4, hop-by-hop (shards: sent != received per sample).  Instance 0:
# both statistics every 2 quanta, every tile's middle record 1 000 000 cycles
# late (one sample stands for the skipped sampling times: repeat > 1);
# 1: network_utilization every 5 quanta; 2: cache_line_replication every
# quantum on small caches and a 256-entry directory (tests/replication_util.py's
# shape A: replaced entries pending at samples); 3: no trace.
_SMALL = dict(l1d_size_kb=2, l2_size_kb=8, dir_total_entries=256, dir_assoc=4)


def _traced(protocol):
    specs = [_spec(16, 4, HBH, 300, protocol, gap=1000000, trace=dict(hot_lines=8)),
             _spec(16, 4, HBH, 260, protocol, trace=dict(hot_lines=16, hot_frac256=80)),
             _spec(16, 4, HBH, 500, protocol, trace=dict(hot_lines=32), cfg=_SMALL),
             _spec(16, 4, HBH, 200, protocol, trace=dict(hot_lines=64, lines_log2=12))]
    return specs, [(ST_NET | ST_REPL, 2), (ST_NET, 5), (ST_REPL, 1), None]


@functools.lru_cache(maxsize=None)
def _lone_series(protocol):
    """stats_trace() of a lone coherent_run per traced instance, on fresh
    contexts with the same configuration (tests/test_stats_trace.py and
    tests/test_gpu_replication.py pin the lone run to the oracle and the
    reference's rows), with the conditions that make the comparison tell."""
    specs, stats = _traced(protocol)
    torch = torch_dev()
    lone = _Ensemble(torch, specs, stats)
    try:
        out = []
        for i, st in enumerate(stats):
            if not st:
                out.append(None)
                continue
            lone.single(i)
            _same(lone.result(i), _oracle(specs[i]), "lone traced run %d vs oracle" % i)
            out.append(lone.bes[i].stats_trace())
    finally:
        lone.close()
    assert all(len(s["time_ns"]) >= 4 for s in out if s), [len(s["time_ns"]) for s in out if s]
    assert any(int(s["repeat"].max()) > 1 for s in out if s)
    assert int(out[0]["repeat"].max()) > 1
    n = min(len(out[0]["time_ns"]), len(out[1]["time_ns"]))
    assert not np.array_equal(out[0]["flits_sent"][:n], out[1]["flits_sent"][:n])
    for i in (0, 1):
        assert np.any(out[i]["flits_sent"] != out[i]["flits_received"]), i
    assert out[2]["sharer_hist"][:, 1:].sum() > 0
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("protocol", [MSI, MOSI])
def test_statistics_trace_in_an_ensemble(protocol):
    """Four instances in one call — both statistics, network_utilization
    only, cache_line_replication only, no trace; three intervals — each traced
    one with the samples of its lone coherent_run, all with the oracle's
    results; stats_trace() on the untraced one raises as ever."""
    specs, stats = _traced(protocol)
    ref = _lone_series(protocol)
    torch = torch_dev()
    en = _Ensemble(torch, specs, stats)
    try:
        en.begin()
        r = en.advance()
        assert [d for _, d in r] == [1, 1, 1, 1], r
        for i, s in enumerate(specs):
            _same(en.result(i), _oracle(s), "instance %d vs oracle" % i)
            if stats[i]:
                _same_samples(en.bes[i].stats_trace(), ref[i], "instance %d's samples vs its lone run" % i)
        with pytest.raises(B.GGError, match="no statistics trace") as ei:
            en.bes[3].stats_trace()
        assert ei.value.code == GG_ERR_INVALID
    finally:
        en.close()


@pytest.mark.gpu
@pytest.mark.parametrize("protocol", [MSI, MOSI])
@pytest.mark.parametrize("company", [False, True])
def test_trace_and_legs_together(protocol, company):
    """The first instance of the case above, alone and in company, paused
    where a sample is due — at the sample with repeat > 1 among them: the stop
    is its time_ns / quantum_ns, inside the skipped span — and, stepping on a
    quantum at a time, where none is.  After every call the samples so far are
    the lone whole run's up to the barrier time reached (next quantum x
    quantum_ns), time_ns and repeat at the pause boundary included; at the end
    the series is the lone run's."""
    specs, stats = _traced(protocol)
    ref = _lone_series(protocol)[0]
    Q = _cfg(specs[0]).quantum_ns
    k = int(np.argmax(ref["repeat"] > 1))
    assert 1 <= k < len(ref["time_ns"]) - 2                  # samples before and after it
    ix = [0, 1, 3] if company else [0]
    torch = torch_dev()
    en = _Ensemble(torch, [specs[i] for i in ix], [stats[i] for i in ix])
    n = len(ix)
    try:
        def leg(stop):
            nq, done = en.advance([stop] + [None] * (n - 1))[0]
            have = int((ref["time_ns"] <= np.uint64(nq * Q)).sum()) if not done else len(ref["time_ns"])
            _same_samples(en.bes[0].stats_trace(), ref, "samples at next quantum %d" % nq, have)
            return nq, done, have

        en.begin()
        for j in (1, k):                                     # boundaries with a sample due
            nq, done, have = leg(int(ref["time_ns"][j]) // Q)
            assert not done and have == j + 1, (j, nq, done, have)
        assert nq * Q >= int(ref["time_ns"][k]) + (int(ref["repeat"][k]) - 1) * 2 * Q   # (the repeats lie behind)
        quiet = 0
        for _ in range(8):                                   # one quantum at a time: a boundary with none due
            before = have
            nq, done, have = leg(nq + 1)
            assert not done
            quiet += have == before
        assert 1 <= quiet < 8, quiet
        nq, done, have = leg(None)
        assert done == 1 and have == len(ref["time_ns"])
        for j, i in enumerate(ix):
            _same(en.result(j), _oracle(specs[i]), "instance %d vs oracle" % i)
    finally:
        en.close()


@pytest.mark.gpu
def test_full_sample_buffer_is_isolated():
    """Three traced instances, the middle one with max_samples = 2: the call
    raises with that instance's GG_ERR_UNSUPPORTED ("sample buffer"), the
    other two are complete and exact, samples included."""
    specs, stats = _traced(MSI)
    ref = _lone_series(MSI)
    specs, stats = specs[:3], [stats[0], stats[1] + (2,), stats[2]]
    torch = torch_dev()
    en = _Ensemble(torch, specs, stats)
    try:
        en.begin()
        with pytest.raises(B.GGError, match="sample buffer") as ei:
            en.advance()
        assert ei.value.code == GG_ERR_UNSUPPORTED
        assert ei.value.statuses == [0, GG_ERR_UNSUPPORTED, 0]
        assert [ei.value.results[i][1] for i in (0, 2)] == [1, 1]
        for i in (0, 2):
            _same(en.result(i), _oracle(specs[i]), "instance %d vs oracle" % i)
            _same_samples(en.bes[i].stats_trace(), ref[i], "instance %d's samples vs its lone run" % i)
        _same_samples(en.bes[1].stats_trace(), ref[1], "the full buffer's two samples", 2)
    finally:
        en.close()


# ---- 9. rejections ------------------------------------------------------------------
@pytest.mark.gpu
def test_rejections():
    """Each names its index and nothing runs: afterwards the valid contexts,
    begun before the rejected calls, run to the end and equal the oracle."""
    torch = torch_dev()
    base = _spec(16, 2, HBH, 120, trace=dict(hot_lines=8))
    other = _spec(16, 2, HBH, 100, trace=dict(hot_lines=16))
    en = _Ensemble(torch, [base, other])
    odd = {"num_tiles": _spec(64, 2, HBH, 20), "protocol": _spec(16, 2, HBH, 20, MOSI),
           "never begun": _spec(16, 2, HBH, 20, trace=dict(hot_lines=4)),
           "host driven": _spec(16, 2, HBH, 20, trace=dict(hot_lines=2)),
           "own every shard": _spec(16, 2, HBH, 20, cfg=dict(shard_end=1))}
    extra = _Ensemble(torch, list(odd.values()))
    atac = B.Backend(C.default_config(64, net_model=C.NET_ATAC))
    try:
        en.begin()
        names = list(odd)
        extra.begin([names.index(k) for k in names if k != "never begun"])
        extra.bes[names.index("host driven")].coherent_quantum(0)

        def rejected(bes, index, code, *words):
            with pytest.raises(B.GGError) as ei:
                B.coherent_advance_many(bes)
            assert ei.value.code == code, ei.value
            assert "context %d" % index in str(ei.value), ei.value
            for w in words:
                assert w in str(ei.value), ei.value

        x = lambda k: extra.bes[names.index(k)]
        rejected(en.bes + [x("never begun")], 2, GG_ERR_INVALID, "gg_coherent_begin or gg_coherent_restore first")
        rejected(en.bes + [x("host driven")], 2, GG_ERR_INVALID, "driven by gg_coherent_quantum")
        rejected(en.bes + [x("own every shard")], 2, GG_ERR_UNSUPPORTED, "own every shard")
        rejected(en.bes + [x("num_tiles")], 2, GG_ERR_INVALID, "num_tiles")
        rejected(en.bes + [x("protocol")], 2, GG_ERR_INVALID, "protocol")
        rejected(en.bes + [en.bes[0]], 2, GG_ERR_INVALID, "again")
        rejected(en.bes + [atac], 2, GG_ERR_UNSUPPORTED, "batch API only")
        with pytest.raises(B.GGError) as ei:
            B.coherent_advance_many([en.bes[0]] * (B.MANY_MAX + 1))
        assert ei.value.code == GG_ERR_INVALID and "GG_MANY_MAX" in str(ei.value)
        with pytest.raises(ValueError):
            B.coherent_advance_many(en.bes, [1])
        r = en.advance()                                     # the same contexts, now a valid set
        assert [d for _, d in r] == [1, 1], r
        for i, s in enumerate((base, other)):
            _same(en.result(i), _oracle(s), "instance %d after the rejections" % i)
    finally:
        en.close()
        extra.close()
        atac.close()


# ---- 10. company does not matter ----------------------------------------------------
@pytest.mark.gpu
def test_company_does_not_matter():
    """An instance paused and resumed in an ensemble of three equals the same
    instance driven with n = 1 and in reversed order; coherent_run_many on the
    same contexts afterwards still equals the oracle."""
    specs = [_spec(16, 1, HC, 200, trace=dict(hot_lines=8)),
             _spec(16, 1, HC, 290, trace=dict(hot_lines=16, hot_frac256=90)),
             _spec(16, 1, HC, 350, trace=dict(hot_lines=64, lines_log2=12))]
    torch = torch_dev()
    en, alone = _Ensemble(torch, specs), _Ensemble(torch, specs[1:2])
    stop = _final_quantum(specs[1]) // 2
    try:
        alone.begin()
        a1 = alone.advance([stop])[0]
        mid = alone.result(0)
        a2 = alone.advance()[0]
        assert a1[1] == 0 and a2[1] == 1
        for order in ([0, 1, 2], [2, 1, 0]):
            en.begin()
            stops = [None, None, None]
            stops[order.index(1)] = stop
            r = en.advance(stops, order)
            assert r[order.index(1)] == a1 and [r[order.index(i)][1] for i in (0, 2)] == [1, 1], r
            _same(en.result(1), mid, "paused in company (order %s) vs alone" % order, ALL)
            r = en.advance(None, order)
            assert r[order.index(1)] == a2, r
            for i, s in enumerate(specs):
                _same(en.result(i), _oracle(s), "order %s, instance %d vs oracle" % (order, i))
        _same(alone.result(0), _oracle(specs[1]), "alone vs oracle")
        assert en.run_many() == [0, 0, 0]
        for i, s in enumerate(specs):
            _same(en.result(i), _oracle(s), "coherent_run_many afterwards, instance %d" % i)
    finally:
        en.close()
        alone.close()


# ---- CPU: the surface exists (no GPU call).  Last in the file: a process that
# calls into the library before torch has initialised the GPU finds no device
# afterwards, so run alone this file's GPU tests come first. ----------------
def test_symbol_and_binding_exist():
    lib = ctypes.CDLL(B.LIB_PATH)
    assert hasattr(lib, "gg_coherent_advance_many")
    assert "gg_coherent_advance_many" in B.EXPORTS
    assert callable(getattr(B, "coherent_advance_many", None))


def test_n_zero_is_invalid_without_a_gpu():
    L = B.load()
    assert L.gg_coherent_advance_many(None, 0, None, None, None, None, None) == GG_ERR_INVALID
    assert b"n == 0" in L.gg_last_error()
