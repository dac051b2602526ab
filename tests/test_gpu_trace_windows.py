"""A coherent run fed its trace in windows (gg_coherent_begin_window /
_next_window / _window_state).

A windowed run over pieces of a trace must equal gg_coherent_run over the
whole trace, which the oracle pins: every comparison here is word for word.
The whole runs (quantum_ns = 100, so that a window is about a hundred records)
are computed once per case, go through the oracle comparison first, and are
shared read-only."""
import functools
import os
import subprocess

import numpy as np
import pytest

from graphite_amd import config as C
from tests.gpu_util import torch_dev, to_dev, to_np
from tests.test_gpu_checkpoint import HBH, HC, MAGIC, FINAL, _ro, _state, _same, _with_barriers

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REPLAY = os.path.join(ROOT, "graphite_amd", "host", "gg_replay")
ERR_INVALID, ERR_UNSUPPORTED, ERR_STATE = -1, -3, -5
NEED = 3                                   # GG_ADV_NEED_WINDOW
QNS = 100

# the checkpoint tests' shapes: (tiles, records per tile, shards, network, protocol)
CASES = {
    "hbh_mosi_16x4": (16, 400, 4, HBH, C.PROTO_MOSI),
    "hbh_msi_64x8": (64, 300, 8, HBH, C.PROTO_MSI),
    "hc_msi_16x1": (16, 400, 1, HC, C.PROTO_MSI),
    "hbh_shl2_mesi_16x4": (16, 400, 4, HBH, C.PROTO_SHL2_MESI),
    "magic_shl2_msi_16": (16, 400, 1, MAGIC, C.PROTO_SHL2_MSI),
}


@functools.lru_cache(maxsize=None)
def case(name, **over):
    from oracle import pyoracle as po
    T, N, K, net, proto = CASES[name]
    cfg = C.default_config(T, num_shards=K, net_model=net, protocol=proto, quantum_ns=QNS, **over)
    a, m, o = _ro(*po.gen_trace(T, N))
    return cfg, a, m, o


def _whole(cfg, a, m, o, prepare=None):
    """gg_coherent_run over the whole trace: the backend and its state."""
    torch = torch_dev()
    from graphite_amd import backend as B
    be = B.Backend(cfg)
    if prepare:
        prepare(be)
    addr = to_dev(torch, np.array(a), torch.int64)
    meta = to_dev(torch, np.array(m), torch.int32)
    out = torch.zeros(len(a), dtype=torch.int64, device="cuda")
    be.coherent_run(addr, meta, o, out)
    return be, _state(be, out)


@functools.lru_cache(maxsize=None)
def reference(name):
    """The run without windows under the same config, against the oracle."""
    cfg, a, m, o = case(name)
    if cfg.protocol in (C.PROTO_SHL2_MSI, C.PROTO_SHL2_MESI):
        from tests.test_gpu_shl2 import _compare
    else:
        from tests.coherent_util import _compare
    g = _compare(cfg, np.array(a), np.array(m), np.array(o))
    be, w = _whole(cfg, a, m, o)
    be.close()
    _same(w[:4] + [w[5]], list(g[:4]) + [g[4]], "the whole run twice: ")
    _ro(*w)
    return w


def _timed(m):
    """Records that start only before the lax barrier: no CONT line, no BARRIER."""
    m = np.asarray(m, np.uint32)
    return (m != np.uint32(C.META_BARRIER)) & ((m & np.uint32(0x80000000)) == 0)


class Windowed:
    """Drives a windowed run of the trace (a, m, o).  size(t, need) -> the
    records of tile t's next window counted up to its last timed record
    (>= need, gg_coherent_window_state's min_records); tail: up to this many
    CONT lines / BARRIER records that follow are put into the window too, so
    that windows end inside a multi-line access or behind a barrier."""

    def __init__(self, cfg, a, m, o, size, tail=0, whole_tiles=(), prepare=None, first=1):
        torch = torch_dev()
        from graphite_amd import backend as B
        self.torch = torch
        self.cfg, self.size, self.tail = cfg, size, tail
        self.a, self.m = np.asarray(a, np.uint64), np.asarray(m, np.uint32)
        self.o = np.asarray(o, np.int64)
        self.T = len(self.o) - 1
        self.timed = _timed(self.m)
        self.whole = set(whole_tiles)
        self.words = np.zeros(len(self.a), np.uint64)
        self.consumed = np.zeros(self.T, np.int64)
        self.handovers = 0
        self.ends = {"timed": 0, "cont": 0, "barrier": 0, "first_line": 0}
        self.max_need = 0
        self.be = B.Backend(cfg)
        if prepare:
            prepare(self.be)
        self.final = np.zeros(self.T, bool)                # a final tile stays final: its whole rest every time
        self.cur = self._make(np.full(self.T, first, np.int64), count=False)
        self.be.coherent_begin_window(*self.cur[:4], final_tiles=self.cur[4])
        self.final = self.cur[4].astype(bool)

    def _make(self, need, count=True):
        lo, hi, fin = np.zeros(self.T, np.int64), np.zeros(self.T, np.int64), np.zeros(self.T, np.uint8)
        for t in range(self.T):
            s, end = int(self.o[t] + self.consumed[t]), int(self.o[t + 1])
            want = end - s if t in self.whole or self.final[t] else max(int(self.size(t, int(need[t]))), int(need[t]), 1)
            e = min(s + want, end)
            while e < end and not self.timed[e - 1]:      # up to a timed record: it is what min_records counts to
                e += 1
            for _ in range(self.tail):                     # then into the access / behind the barrier that follows
                if e < end and not self.timed[e]:
                    e += 1
            lo[t], hi[t], fin[t] = s, e, e == end
            if count and not fin[t]:
                last = self.m[e - 1]
                kind = "barrier" if last == np.uint32(C.META_BARRIER) else "cont" if not self.timed[e - 1] else \
                    "first_line" if not self.timed[e] and self.m[e] != np.uint32(C.META_BARRIER) else "timed"
                self.ends[kind] += 1
        idx = np.concatenate([np.arange(lo[t], hi[t]) for t in range(self.T)]) if self.T else np.zeros(0, np.int64)
        woffs = np.concatenate([[0], np.cumsum(hi - lo)]).astype(np.uint64)
        torch = self.torch
        addr = to_dev(torch, self.a[idx], torch.int64)
        meta = to_dev(torch, self.m[idx], torch.int32)
        out = torch.zeros(len(idx), dtype=torch.int64, device="cuda")
        return addr, meta, woffs, out, fin, lo

    def gather(self):
        """The access words of the records consumed since the last gather, out
        of the buffer that was bound while they were consumed."""
        c, need = self.be.coherent_window_state()
        c = c.astype(np.int64)
        w = to_np(self.cur[3], np.uint64)
        woffs, lo = self.cur[2].astype(np.int64), self.cur[5]
        for t in range(self.T):
            k0, k1 = int(self.o[t] + self.consumed[t]), int(self.o[t] + c[t])
            assert lo[t] == k0 or k1 == k0
            self.words[k0:k1] = w[woffs[t]:woffs[t] + (k1 - k0)]
        self.consumed = c
        return need.astype(np.int64)

    def hand_over(self):
        need = self.gather()
        self.max_need = max(self.max_need, int(need.max()))
        nxt = self._make(need)
        self.be.coherent_next_window(*nxt[:4], final_tiles=nxt[4])
        self.cur = nxt
        self.final = nxt[4].astype(bool)
        self.handovers += 1

    def run(self, limit=4000):
        while True:
            nq, done = self.be.coherent_advance()
            if done == 1:
                break
            assert done == NEED, done
            self.hand_over()
            assert self.handovers < limit, "no end in %d hand-overs" % limit
        self.gather()
        assert np.array_equal(self.consumed, np.diff(self.o))
        return self

    def state(self):
        st = _state(self.be, self.cur[3])
        st[0] = self.words.copy()
        return st


# ---- 1. windowed == whole == oracle ---------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(CASES))
def test_windowed_equals_whole(name):
    cfg, a, m, o = case(name)
    ref = reference(name)
    # min_records + 8 after a first window of one record: min_records is 2 + the
    # records of the time to the next barrier at 1 ns each, about 110 of a
    # tile's 300 / 400 records while it keeps up with the barrier (a tile that
    # fell behind gets more at once); the count is printed and asserted
    w = Windowed(cfg, a, m, o, lambda t, need: need + 8).run()
    got = w.state()
    w.be.close()
    print(name, "hand-overs", w.handovers, "largest min_records", w.max_need, "final quantum", int(ref[5][FINAL]))
    assert w.handovers >= 3
    _same(got, ref, "%s in windows: " % name)


@pytest.mark.gpu
def test_miss_types_in_windows():
    name = "hbh_mosi_16x4"
    over = dict(l1d_track_miss_types=1, l2_track_miss_types=1, miss_track_lines=1024)
    cfg, a, m, o = case(name, **over)
    be, ref = _whole(cfg, a, m, o)
    mt = be.miss_types()
    be.close()
    assert mt.sum() > 0
    w = Windowed(cfg, a, m, o, lambda t, need: need + 8).run()
    got, mg = w.state(), w.be.miss_types()
    w.be.close()
    assert w.handovers >= 3
    _same(got, ref, "miss-type tracking on, in windows: ")
    assert np.array_equal(mg, mt)


@pytest.mark.gpu
def test_statistics_trace_in_windows():
    cfg, a, m, o = case("hbh_mosi_16x4")
    prep = lambda be: be.stats_trace_configure(3, 4 * cfg.quantum_ns, 4096)
    be, ref = _whole(cfg, a, m, o, prepare=prep)
    tr = be.stats_trace()
    be.close()
    w = Windowed(cfg, a, m, o, lambda t, need: need + 8, prepare=prep).run()
    got, tg = w.state(), w.be.stats_trace()
    w.be.close()
    assert w.handovers >= 3 and len(tr["time_ns"]) > 10
    _same(got, ref, "statistics trace on, in windows: ")
    assert sorted(tg) == sorted(tr)
    for k in tr:
        assert np.array_equal(tg[k], tr[k]), "statistics trace field %s differs in windows" % k


# ---- 2. the cut points do not matter -----------------------------------------------
@pytest.mark.gpu
def test_cut_points_do_not_matter():
    cfg, a, m, o = case("hbh_mosi_16x4")
    ref = reference("hbh_mosi_16x4")
    sizes = {
        "min + 1": lambda t, need: need + 1,
        "min + 57": lambda t, need: need + 57,
        "per tile": lambda t, need: need + 3 + 29 * (t % 5),
    }
    for what, size in sizes.items():
        w = Windowed(cfg, a, m, o, size, whole_tiles=(5,)).run()      # tile 5: its whole trace, final from the start
        got = w.state()
        w.be.close()
        print(what, "hand-overs", w.handovers)
        assert w.handovers >= 3
        _same(got, ref, "windows of %s: " % what)


# ---- 3. BARRIER records and multi-line accesses ---------------------------------------
def _split_trace(T, N):
    """Accesses of 2-5 lines through gg_split_accesses (as tests/test_access_split.py)."""
    torch = torch_dev()
    from graphite_amd import backend as B
    from oracle import pyoracle as po
    rng = np.random.default_rng(11)
    a, m, offs = po.gen_trace(T, N, hot_lines=16)
    a = a + rng.integers(0, 64, len(a)).astype(np.uint64)
    lines = rng.integers(2, 6, len(a))
    size = ((lines - 1) * 64 + 1).astype(np.uint32)          # from any byte of a line: exactly `lines` lines
    la, lm, first, lo = B.split_accesses(to_dev(torch, a, torch.int64), to_dev(torch, size, torch.int32),
                                         to_dev(torch, m, torch.int32), offs, 64)
    return to_np(la, np.uint64), to_np(lm, np.uint32), np.asarray(lo, np.uint64)


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["barriers", "multi_line"])
def test_barriers_and_multi_line_accesses(kind):
    from oracle import pyoracle as po
    T, K = 16, 4
    cfg = C.default_config(T, num_shards=K, net_model=HBH, protocol=C.PROTO_MSI, quantum_ns=QNS)
    if kind == "barriers":
        a, m, o = _with_barriers(*po.gen_trace(T, 360), 7)
        # pairs of BARRIER records: a window that ends between the two ends inside a barrier run
        a, m, o = _with_barriers(a, m, o, 8)
    else:
        a, m, o = _split_trace(T, 120)
        assert ((m & np.uint32(0x80000000)) != 0).sum() > T * 120
    be, ref = _whole(cfg, a, m, o)
    be.close()
    for tail in (0, 1, 2):
        w = Windowed(cfg, a, m, o, lambda t, need: need + 2 + t % 3, tail=tail).run()
        got = w.state()
        w.be.close()
        print(kind, "tail", tail, "hand-overs", w.handovers, "window ends", w.ends)
        assert w.handovers >= 3
        if tail:
            assert w.ends["barrier" if kind == "barriers" else "cont"] > 0
        elif kind == "multi_line":
            assert w.ends["first_line"] > 0
        _same(got, ref, "%s, windows with %d records behind the last timed one: " % (kind, tail))


# ---- 4. the densest trace: every record an L1-D hit with gap 0 ------------------------------
def _dense(T, N, miss_at=None):
    a = np.repeat((np.arange(T, dtype=np.uint64) + np.uint64(1)) << np.uint64(16), N)
    m = np.zeros(T * N, np.uint32)
    o = (np.arange(T + 1) * N).astype(np.uint64)
    if miss_at is not None:
        # tile 0 writes a line every other tile has read: invalidations across
        # the shards, quanta pass while its clock stands, then hits again
        shared = np.uint64(1) << np.uint64(30)
        for t in range(1, T):
            a[t * N + 1] = shared
        a[miss_at] = shared
        m[miss_at] = 1
    return a, m, o


@pytest.mark.gpu
@pytest.mark.parametrize("variant", ["all_hits", "one_tile_behind"])
def test_densest_trace_exact_windows(variant):
    T, N, K = 16, 600, 4
    cfg = C.default_config(T, num_shards=K, net_model=HBH, protocol=C.PROTO_MSI, quantum_ns=QNS)
    a, m, o = _dense(T, N, miss_at=150 if variant == "one_tile_behind" else None)
    be, ref = _whole(cfg, a, m, o)
    be.close()
    hits = int(((ref[0] & np.uint64(3)) == C.LVL_L1).sum())
    assert hits >= T * N - 3 * T
    w = Windowed(cfg, a, m, o, lambda t, need: need).run()           # exactly min_records: GG_ERR_STATE if the horizon is wrong
    got = w.state()
    w.be.close()
    hit_ps = cfg.l1d_data_cycles * 1000.0 / cfg.frequency_ghz         # the L1-D hit path
    per_quantum = int(cfg.quantum_ns * 1000 // hit_ps)                # records of one quantum at that pace
    print(variant, "hand-overs", w.handovers, "largest min_records", w.max_need, "records per quantum", per_quantum)
    assert w.handovers >= 3
    if variant == "one_tile_behind":
        assert w.max_need > 2 * per_quantum, "no tile was ever more than a quantum behind the barrier"
    _same(got, ref, "%s in windows of exactly min_records: " % variant)


# ---- 5. the rules --------------------------------------------------------------------------
def _raises(code, fn, *args, **kw):
    from graphite_amd import backend as B
    with pytest.raises(B.GGError) as e:
        fn(*args, **kw)
    assert e.value.code == code, (e.value.code, str(e.value))
    return str(e.value)


@pytest.mark.gpu
def test_rules_and_refusals():
    from graphite_amd import backend as B
    name = "hbh_mosi_16x4"
    cfg, a, m, o = case(name)
    ref = reference(name)
    w = Windowed(cfg, a, m, o, lambda t, need: need + 8)
    be = w.be
    # windows of one record are too short: min_records says so, advance asks at once, with no launch
    c0, need0 = be.coherent_window_state()
    hit_ps = cfg.l1d_data_cycles * 1000.0 / cfg.frequency_ghz
    assert not c0.any() and (need0 >= 2 + int(cfg.quantum_ns * 1000 // hit_ps)).all()
    assert be.coherent_advance() == (0, NEED)
    assert be.coherent_advance(5) == (0, NEED)
    assert be.coherent_advance(0) == (0, 0)                          # stop <= current: as ever
    st, cc, ri = be.coherent_stats()
    assert int(ri[C.RUN_INFO.index("steps")]) == 0 and not st.any()
    # the refusals on a windowed run
    _raises(ERR_UNSUPPORTED, be.coherent_snapshot_size)
    _raises(ERR_UNSUPPORTED, be.coherent_snapshot, 1 << 20)
    _raises(ERR_UNSUPPORTED, B.coherent_advance_many, [be])
    _raises(ERR_INVALID, be.coherent_quantum, 0)
    # the round, split at its transport: refused before anything is enqueued
    assert "fed in windows" in _raises(ERR_INVALID, be.round_pack, 1, 0, 0)
    io = B.RoundIO()
    _raises(ERR_INVALID, be.round_unpack, io)
    _raises(ERR_INVALID, be.round_finish, io)
    torch = w.torch
    full = (to_dev(torch, w.a, torch.int64), to_dev(torch, w.m, torch.int32), np.asarray(o, np.uint64))
    _raises(ERR_UNSUPPORTED, B.coherent_run_many, [be], [full[0]], [full[1]], [full[2]])
    words = torch.zeros(len(w.a), dtype=torch.int64, device="cuda")
    _raises(ERR_UNSUPPORTED, be.core_model_run, full[1], full[2], words)
    w.hand_over()
    # some quanta in, then the hand-overs that must be refused with nothing changed
    nq, done = be.coherent_advance(3)
    while done == NEED:
        w.hand_over()
        nq, done = be.coherent_advance(3)
    assert done == 0 and nq >= 3
    need = w.gather()

    def changed(field, t):
        addr, meta, woffs, out, fin, lo = w._make(need, count=False)
        x = (addr if field == "addr" else meta).clone()
        x[int(woffs[t])] ^= 64 if field == "addr" else 1
        return (x, meta, woffs, out) if field == "addr" else (addr, x, woffs, out), fin

    blocked = int(np.argmax(be.coherent_window_state()[0]))           # any tile: each stands on a record
    for field in ("addr", "meta"):
        args, fin = changed(field, blocked)
        assert "first record" in _raises(ERR_INVALID, be.coherent_next_window, *args, final_tiles=fin)
    # a final tile made non-final: tile 3 is handed its whole rest and marked final, then not
    rest = Windowed.__new__(Windowed)
    rest.__dict__.update(w.__dict__)
    rest.whole = {3}
    fin_win = rest._make(need, count=False)
    assert fin_win[4][3] == 1
    be.coherent_next_window(*fin_win[:4], final_tiles=fin_win[4])
    w.cur = fin_win
    w.final = fin_win[4].astype(bool)
    w.handovers += 1
    need = w.gather()
    w.final[3] = False
    back = w._make(need, count=False)                                 # tile 3 not final again, with fewer records
    w.final[3] = True
    assert back[4][3] == 0
    assert "final" in _raises(ERR_INVALID, be.coherent_next_window, *back[:4], final_tiles=back[4])
    fin_cleared = fin_win[4].copy()                                   # and its whole rest with the flag cleared
    fin_cleared[3] = 0
    assert "final" in _raises(ERR_INVALID, be.coherent_next_window, *fin_win[:4], final_tiles=fin_cleared)
    w.whole = {3}
    # every refusal left the state as it was: on to the right result
    w.run()
    got = w.state()
    _same(got, ref, "after refused hand-overs: ")
    # the run is over: no clean point for a window any more
    assert "clean point" in _raises(ERR_INVALID, be.coherent_next_window, *w.cur[:4], final_tiles=w.cur[4])
    # a run that is not windowed
    addr, meta, offs = full
    be.coherent_begin(addr, meta, offs, words)
    _raises(ERR_INVALID, be.coherent_next_window, addr, meta, offs, words)
    _raises(ERR_INVALID, be.coherent_window_state)
    nq, done = be.coherent_advance()
    assert done == 1                                                  # and an ordinary run never sees NEED
    be.close()


@pytest.mark.gpu
def test_zero_cycle_l1d_and_bad_first_windows():
    from graphite_amd import backend as B
    torch = torch_dev()
    cfg, a, m, o = case("hc_msi_16x1")
    addr = to_dev(torch, np.array(a), torch.int64)
    meta = to_dev(torch, np.array(m), torch.int32)
    offs = np.asarray(o, np.uint64)
    be = B.Backend(C.default_config(16, num_shards=1, net_model=HC, protocol=C.PROTO_MSI, quantum_ns=QNS,
                                    l1d_data_cycles=0))
    assert "L1-D" in _raises(ERR_UNSUPPORTED, be.coherent_begin_window, addr, meta, offs)
    be.close()
    be = B.Backend(cfg)
    empty = offs.copy()
    empty[4:] -= offs[4] - offs[3]                                    # tile 3: no record, not final
    n = int(empty[-1])
    _raises(ERR_INVALID, be.coherent_begin_window, addr[:n].contiguous(), meta[:n].contiguous(), empty)
    be.close()
    # a context that does not own every shard
    part = C.default_config(16, num_shards=4, net_model=HBH, protocol=C.PROTO_MSI, quantum_ns=QNS,
                            shard_begin=0, shard_end=2)
    be = B.Backend(part)
    _raises(ERR_UNSUPPORTED, be.coherent_begin_window, addr, meta, offs)
    be.close()


@pytest.mark.gpu
def test_atac_context_is_refused():
    """The coherent mode refuses an ATAC context everywhere; the window entries too."""
    from graphite_amd import backend as B
    torch = torch_dev()
    be = B.Backend(C.default_config(64, net_model=C.NET_ATAC))
    addr = torch.zeros(64, dtype=torch.int64, device="cuda")
    meta = torch.zeros(64, dtype=torch.int32, device="cuda")
    offs = np.arange(65, dtype=np.uint64)
    for call in (lambda: be.coherent_begin_window(addr, meta, offs), lambda: be.coherent_next_window(addr, meta, offs),
                 lambda: be.coherent_window_state()):
        with pytest.raises(B.GGError, match="batch API only") as e:
            call()
        assert e.value.code == ERR_UNSUPPORTED
    be.close()


@pytest.mark.gpu
def test_backstop_status_through_the_host_path(monkeypatch):
    """A tile off a window that is not the end of its trace sets GG_DERR_WINDOW
    at the quantum end.  No tile is driven there (a reachable case would be a
    bug in the rule): the test knob GG_WINDOW_FAIL_EXHAUSTED sets that bit from
    the host on a paused run, and the run must end as the backstop promises —
    GG_ERR_STATE "window exhausted", never done = 1, no further hand-over."""
    import ctypes
    from graphite_amd import backend as B
    cfg, a, m, o = case("hbh_mosi_16x4")
    w = Windowed(cfg, a, m, o, lambda t, need: need + 8)
    be = w.be
    assert be.coherent_advance()[1] == NEED
    w.hand_over()
    nq, done = be.coherent_advance(3)
    while done == NEED:
        w.hand_over()
        nq, done = be.coherent_advance(3)
    assert done == 0
    monkeypatch.setenv("GG_WINDOW_FAIL_EXHAUSTED", "1")
    for stop in (B.Backend.NEVER, nq + 1, nq):                       # a launch path and the at-once path
        q, d = ctypes.c_uint64(0), ctypes.c_int(-1)
        rc = B.load().gg_coherent_advance(be.h, stop, ctypes.byref(q), ctypes.byref(d))
        assert rc == ERR_STATE and d.value != 1, (rc, d.value)
        assert "window exhausted" in B.load().gg_last_error().decode()
    monkeypatch.delenv("GG_WINDOW_FAIL_EXHAUSTED")
    assert "window exhausted" in _raises(ERR_STATE, be.coherent_advance)          # the run stays failed
    need = w.gather()
    nxt = w._make(need, count=False)
    assert "clean point" in _raises(ERR_INVALID, be.coherent_next_window, *nxt[:4], final_tiles=nxt[4])
    be.close()


# ---- 6. gg_replay --window ---------------------------------------------------------------------
@pytest.mark.gpu
def test_replay_window_prints_the_same():
    base = [REPLAY, "--coherent", "--tiles", "16", "--per-tile", "3000", "--net", "hop_by_hop", "--shards", "4"]
    whole = subprocess.run(base, capture_output=True, text=True, timeout=120)
    assert whole.returncode == 0, whole.stderr
    for recs in ("1", "700"):
        win = subprocess.run(base + ["--window", recs], capture_output=True, text=True, timeout=120)
        assert win.returncode == 0, win.stderr
        print(win.stderr.strip())
        assert "windows handed over" in win.stderr
        assert win.stdout == whole.stdout and len(whole.stdout) > 1000
