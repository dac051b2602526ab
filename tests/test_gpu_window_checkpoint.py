"""A windowed coherent run in legs: gg_coherent_window_snapshot /
_window_restore / gg_window_snapshot_state.

A run fed its trace in windows, paused at a quantum boundary, snapshotted,
restored in a fresh context and continued from windows cut anywhere must equal
the uninterrupted whole-trace run, which the oracle pins (reference() of
tests/test_gpu_trace_windows.py): every comparison here is word for word.  The
shapes are the small ones of the window and checkpoint tests."""
import os
import struct
import subprocess

import numpy as np
import pytest

from graphite_amd import config as C
from tests.gpu_util import torch_dev, to_dev, to_np
from tests.test_gpu_checkpoint import HBH, FINAL, _state, _same, _with_barriers, _sections, _section_at
from tests.test_gpu_trace_windows import Windowed, case, reference, CASES, QNS, _whole

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REPLAY = os.path.join(ROOT, "graphite_amd", "host", "gg_replay")
ERR_INVALID, ERR_UNSUPPORTED = -1, -3
NEED = 3                                   # GG_ADV_NEED_WINDOW
QS_DONE, QS_REL = 2, 11                    # words of the snapshot's qs section (gg_coh_dev.h)

GROW = lambda t, need: need + 8            # the first leg's windows
OTHER = lambda t, need: need + 3           # the later legs': another rule, tail 2
ONE = lambda t, need: 1                    # one record: the next advance must ask for windows at once


class Legs(Windowed):
    """Windowed whose gather may be called more than once per window: a pause
    gathers the words, and the same context may go on in the same window."""

    def gather(self):
        c, need = self.be.coherent_window_state()
        c = c.astype(np.int64)
        w = to_np(self.cur[3], np.uint64)
        woffs, lo = self.cur[2].astype(np.int64), self.cur[5]
        for t in range(self.T):
            k0, k1 = int(self.o[t] + self.consumed[t]), int(self.o[t] + c[t])
            assert k1 == k0 or lo[t] <= k0
            at = int(woffs[t]) + (k0 - int(lo[t]))
            assert k1 == k0 or at + (k1 - k0) <= int(woffs[t + 1])
            self.words[k0:k1] = w[at:at + (k1 - k0)]
        self.consumed = c
        return need.astype(np.int64)


def _shell(cfg, a, m, o, consumed, words, size, tail=0, whole_tiles=(), be=None):
    """A Windowed over (a, m, o) that stands where a snapshot says, without a
    run yet: its _make cuts windows from consumed[t]."""
    from graphite_amd import backend as B
    from tests.test_gpu_trace_windows import _timed
    w = Legs.__new__(Legs)
    w.torch = torch_dev()
    w.cfg, w.size, w.tail = cfg, size, tail
    w.a, w.m, w.o = np.asarray(a, np.uint64), np.asarray(m, np.uint32), np.asarray(o, np.int64)
    w.T = len(w.o) - 1
    w.timed = _timed(w.m)
    w.whole = set(whole_tiles)
    w.words = np.array(words, np.uint64)
    w.consumed = np.asarray(consumed, np.int64).copy()
    w.handovers, w.max_need = 0, 0
    w.ends = {"timed": 0, "cont": 0, "barrier": 0, "first_line": 0}
    w.final = np.zeros(w.T, bool)
    w.be = be if be is not None else B.Backend(cfg)
    return w


def _resume(cfg, a, m, o, blob, words, size, tail=0, whole_tiles=(), first=ONE, be=None):
    """A fresh context (no prepare: restore re-establishes the configuration)
    restored from blob with first windows cut by `first` from where the file
    says every tile stands; continues with `size`."""
    from graphite_amd import backend as B
    T = len(o) - 1
    consumed, finished = B.window_snapshot_state(blob, T)
    assert np.array_equal(finished, consumed.astype(np.int64) == np.diff(np.asarray(o, np.int64)))
    w = _shell(cfg, a, m, o, consumed, words, first, tail, whole_tiles, be)
    w.cur = w._make(np.ones(T, np.int64), count=False)
    w.be.coherent_window_restore(*w.cur[:4], final_tiles=w.cur[4], blob=blob)
    w.final = w.cur[4].astype(bool)
    w.size = size
    return w


def _advance_to(w, stop):
    """advance(stop) over the hand-overs it asks for; (next quantum, done)."""
    while True:
        nq, done = w.be.coherent_advance(stop)
        if done != NEED:
            return nq, done
        w.hand_over()


def _pause(w, stop):
    """To the pause at stop; the snapshot, with the words gathered so far.
    window_snapshot_state of the blob must say what coherent_window_state says."""
    from graphite_amd import backend as B
    nq, done = _advance_to(w, stop)
    assert done == 0 and nq >= stop, (nq, done, stop)
    w.gather()
    c = w.be.coherent_window_state()[0]
    blob = w.be.coherent_window_snapshot()
    assert len(blob) == w.be.coherent_window_snapshot_size()
    got, fin = B.window_snapshot_state(blob, w.T)
    assert np.array_equal(got, c), "window_snapshot_state != coherent_window_state before the snapshot"
    return nq, blob


def _in_legs(cfg, a, m, o, stops, prepare=None):
    """Windowed (need + 8) to every stop; there: gather, snapshot, close, a
    fresh context restored with one-record windows, on with need + 3, tail 2.
    The finished Windowed (its backend open) and the hand-overs of every leg."""
    w = Legs(cfg, a, m, o, GROW, prepare=prepare)
    legs = []
    for stop in stops:
        nq, blob = _pause(w, stop)
        legs.append(w.handovers)
        words = w.words
        w.be.close()
        w = _resume(cfg, a, m, o, blob, words, OTHER, tail=2)
        assert w.be.coherent_advance() == (nq, NEED), "one-record windows: the next advance asks at once"
    w.run()
    legs.append(w.handovers)
    return w, legs


def _blob_diff(x, y):
    if len(x) != len(y):
        return "sizes %d != %d" % (len(x), len(y))
    d = np.flatnonzero(np.asarray(x) != np.asarray(y))
    if d.size == 0:
        return None
    return "%d of %d bytes differ, first at %d, in %s" % (d.size, len(x), d[0], sorted({_section_at(x, int(i)) for i in d[:4096]}))


def _qs(blob):
    s = [s for s in _sections(bytes(blob)) if s[0] == "qs"][0]
    return struct.unpack_from("<%dQ" % (s[4] // 8), bytes(blob), s[3])


# ---- 1. legs equal whole ---------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(CASES))
def test_windowed_legs_equal_whole(name):
    cfg, a, m, o = case(name)
    ref = reference(name)
    F = int(ref[5][FINAL])
    assert F >= 6
    w, legs = _in_legs(cfg, a, m, o, [F // 3, 2 * F // 3])
    got = w.state()
    w.be.close()
    print(name, "final quantum", F, "hand-overs per leg", legs)
    assert len(legs) == 3 and all(h >= 1 for h in legs)
    _same(got, ref, "%s, windowed, two pauses in fresh contexts: " % name)


# ---- 2. the bytes do not depend on the cuts -----------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("name", ["hbh_mosi_16x4", "hbh_shl2_mesi_16x4"])
def test_snapshot_bytes_do_not_depend_on_the_cuts(name):
    cfg, a, m, o = case(name)
    ref = reference(name)
    T = len(o) - 1
    stop = int(ref[5][FINAL]) // 2
    one = Legs(cfg, a, m, o, GROW, whole_tiles=range(T))          # the whole trace as one window, every tile final
    q1, b1 = _pause(one, stop)
    w1 = one.words
    assert one.handovers == 0
    one.be.close()
    cut = Legs(cfg, a, m, o, GROW)
    q2, b2 = _pause(cut, stop)
    w2 = cut.words
    assert cut.handovers >= 2
    cut.be.close()
    assert q1 == q2
    assert np.array_equal(w1, w2)
    assert _blob_diff(b1, b2) is None, _blob_diff(b1, b2)
    # each one's snapshot continued the other way
    w = _resume(cfg, a, m, o, b1, w1, GROW).run()
    got = w.state()
    w.be.close()
    assert w.handovers >= 1
    _same(got, ref, "%s: the one-window run's snapshot continued in windows: " % name)
    w = _resume(cfg, a, m, o, b2, w2, GROW, whole_tiles=range(T)).run()
    got = w.state()
    w.be.close()
    assert w.handovers == 0
    _same(got, ref, "%s: the windowed run's snapshot continued in whole-rest final windows: " % name)


# ---- 3. what rides along ------------------------------------------------------------------
@pytest.mark.gpu
def test_barrier_release_pending_at_the_pause():
    from oracle import pyoracle as po
    T, K = 16, 4
    cfg = C.default_config(T, num_shards=K, net_model=HBH, protocol=C.PROTO_MSI, quantum_ns=QNS)
    a, m, o = _with_barriers(*po.gen_trace(T, 240), 30)
    be, ref = _whole(cfg, a, m, o)
    be.close()
    assert int(((ref[0] & np.uint64(3)) == C.LVL_SYNC).sum()) == T * 7
    # single-step to the first boundary past quantum 4 whose snapshot carries a
    # release for the next quantum's step 0 (QS_REL: the latest arrival + 1)
    w = Legs(cfg, a, m, o, GROW, tail=1)
    nq, blob = 0, None
    while True:
        nq, done = _advance_to(w, nq + 1)
        assert done == 0, "the run ended before a pause with a release pending"
        if nq <= 4:
            continue
        blob = w.be.coherent_window_snapshot()
        if _qs(blob)[QS_REL] != 0:
            break
    w.gather()
    waiting = int((w.m[w.o[:-1] + w.consumed] == np.uint32(C.META_BARRIER)).sum())
    print("paused before quantum", nq, "release at", _qs(blob)[QS_REL], "ps, tiles at a BARRIER record", waiting)
    assert waiting == T                                                # every tile waits: the release is pending
    words = w.words
    w.be.close()
    w = _resume(cfg, a, m, o, blob, words, OTHER, tail=2).run()
    got = w.state()
    w.be.close()
    assert w.handovers >= 1
    _same(got, ref, "a barrier release pending at the pause: ")


@pytest.mark.gpu
def test_miss_types_across_a_windowed_pause():
    name = "hbh_mosi_16x4"
    over = dict(l1d_track_miss_types=1, l2_track_miss_types=1, miss_track_lines=1024)
    cfg, a, m, o = case(name, **over)
    be, ref = _whole(cfg, a, m, o)
    mt = be.miss_types()
    be.close()
    assert mt.sum() > 0
    F = int(ref[5][FINAL])
    w, legs = _in_legs(cfg, a, m, o, [F // 2])
    got, mg = w.state(), w.be.miss_types()
    w.be.close()
    assert all(h >= 1 for h in legs)
    _same(got, ref, "miss-type tracking on, windowed, one pause: ")
    assert np.array_equal(mg, mt)


@pytest.mark.gpu
def test_statistics_trace_across_a_windowed_pause():
    cfg, a, m, o = case("hbh_mosi_16x4")
    prep = lambda be: be.stats_trace_configure(3, 4 * cfg.quantum_ns, 4096)
    be, ref = _whole(cfg, a, m, o, prepare=prep)
    tr = be.stats_trace()
    be.close()
    F = int(ref[5][FINAL])
    stop = 4 * (F // 8)                                                # a sample is due at this boundary
    assert 0 < stop < F and len(tr["time_ns"]) > 10
    w, legs = _in_legs(cfg, a, m, o, [stop], prepare=prep)
    got, tg = w.state(), w.be.stats_trace()
    w.be.close()
    assert all(h >= 1 for h in legs)
    _same(got, ref, "statistics trace on, windowed, one pause: ")
    assert sorted(tg) == sorted(tr)
    for k in tr:
        assert np.array_equal(tg[k], tr[k]), "statistics trace field %s differs across the windowed pause" % k


# ---- 4. every clean point ------------------------------------------------------------------
@pytest.mark.gpu
def test_every_clean_point():
    name = "hbh_mosi_16x4"
    cfg, a, m, o = case(name)
    ref = reference(name)
    F = int(ref[5][FINAL])
    T = len(o) - 1
    w = Legs(cfg, a, m, o, GROW)
    be = w.be
    shots = {}

    def shoot(what):
        shots[what] = (be.coherent_window_snapshot(), w.words.copy(), be.coherent_window_state()[0].copy())

    shoot("after begin_window")
    assert not shots["after begin_window"][2].any()
    assert be.coherent_advance() == (0, NEED)
    w.hand_over()
    nq, done = be.coherent_advance()
    assert done == NEED and nq > 0
    w.gather()
    shoot("at a NEED_WINDOW pause")
    assert _qs(shots["at a NEED_WINDOW pause"][0])[QS_DONE] == 4        # stored as a pause, whatever asked for it
    w.hand_over()
    shoot("after a hand-over")
    nq, done = _advance_to(w, 2 * F // 3)
    assert done == 0
    w.gather()
    shoot("at a stop")
    w.run()                                                            # the snapshots left the run as it was
    got = w.state()
    _same(got, ref, "snapshots taken along the way, the same context continued: ")
    shoot("after done == 1")
    be.close()
    for what, (blob, words, consumed) in shots.items():
        from graphite_amd import backend as B
        c, fin = B.window_snapshot_state(blob, T)
        assert np.array_equal(c, consumed), what
        if what == "after done == 1":
            assert fin.all()
            r = _resume(cfg, a, m, o, blob, words, OTHER)               # empty final windows
            assert r.cur[2][-1] == 0 and r.cur[4].all()
            assert r.be.coherent_advance()[1] == 1                      # over, with no launch
            got = _state(r.be, r.cur[3])
            got[0] = r.words.copy()
        else:
            r = _resume(cfg, a, m, o, blob, words, OTHER, tail=2).run()
            assert r.handovers >= 1
            got = r.state()
        r.be.close()
        _same(got, ref, "snapshot %s, restored in a fresh context: " % what)


@pytest.mark.gpu
def test_restore_then_snapshot_is_the_identity():
    name = "hbh_shl2_mesi_16x4"
    cfg, a, m, o = case(name)
    F = int(reference(name)[5][FINAL])
    w = Legs(cfg, a, m, o, GROW)
    nq, blob = _pause(w, F // 2)
    words = w.words
    w.be.close()
    r = _resume(cfg, a, m, o, blob, words, OTHER, first=lambda t, need: 5 + t)
    again = r.be.coherent_window_snapshot()
    r.be.close()
    assert _blob_diff(blob, again) is None, _blob_diff(blob, again)


# ---- 5. refusals -----------------------------------------------------------------------------
def _raises(code, fn, *args, **kw):
    from graphite_amd import backend as B
    with pytest.raises(B.GGError) as e:
        fn(*args, **kw)
    assert e.value.code == code, (e.value.code, str(e.value))
    return str(e.value)


def _windows(a, m, o, consumed, counts):
    """counts[t] records of every tile from record consumed[t]: (addr, meta,
    offsets, out), final flags (a window that reaches the end of its trace)."""
    torch = torch_dev()
    a, m, o = np.asarray(a, np.uint64), np.asarray(m, np.uint32), np.asarray(o, np.int64)
    lo = o[:-1] + np.asarray(consumed, np.int64)
    hi = np.minimum(lo + np.asarray(counts, np.int64), o[1:])
    idx = np.concatenate([np.arange(x, y) for x, y in zip(lo, hi)]).astype(np.int64)
    woffs = np.concatenate([[0], np.cumsum(hi - lo)]).astype(np.uint64)
    out = torch.zeros(len(idx), dtype=torch.int64, device="cuda")
    return [to_dev(torch, a[idx], torch.int64), to_dev(torch, m[idx], torch.int32), woffs, out], (hi == o[1:]).astype(np.uint8)


@pytest.mark.gpu
def test_refusals(monkeypatch):
    from graphite_amd import backend as B
    torch = torch_dev()
    name = "hbh_mosi_16x4"
    T, N, K, net, proto = CASES[name]
    cfg, a, m, o = case(name)
    ref = reference(name)
    F = int(ref[5][FINAL])
    w = Legs(cfg, a, m, o, GROW)
    nq, blob = _pause(w, F // 2)
    # the old contract on a windowed run is intact
    _raises(ERR_UNSUPPORTED, w.be.coherent_snapshot_size)
    _raises(ERR_UNSUPPORTED, w.be.coherent_snapshot, 1 << 20)
    words, consumed = w.words, w.consumed.copy()
    w.run()
    over = w.be.coherent_window_snapshot()                             # every tile finished
    w.be.close()
    assert (consumed > 0).all() and (consumed < N).all()

    be = B.Backend(cfg)
    zero = np.zeros(T, np.int64)
    fresh, fresh_fin = _windows(a, m, o, zero, np.full(T, N))          # a first window for a fresh run: the whole trace

    def still_good():
        be.coherent_begin_window(*fresh, final_tiles=fresh_fin)
        assert be.coherent_window_state()[0].sum() == 0

    def refused(code, word, args, fin, b):
        text = _raises(code, be.coherent_window_restore, *args, final_tiles=fin, blob=b)
        assert word in text, text
        still_good()
        return text

    good, good_fin = _windows(a, m, o, consumed, np.full(T, 5))
    # one flipped address bit in one tile's first record
    bad = list(good)
    bad[0] = good[0].clone()
    bad[0][int(good[2][7])] ^= 64
    assert "tile 7" in refused(ERR_INVALID, "first record", bad, good_fin, blob)
    # an unfinished tile with an empty range
    cnt = np.full(T, 5)
    cnt[3] = 0
    args, fin = _windows(a, m, o, consumed, cnt)
    assert "tile 3" in refused(ERR_INVALID, "unfinished", args, fin, blob)
    # a finished tile with records; and every tile finished, no window, but not marked final
    args, fin = _windows(a, m, o, zero, np.full(T, 1))
    refused(ERR_INVALID, "finished tile", args, np.ones(T, np.uint8), over)
    none, none_fin = _windows(a, m, o, np.full(T, N), zero)
    assert none_fin.all()
    refused(ERR_INVALID, "not final", none, None, over)
    # an ordinary snapshot into the windowed restore, a windowed one into the ordinary restore
    full = [to_dev(torch, np.array(a), torch.int64), to_dev(torch, np.array(m), torch.int32), np.asarray(o, np.uint64)]
    be.coherent_begin(*full)
    assert be.coherent_advance(F // 2)[1] == 0
    # (a run that is not windowed has no windowed snapshot)
    assert "gg_coherent_snapshot" in _raises(ERR_INVALID, be.coherent_window_snapshot)
    assert "gg_coherent_snapshot" in _raises(ERR_INVALID, be.coherent_window_snapshot_size)
    plain = be.coherent_snapshot()
    refused(ERR_INVALID, "gg_coherent_restore", good, good_fin, plain)
    text = _raises(ERR_INVALID, be.coherent_restore, blob, *full)
    assert "gg_coherent_window_restore" in text, text
    still_good()
    # cut short by 8 bytes; a payload byte flipped
    refused(ERR_INVALID, "truncated", good, good_fin, blob[:-8].copy())
    flip = blob.copy()
    flip[len(flip) // 2] ^= 1
    refused(ERR_INVALID, "checksum", good, good_fin, flip)
    # a failed run has no snapshot
    monkeypatch.setenv("GG_WINDOW_FAIL_EXHAUSTED", "1")
    assert "window exhausted" in _raises(-5, be.coherent_advance)
    monkeypatch.delenv("GG_WINDOW_FAIL_EXHAUSTED")
    assert "failed" in _raises(ERR_INVALID, be.coherent_window_snapshot)
    still_good()
    # after all of it the intact snapshot restores here and finishes as the reference does
    r = _resume(cfg, a, m, o, blob, words, OTHER, tail=2, be=be).run()
    got = r.state()
    be.close()
    _same(got, ref, "restored after the refusals: ")
    # another quantum_ns
    be = B.Backend(C.default_config(T, num_shards=K, net_model=net, protocol=proto, quantum_ns=2 * QNS))
    refused(ERR_INVALID, "gg_config", good, good_fin, blob)
    be.close()
    # a context that does not own every shard
    be = B.Backend(C.default_config(T, num_shards=K, net_model=net, protocol=proto, quantum_ns=QNS, shard_begin=0, shard_end=2))
    assert "every shard" in _raises(ERR_UNSUPPORTED, be.coherent_window_restore, *good, final_tiles=good_fin, blob=blob)
    be.close()


@pytest.mark.gpu
def test_atac_context_is_refused():
    from graphite_amd import backend as B
    torch = torch_dev()
    be = B.Backend(C.default_config(64, net_model=C.NET_ATAC))
    addr = torch.zeros(64, dtype=torch.int64, device="cuda")
    meta = torch.zeros(64, dtype=torch.int32, device="cuda")
    offs = np.arange(65, dtype=np.uint64)
    for call in (be.coherent_window_snapshot_size, lambda: be.coherent_window_snapshot(1 << 16),
                 lambda: be.coherent_window_restore(addr, meta, offs, blob=np.zeros(64, np.uint8))):
        with pytest.raises(B.GGError, match="batch API only") as e:
            call()
        assert e.value.code == ERR_UNSUPPORTED
    be.close()


# ---- 6. gg_replay --window with --checkpoint / --restore ---------------------------------------
@pytest.mark.gpu
def test_replay_window_checkpoint_and_restore(tmp_path):
    torch_dev()
    if not os.path.exists(REPLAY):
        pytest.fail("gg_replay is not built")
    base = [REPLAY, "--coherent", "--tiles", "16", "--per-tile", "3000", "--net", "hop_by_hop", "--shards", "4"]
    run = lambda extra: subprocess.run(base + extra, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=120)
    whole = run([])
    assert whole.returncode == 0, whole.stderr
    ck = str(tmp_path / "run.ckpt")
    first = run(["--window", "64", "--checkpoint", ck, "--checkpoint-quantum", "40"])
    assert first.returncode == 0, first.stderr
    print(first.stderr.strip())
    assert "paused at quantum" in first.stderr and first.stdout == "" and os.path.getsize(ck) > 0
    second = run(["--window", "37", "--restore", ck])
    assert second.returncode == 0, second.stderr
    print(second.stderr.strip())
    assert "windows handed over" in second.stderr
    assert len(whole.stdout) > 1000 and second.stdout == whole.stdout
