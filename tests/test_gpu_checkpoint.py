"""Pause, snapshot and restore of a coherent run at a quantum boundary
(gg_coherent_advance / _snapshot / _restore).

An interrupted and restored run must equal the uninterrupted run, which the
oracle pins: every comparison here is word for word.  The shapes are the small
ones of the other coherent tests; the whole runs and the oracle's results are
computed once per case and shared (read-only)."""
import functools
import os
import struct
import subprocess

import numpy as np
import pytest

from graphite_amd import config as C
from graphite_amd.coherent import next_quantum
from tests.gpu_util import torch_dev, to_dev, to_np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REPLAY = os.path.join(ROOT, "graphite_amd", "host", "gg_replay")
HBH, HC, MAGIC = C.NET_EMESH_HOP_BY_HOP, C.NET_EMESH_HOP_COUNTER, C.NET_MAGIC
FINAL = C.RUN_INFO.index("final_quantum")
ERR_INVALID, ERR_UNSUPPORTED, ERR_RANGE = -1, -3, -4

# name: (tiles, records per tile, shards, network, protocol)
CASES = {
    "hbh_mosi_16x4": (16, 300, 4, HBH, C.PROTO_MOSI),
    "hbh_msi_64x8": (64, 200, 8, HBH, C.PROTO_MSI),
    "hc_msi_16x1": (16, 300, 1, HC, C.PROTO_MSI),          # the persistent kernels on the last leg
    "hbh_shl2_mesi_16x4": (16, 300, 4, HBH, C.PROTO_SHL2_MESI),
    "magic_shl2_msi_16": (16, 300, 1, MAGIC, C.PROTO_SHL2_MSI),
}


def _ro(*xs):
    for x in xs:
        x.setflags(write=False)
    return xs


@functools.lru_cache(maxsize=None)
def case(name, **over):
    from oracle import pyoracle as po
    T, N, K, net, proto = CASES[name]
    cfg = C.default_config(T, num_shards=K, net_model=net, protocol=proto, **over)
    a, m, o = _ro(*po.gen_trace(T, N))
    return cfg, a, m, o


def _dev(torch, a, m):
    return to_dev(torch, np.array(a), torch.int64), to_dev(torch, np.array(m), torch.int32)


def _state(be, out):
    """Everything a finished (or paused) run reports: access words, tile
    statistics, cache counters, NoC counters, protocol statistics, run info."""
    st, cc, ri = be.coherent_stats()
    return [to_np(out, np.uint64).copy(), st, cc, be.noc_counters(), be.protocol_stats(), ri]


NAMES = ("access words", "tile statistics", "cache counters", "NoC counters", "protocol statistics", "run info")


def _same(x, y, what=""):
    for name, p, q in zip(NAMES, x, y):
        if not np.array_equal(p, q):
            d = np.argwhere(np.asarray(p) != np.asarray(q))
            raise AssertionError("%s%s differ at %d places, first %s: %s != %s"
                                 % (what, name, len(d), d[0], np.asarray(p)[tuple(d[0])], np.asarray(q)[tuple(d[0])]))


def _whole(cfg, a, m, o, prepare=None):
    """begin + advance(never): the uninterrupted run through the new entry."""
    torch = torch_dev()
    from graphite_amd import backend as B
    be = B.Backend(cfg)
    if prepare:
        prepare(be)
    addr, meta = _dev(torch, a, m)
    out = torch.zeros(len(a), dtype=torch.int64, device="cuda")
    be.coherent_begin(addr, meta, o, out)
    nq, done = be.coherent_advance()
    assert done == 1
    return be, _state(be, out)


def _legs(cfg, a, m, o, stops, prepare=None, fresh=lambda i: True, blobs=None):
    """begin, advance to every stop; at each pause snapshot and restore (into a
    new context where fresh(i), closing the old one; else into the same), then
    the last leg to the end.  Returns the backend and the final state."""
    torch = torch_dev()
    from graphite_amd import backend as B
    be = B.Backend(cfg)
    if prepare:
        prepare(be)
    addr, meta = _dev(torch, a, m)
    out = torch.zeros(len(a), dtype=torch.int64, device="cuda")
    be.coherent_begin(addr, meta, o, out)
    for i, stop in enumerate(stops):
        nq, done = be.coherent_advance(stop)
        if done:
            break
        assert nq >= stop
        blob = be.coherent_snapshot()
        if blobs is not None:
            blobs.append((nq, blob))
        if fresh(i):
            be.close()
            be = B.Backend(cfg)            # (no prepare: restore re-establishes the configuration)
        be.coherent_restore(blob, addr, meta, o, out)
    nq, done = be.coherent_advance()
    assert done == 1
    return be, _state(be, out)


@functools.lru_cache(maxsize=None)
def reference(name):
    """The uninterrupted run of a case: gg_coherent_run against the oracle
    (_compare), and begin + advance(~0), which must give the same."""
    cfg, a, m, o = case(name)
    if cfg.protocol in (C.PROTO_SHL2_MSI, C.PROTO_SHL2_MESI):
        # the same comparison with the oracle, with the shared-L2 invariants
        # (coherent_util's are those of a private L2: L2 accesses = L1-D misses per tile)
        from tests.test_gpu_shl2 import _compare
    else:
        from tests.coherent_util import _compare
    g = _compare(cfg, np.array(a), np.array(m), np.array(o))
    be, w = _whole(cfg, a, m, o)
    be.close()
    _same(w[:4] + [w[5]], list(g[:4]) + [g[4]], "begin + advance(~0) against gg_coherent_run: ")
    _ro(*w)
    return w


# ---- 1. interrupted == uninterrupted == oracle -------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(CASES))
def test_interrupted_equals_uninterrupted(name):
    cfg, a, m, o = case(name)
    ref = reference(name)
    F = int(ref[5][FINAL])
    assert F >= 3
    blobs = []
    be, got = _legs(cfg, a, m, o, [1, F // 3, 2 * F // 3], blobs=blobs)
    be.close()
    print(name, "final quantum", F, "pauses at", [q for q, _ in blobs], "snapshot bytes", [len(b) for _, b in blobs])
    assert len(blobs) == 3
    _same(got, ref, "%s, three pauses in fresh contexts: " % name)


# ---- 2. the pause point against the stepped oracle -----------------------------
def _oracle_to(cfg, a, m, o, stop):
    """The drive / next_quantum loop of tests/test_stats_trace.py, until the
    quantum to run next is >= stop: (engine, that quantum)."""
    from tests.coherent_util import OracleEngine
    eng = OracleEngine(cfg, np.array(a), np.array(m), np.array(o))
    q = 0
    while True:
        st = eng.quantum(q)
        buf, per_shard = eng.export()
        msgs = int(np.asarray(per_shard, np.int64).sum())
        nq = next_quantum(q, cfg.quantum_ns * 1000, msgs, st["active_tiles"], st["blocked_tiles"], st["min_next_ps"])
        if len(buf):
            eng.import_(buf)
        if nq is None:
            return eng, None
        q = nq
        if q >= stop:
            return eng, q


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["hbh_mosi_16x4", "hbh_msi_64x8"])
def test_pause_point_equals_stepped_oracle(name):
    torch = torch_dev()
    from graphite_amd import backend as B
    cfg, a, m, o = case(name)
    F = int(reference(name)[5][FINAL])
    be = B.Backend(cfg)
    addr, meta = _dev(torch, a, m)
    out = torch.zeros(len(a), dtype=torch.int64, device="cuda")
    be.coherent_begin(addr, meta, o, out)
    for stop in (F // 3, 2 * F // 3):
        eng, oq = _oracle_to(cfg, a, m, o, stop)
        nq, done = be.coherent_advance(stop)
        assert done == 0 and nq == oq, (stop, nq, oq)
        st, cc, ri = be.coherent_stats()            # the getters work on a paused run
        nc = be.noc_counters()
        for what, x, y in (("tile statistics", st, eng.o.tile_stats()), ("cache counters", cc, eng.o.cache_counters()),
                           ("NoC counters", nc, eng.o.net_counters())):
            assert np.array_equal(x, y), "%s at the pause before quantum %d differ from the stepped oracle" % (what, nq)
    be.close()


# ---- 3. every boundary, with barriers -----------------------------------------
def _with_barriers(a, m, offs, every):
    A, M = [], []
    for t in range(len(offs) - 1):
        s, e = int(offs[t]), int(offs[t + 1])
        pos = np.arange(every, e - s, every)
        A.append(np.insert(a[s:e], pos, np.uint64(0)))
        M.append(np.insert(m[s:e], pos, np.uint32(C.META_BARRIER)))
    o = np.concatenate([[0], np.cumsum([len(x) for x in A])]).astype(np.uint64)
    return np.concatenate(A), np.concatenate(M).astype(np.uint32), o


@pytest.mark.gpu
@pytest.mark.parametrize("proto", [C.PROTO_MSI, C.PROTO_MOSI])
def test_every_boundary_with_barriers(proto):
    """Single-step: advance(next + 1) in a loop, every boundary a pause — those
    with a barrier release pending included; snapshot and restore into the
    same context at every pause, into a fresh one at every tenth."""
    torch = torch_dev()
    from graphite_amd import backend as B
    from oracle import pyoracle as po
    T, N, K = 16, 120, 4
    cfg = C.default_config(T, num_shards=K, net_model=HBH, protocol=proto)
    a, m, o = _with_barriers(*po.gen_trace(T, N), 30)
    oc = po.OracleCoherent(cfg)
    ref = [oc.run(a, m, o), oc.tile_stats(), oc.cache_counters(), oc.net_counters()]
    assert int(((ref[0] & 3) == C.LVL_SYNC).sum()) == T * 3
    be = B.Backend(cfg)
    addr, meta = _dev(torch, a, m)
    out = torch.zeros(len(a), dtype=torch.int64, device="cuda")
    be.coherent_begin(addr, meta, o, out)
    nq, pauses = 0, 0
    while True:
        nq, done = be.coherent_advance(nq + 1)
        if done:
            break
        pauses += 1
        blob = be.coherent_snapshot()
        if pauses % 10 == 0:
            be.close()
            be = B.Backend(cfg)
        be.coherent_restore(blob, addr, meta, o, out)
    assert done == 1
    got = _state(be, out)
    be.close()
    print("protocol", proto, "pauses", pauses, "final quantum", int(got[5][FINAL]))
    assert pauses > 20
    _same(got[:4], ref, "single-stepped with barriers against OracleCoherent.run: ")


# ---- 4. skipped quanta and no-ops ----------------------------------------------
@pytest.mark.gpu
def test_skipped_quanta_and_noops():
    torch = torch_dev()
    from graphite_amd import backend as B
    cfg, a, m, o = case("hbh_mosi_16x4")
    T, N = CASES["hbh_mosi_16x4"][:2]
    m = np.array(m)
    mid = np.asarray(o[:-1], np.int64) + N // 2        # the skipped_boundaries construction:
    m[mid] = (np.uint32(1000000) << np.uint32(1)) | (m[mid] & np.uint32(1))   # every tile's middle record waits
    addr, meta = _dev(torch, a, m)
    out = torch.zeros(len(a), dtype=torch.int64, device="cuda")
    be = B.Backend(cfg)
    be.coherent_begin(addr, meta, o, out)
    seq, nq = [0], 0
    while True:                                        # the quanta the run takes
        nq, done = be.coherent_advance(nq + 1)
        if done:
            break
        seq.append(nq)
    whole = _state(be, out)
    be.close()
    gaps = [(x, y) for x, y in zip(seq, seq[1:]) if y - x > 2]
    assert gaps, "no empty span in this trace"
    lo, hi = max(gaps, key=lambda g: g[1] - g[0])
    be = B.Backend(cfg)
    out2 = torch.zeros(len(a), dtype=torch.int64, device="cuda")
    be.coherent_begin(addr, meta, o, out2)
    stop = lo + (hi - lo) // 2
    nq, done = be.coherent_advance(stop)
    assert (nq, done) == (hi, 0) and stop < hi          # a stop inside the span: the first quantum chosen
    before = be.coherent_snapshot()
    for s in (0, lo, stop, hi):
        assert be.coherent_advance(s) == (hi, 0)        # stop <= current: at once
        assert np.array_equal(be.coherent_snapshot(), before), "a no-op advance changed the state"
    be.coherent_restore(before, addr, meta, o, out2)
    assert be.coherent_advance(hi) == (hi, 0)
    assert np.array_equal(be.coherent_snapshot(), before), "snapshot -> restore -> snapshot is not the identity"
    assert be.coherent_advance() [1] == 1
    _same(_state(be, out2), whole, "paused inside an empty span: ")
    be.close()


# ---- 5. statistics trace across a pause -------------------------------------------
@pytest.mark.gpu
def test_statistics_trace_across_a_pause():
    cfg, a, m, o = case("hbh_mosi_16x4")
    interval = 4 * cfg.quantum_ns
    prep = lambda be: be.stats_trace_configure(3, interval, 4096)
    be, ref = _whole(cfg, a, m, o, prepare=prep)
    tr = be.stats_trace()
    be.close()
    F = int(ref[5][FINAL])
    s1 = 4 * (F // 12)
    s2 = 4 * (F // 6) + 1
    assert 0 < s1 < s2 < F
    blobs = []
    be, got = _legs(cfg, a, m, o, [s1, s2], prepare=prep, blobs=blobs)
    tg = be.stats_trace()
    be.close()
    print("pauses at", [q for q, _ in blobs], "samples", len(tr["time_ns"]), "max repeat", int(tr["repeat"].max()))
    assert len(blobs) == 2 and len(tr["time_ns"]) > 10
    _same(got, ref, "statistics trace on, two pauses: ")
    assert sorted(tg) == sorted(tr)
    for k in tr:
        assert np.array_equal(tg[k], tr[k]), "statistics trace field %s differs across the pauses" % k


# ---- 6. miss types across a pause ----------------------------------------------------
@pytest.mark.gpu
def test_miss_types_across_a_pause():
    cfg, a, m, o = case("hbh_mosi_16x4", l1d_track_miss_types=1, l2_track_miss_types=1, miss_track_lines=1024)
    be, ref = _whole(cfg, a, m, o)
    mt = be.miss_types()
    be.close()
    assert mt.sum() > 0 and mt[:, 1].sum() > 0
    F = int(ref[5][FINAL])
    be, got = _legs(cfg, a, m, o, [F // 3, 2 * F // 3])
    mg = be.miss_types()
    be.close()
    _same(got, ref, "miss-type tracking on, two pauses: ")
    assert np.array_equal(mg, mt)


# ---- 7. determinism and size ------------------------------------------------------------
@pytest.mark.gpu
def test_snapshot_bytes_are_deterministic():
    cfg, a, m, o = case("hbh_mosi_16x4")
    F = int(reference("hbh_mosi_16x4")[5][FINAL])
    got = []
    for _ in range(2):
        blobs = []
        be, _ = _legs(cfg, a, m, o, [F // 2], blobs=blobs)
        be.close()
        got.append(blobs[0])
    assert got[0][0] == got[1][0]
    x, y = got[0][1], got[1][1]
    assert len(x) == len(y)
    d = np.flatnonzero(x != y)
    where = sorted({_section_at(x, int(i)) for i in d[:4096]})
    assert d.size == 0, "%d of %d bytes differ, first at %d, in %s" % (d.size, len(x), d[0], where)


def _sections(blob):
    """[(name, kind, record bytes, offset, bytes, records)] of a snapshot's table (gg_snapshot.h)."""
    magic, version, n, total, csum = struct.unpack_from("<QIIQQ", blob, 0)
    out = []
    for i in range(n):
        name, kind, rec, off, size, records = struct.unpack_from("<16sIIQQQ", blob, 32 + 48 * i)
        out.append((name.split(b"\0")[0].decode(), kind, rec, off, size, records))
    return out


def _section_at(blob, pos):
    for s in _sections(bytes(blob[:32 + 48 * 256])):
        if s[3] <= pos < s[3] + s[4]:
            return s[0]
    return "header / table / padding"


@pytest.mark.gpu
def test_snapshot_is_smaller_than_an_eighth_of_the_dense_directory():
    torch = torch_dev()
    from graphite_amd import backend as B
    from oracle import pyoracle as po
    T = 256
    cfg = C.default_config(T, num_shards=1, net_model=HC, protocol=C.PROTO_MSI)
    a, m, o = po.gen_trace(T, 4)
    be = B.Backend(cfg)
    addr, meta = _dev(torch, a, m)
    be.coherent_begin(addr, meta, o, None)
    n = be.coherent_snapshot_size()
    blob = be.coherent_snapshot()
    be.close()
    # DirectoryCache sizing (gg_coherent.hip, coh_alloc): 2 x the L2's lines per slice
    E = 2 * cfg.l2_size_kb * 1024 // 64
    W = (T + 63) // 64
    dense = T * E * (16 + 8 * W)
    print("snapshot", n, "bytes; dense directory arrays", dense, "bytes; sections",
          [(s[0], s[4]) for s in _sections(bytes(blob)) if s[4] > (1 << 16)])
    assert len(blob) == n
    assert n < dense // 8


# ---- 8. errors -------------------------------------------------------------------------------
def _run_and_compare(be, cfg, a, m, o, ref):
    torch = torch_dev()
    addr, meta = _dev(torch, a, m)
    out = torch.zeros(len(a), dtype=torch.int64, device="cuda")
    be.coherent_run(addr, meta, o, out)
    _same(_state(be, out), ref, "a fresh run after a refused restore: ")


def _refused(be, blob, addr, meta, o, out=None):
    from graphite_amd import backend as B
    with pytest.raises(B.GGError) as e:
        be.coherent_restore(blob, addr, meta, o, out)
    assert e.value.code == ERR_INVALID, e.value
    return str(e.value)


@pytest.mark.gpu
def test_restore_refuses_what_does_not_fit():
    torch = torch_dev()
    from graphite_amd import backend as B
    name = "hbh_mosi_16x4"
    cfg, a, m, o = case(name)
    ref = reference(name)
    F = int(ref[5][FINAL])
    blobs = []
    be, _ = _legs(cfg, a, m, o, [F // 2], blobs=blobs)
    blob = blobs[0][1]
    addr, meta = _dev(torch, a, m)
    # different tile_offsets (same records, another split)
    o2 = np.array(o)
    o2[1] -= 1
    print(_refused(be, blob, addr, meta, o2))
    _run_and_compare(be, cfg, a, m, o, ref)
    # cut at several lengths
    for n in (0, 16, 31, 32, 100, 32 + 48 * 3, len(blob) // 2, len(blob) - 8, len(blob) - 1):
        _refused(be, blob[:n].copy(), addr, meta, o)
    _run_and_compare(be, cfg, a, m, o, ref)
    # a section length overwritten with a huge value (every section in turn), and with one word more
    secs = _sections(bytes(blob))
    assert {"dir", "rep", "l2_tag", "qs", "ts", "cfg", "launch", "offsets"} <= {s[0] for s in secs}
    for i, s in enumerate(secs):
        for v in (1 << 60, (1 << 64) - 8, s[4] + 8):
            bad = blob.copy()
            struct.pack_into("<Q", bad, 32 + 48 * i + 32, v)
            _refused(be, bad, addr, meta, o)
    # a payload byte changed
    bad = blob.copy()
    bad[len(bad) // 2] ^= 1
    _refused(be, bad, addr, meta, o)
    _run_and_compare(be, cfg, a, m, o, ref)
    be.close()
    # a config that differs
    cfg2, _, _, _ = case(name, l2_assoc=4)
    be2, ref2 = _whole(cfg2, a, m, o)
    print(_refused(be2, blob, addr, meta, o))
    _run_and_compare(be2, cfg2, a, m, o, ref2)
    be2.close()
    # the intact snapshot still restores and finishes as the reference does
    be3 = B.Backend(cfg)
    out = torch.zeros(len(a), dtype=torch.int64, device="cuda")
    be3.coherent_restore(blob, addr, meta, o, out)
    assert be3.coherent_advance()[1] == 1
    got = _state(be3, out)
    be3.close()
    # (the words of the records passed before the pause belong to the caller's first buffer)
    _same(got[1:], ref[1:], "restored into a fresh context with a fresh buffer: ")


@pytest.mark.gpu
def test_driver_rules_and_buffer_size():
    torch = torch_dev()
    from graphite_amd import backend as B
    cfg, a, m, o = case("hbh_mosi_16x4")
    addr, meta = _dev(torch, a, m)
    be = B.Backend(cfg)
    with pytest.raises(B.GGError) as e:                 # nothing begun
        be.coherent_snapshot_size()
    assert e.value.code == ERR_INVALID
    be.coherent_begin(addr, meta, o, None)
    need = be.coherent_snapshot_size()
    with pytest.raises(B.GGError) as e:                 # cap too small: the need comes back
        be.coherent_snapshot(cap=need - 1)
    assert e.value.code == ERR_RANGE and e.value.needed == need
    assert len(be.coherent_snapshot(cap=need + 64)) == need
    be.coherent_quantum(0)                              # the host drives this run from here on
    for call in (be.coherent_snapshot_size, be.coherent_snapshot, lambda: be.coherent_advance(5)):
        with pytest.raises(B.GGError) as e:
            call()
        assert e.value.code == ERR_INVALID, e.value
    be.coherent_begin(addr, meta, o, None)
    assert be.coherent_advance(2)[1] == 0               # ... and the device loop this one
    with pytest.raises(B.GGError) as e:
        be.coherent_quantum(2)
    assert e.value.code == ERR_INVALID, e.value
    be.close()
    part = C.default_config(16, num_shards=4, net_model=HBH, protocol=C.PROTO_MOSI, shard_begin=0, shard_end=2)
    bp = B.Backend(part)
    bp.coherent_begin(addr, meta, o, None)
    for call in (lambda: bp.coherent_advance(3), bp.coherent_snapshot_size):
        with pytest.raises(B.GGError) as e:
            call()
        assert e.value.code == ERR_UNSUPPORTED, e.value
    bp.close()


# ---- 9. gg_replay end to end -----------------------------------------------------------------------
@pytest.mark.gpu
def test_replay_checkpoint_and_restore(tmp_path):
    torch_dev()
    if not os.path.exists(REPLAY):
        pytest.fail("gg_replay is not built")
    common = [REPLAY, "--tiles", "16", "--per-tile", "300", "--coherent", "--net", "hop_by_hop", "--shards", "4"]
    whole = subprocess.run(common, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=120)
    assert whole.returncode == 0, whole.stderr
    ck = str(tmp_path / "run.ckpt")
    first = subprocess.run(common + ["--checkpoint", ck, "--checkpoint-quantum", "40"], stdout=subprocess.PIPE,
                           stderr=subprocess.PIPE, text=True, timeout=120)
    assert first.returncode == 0, first.stderr
    assert os.path.getsize(ck) > 0
    second = subprocess.run(common + ["--restore", ck], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True,
                            timeout=120)
    assert second.returncode == 0, second.stderr
    assert len(whole.stdout) > 100
    assert second.stdout == whole.stdout
