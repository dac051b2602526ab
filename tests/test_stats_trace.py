"""The [statistics_trace] time series (gg_stats_trace_*):
network_utilization_memory.dat and cache_line_replication.dat sampled when
the lax barrier releases at a multiple of the sampling interval.

The expected network series comes from the oracle stepped quantum by quantum
(begin / quantum / export / import_ with the next-quantum rule of
oracle_coh_run), reading its network counters after every quantum: the
oracle's stepped run equals its whole run, so the per-interval flit sums are
the reference series.  The replication counts are checked here against states
known by construction and against protocol invariants; sample by sample they
are pinned to the oracle's census and to the census rows of the reference's
own controllers in tests/test_gpu_replication.py."""
import functools
import os
import subprocess

import numpy as np
import pytest

from graphite_amd import config as C
from graphite_amd.coherent import next_quantum

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REPLAY = os.path.join(ROOT, "graphite_amd", "host", "gg_replay")
ST_NET, ST_REPL = 1, 2
FS, FB, FR = (C.NET_COUNTERS.index(k) for k in ("flits_sent", "flits_broadcasted", "flits_received"))
HBH, HC = C.NET_EMESH_HOP_BY_HOP, C.NET_EMESH_HOP_COUNTER

# name: (tiles, records per tile, shards, network, protocol, interval in quanta, gap of the middle record)
CASES = {
    "hbh_mosi_16x4": (16, 300, 4, HBH, C.PROTO_MOSI, 4, 0),
    "hbh_msi_64x8": (64, 200, 8, HBH, C.PROTO_MSI, 4, 0),
    "hc_mosi_16x1": (16, 300, 1, HC, C.PROTO_MOSI, 10, 0),
    # every tile's middle record waits 1 000 000 cycles, longer than the whole
    # run without the gap (25 000 and 100 000 cycles are hidden behind the
    # slowest tiles: no repeat): every tile idles at once and the run skips
    # empty quanta across many sampling times (a sample with repeat > 1)
    "skipped_boundaries": (16, 300, 4, HBH, C.PROTO_MOSI, 4, 1000000),
}


@functools.lru_cache(maxsize=None)
def case(name):
    from oracle import pyoracle as po
    T, N, K, net, proto, iq, gap = CASES[name]
    cfg = C.default_config(T, num_shards=K, net_model=net, protocol=proto)
    a, m, o = po.gen_trace(T, N)
    if gap:
        m = m.copy()
        mid = o[:-1].astype(np.int64) + N // 2
        m[mid] = (np.uint32(gap) << np.uint32(1)) | (m[mid] & np.uint32(1))
    for x in (a, m, o):
        x.setflags(write=False)
    return cfg, a, m, o, iq * cfg.quantum_ns


def due(q, nq, quantum_ns, interval_ns):
    """(first sampling time, how many) among the barrier times (q+1)*Q ... nq*Q
    the lax barrier passes when quantum q ended and quantum nq runs next."""
    lo, hi = (q + 1) * quantum_ns, nq * quantum_ns
    first = -(-lo // interval_ns) * interval_ns
    return (first, (hi - first) // interval_ns + 1) if first <= hi else None


def drive(engine, cfg, interval_ns, on_sample):
    """The quantum loop of oracle_coh_run / gg_coherent_run over an engine
    (quantum / export / import_), with on_sample(time_ns, repeat) wherever the
    device loop samples: after the quantum's last step (the boundary import
    changes no statistic).  The last quantum counts only its own barrier."""
    q = 0
    while True:
        st = engine.quantum(q)
        buf, per_shard = engine.export()
        msgs = int(np.asarray(per_shard, np.int64).sum())
        nq = next_quantum(q, cfg.quantum_ns * 1000, msgs, st["active_tiles"], st["blocked_tiles"], st["min_next_ps"])
        d = due(q, q + 1 if nq is None else nq, cfg.quantum_ns, interval_ns)
        if d:
            on_sample(*d)
        if len(buf):
            engine.import_(buf)
        if nq is None:
            return
        q = nq


@functools.lru_cache(maxsize=None)
def stepped_oracle(name):
    """The oracle stepped quantum by quantum: (samples [n][5] = time_ns,
    repeat, flits sent / broadcast / received in the interval; access words;
    network counters) — computed once per case, shared, read-only."""
    from coherent_util import OracleEngine
    cfg, a, m, o, interval = case(name)
    eng = OracleEngine(cfg, a, m, o)
    rows, prev = [], np.zeros(3, np.int64)

    def on_sample(t, rep):
        nc = eng.o.net_counters().astype(np.int64)
        cur = np.array([nc[:, FS].sum(), nc[:, FB].sum(), nc[:, FR].sum()])
        rows.append([t, rep] + list(cur - prev))
        prev[:] = cur

    drive(eng, cfg, interval, on_sample)
    s = np.array(rows, np.uint64).reshape(-1, 5)
    out, nc = eng.out.copy(), eng.o.net_counters()
    for x in (s, out, nc):
        x.setflags(write=False)
    return s, out, nc


# ---- CPU ---------------------------------------------------------------

@pytest.mark.parametrize("name", sorted(CASES))
def test_stepped_oracle_is_the_reference_series(name):
    from oracle import pyoracle as po
    cfg, a, m, o, interval = case(name)
    s, out, nc = stepped_oracle(name)
    whole = po.OracleCoherent(cfg)
    ref = whole.run(a, m, o)
    assert np.array_equal(out, ref), "stepped oracle != whole run (access words)"
    assert np.array_equal(nc, whole.net_counters()), "stepped oracle != whole run (network counters)"
    assert len(s) > 0
    assert np.all(s[1:, 0] > s[:-1, 0]) and np.all(s[:, 0] % interval == 0) and np.all(s[:, 1] >= 1)
    # consecutive samples leave no sampling time out
    assert np.array_equal(s[1:, 0], s[:-1, 0] + s[:-1, 1] * interval)
    tot = nc.astype(np.int64)
    assert s[:, 2].sum() <= tot[:, FS].sum() and s[:, 4].sum() <= tot[:, FR].sum() and s[:, 3].sum() == 0
    if cfg.num_shards > 1:
        # packets held at a shard edge are sent but not yet received: the two columns differ
        assert np.any(s[:, 2] != s[:, 4])
    else:
        assert s[:, 2].sum() > 0


def test_skipped_boundary_case_has_a_repeat():
    s, _, _ = stepped_oracle("skipped_boundaries")
    assert s[:, 1].max() > 1


def test_text_writers_match_hand_written_strings():
    """Three samples (4 application tiles, total_tiles 6, interval 1000 ns; the
    second stands for 3 sampling times, the third has no shared line) through
    the host writers; the expected text is written out by hand from
    network.cc:632-635 and …mosi/memory_manager.cc:553-599."""
    if not os.path.exists(REPLAY):
        pytest.skip("gg_replay not built")
    out = subprocess.run([REPLAY, "--stats-trace-selftest"], capture_output=True, text=True, check=True).stdout
    net = ("0.0536667, 0, 0.0323333\n"        # 322 / 6000, 0, 194 / 6000
           "0.00116667, 0.000166667, 1\n"     # 7 / 6000, 1 / 6000, 6000 / 6000
           "0, 0, 0\n"
           "0, 0, 0\n"
           "0, 0, 0\n")
    # sample 1: L1 5 / 6, L2 9 / 12, entries by sharers 11 2 1 1.  Degrees:
    # [1] = 9 - 5, [2] = 5; bin 1 -> 11 - 9 = 2 lines; ratio 6 / 12:
    # 1 sharer: 2 lines at 0.5 -> 1 low ([1]) + 1 high ([2]); 2 sharers: 2 lines
    # at 1 -> [3]; 3 sharers: 1 line at 1.5 -> (uint64) 0.5 = 0 low, 1 high ([5]);
    # 4 sharers: 1 line at 2 -> [6]
    rep1 = ("5, 6, \n"
            "9, 12, \n"
            "11, 2, 1, 1, 0, 0, \n"
            "5, 6, 2, 0, 1, 1, 0, 0, 0, 0, 0, 0, \n"
            "\n")
    # sample 2: no shared L1 line: every shared line at degree 0 -> [3] for the 3-sharer line
    rep2 = ("2, 0, \n"
            "4, 3, \n"
            "4, 0, 1, 0, 0, 0, \n"
            "2, 2, 1, 0, 0, 0, 0, 0, 0, 0, 0, 0, \n"
            "\n")
    # sample 3: no shared L2 line (the reference divides by zero here): bins empty after the exclusive lines
    rep3 = ("3, 0, \n"
            "3, 0, \n"
            "3, 0, 0, 0, 0, 0, \n"
            "0, 3, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, \n"
            "\n")
    assert out == net + rep1 + rep2 * 3 + rep3


# ---- GPU ---------------------------------------------------------------

def _dev_trace(torch, a, m):
    from gpu_util import to_dev
    return to_dev(torch, a, torch.int64), to_dev(torch, m, torch.int32)


def _fields(tr, names=("time_ns", "repeat", "flits_sent", "flits_broadcasted", "flits_received")):
    return np.stack([tr[k] for k in names], axis=1)


def expand(tr):
    """Samples with their repeats written out (zero utilisation, the same
    replication state), one row per sampling time: [time, 3 flits, 4 line
    counts, histogram]."""
    rows = []
    for i in range(len(tr["time_ns"])):
        for r in range(int(tr["repeat"][i])):
            fl = [0, 0, 0] if r else [int(tr[k][i]) for k in ("flits_sent", "flits_broadcasted", "flits_received")]
            rows.append([int(tr["time_ns"][i]), r] + fl +
                        [int(tr[k][i]) for k in ("l1_exclusive", "l1_shared", "l2_exclusive", "l2_shared")] +
                        [int(x) for x in tr["sharer_hist"][i]])
    return rows


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(CASES))
def test_network_utilisation_matches_stepped_oracle(name):
    from gpu_util import torch_dev, to_np
    torch = torch_dev()
    from graphite_amd import backend as B
    cfg, a, m, o, interval = case(name)
    exp, ref_out, ref_nc = stepped_oracle(name)
    be = B.Backend(cfg)
    be.stats_trace_configure(ST_NET, interval, len(exp) + 8)
    addr, meta = _dev_trace(torch, a, m)
    out = torch.zeros(len(a), dtype=torch.int64, device="cuda")
    be.coherent_run(addr, meta, o, out)
    tr = be.stats_trace()
    got = _fields(tr)
    nc = be.noc_counters()
    res = to_np(out, np.uint64)
    be.close()
    print(name, "samples", len(got), "expected", len(exp), "repeat max", int(exp[:, 1].max()))
    assert got.shape == exp.shape, (got.shape, exp.shape)
    assert np.array_equal(got, exp), "first differing sample %s" % np.argwhere(got != exp)[0]
    assert np.array_equal(res, ref_out), "access words differ from the oracle with the trace on"
    assert np.array_equal(nc, ref_nc), "network counters differ from the oracle with the trace on"


@pytest.mark.gpu
def test_device_loop_equals_host_loop():
    """MOSI, hop-by-hop, 64 tiles in 8 shards, both statistics: gg_coherent_run's
    samples against a host-driven run (coherent_begin / quantum / export /
    import) that calls stats_trace_sample at the same boundaries.  A device
    sample with repeat r is r host samples: compared with the repeats written
    out (all fields, histogram included)."""
    from gpu_util import torch_dev
    torch = torch_dev()
    from graphite_amd import backend as B
    from oracle import pyoracle as po
    T, N, K = 64, 200, 8
    cfg = C.default_config(T, num_shards=K, net_model=HBH, protocol=C.PROTO_MOSI)
    a, m, o = po.gen_trace(T, N)
    interval = 4 * cfg.quantum_ns
    addr, meta = _dev_trace(torch, a, m)
    dev = B.Backend(cfg)
    dev.stats_trace_configure(ST_NET | ST_REPL, interval, 4096)
    dev.coherent_run(addr, meta, o, None)
    td = dev.stats_trace()
    dev.close()
    host = B.Backend(cfg)
    host.stats_trace_configure(ST_NET | ST_REPL, interval, 4096)
    eng = B.CoherentEngine(host, addr, meta, o)

    def on_sample(t, rep):
        for r in range(rep):
            host.stats_trace_sample(t + r * interval)

    drive(eng, cfg, interval, on_sample)
    th = host.stats_trace()
    host.close()
    assert len(td["time_ns"]) > 10 and td["l2_exclusive"].max() > 0 and td["sharer_hist"][:, 2:].sum() > 0
    assert np.all(th["repeat"] == 1)
    # sampling times: the device's first + k * interval, the host's as called
    tdx = [int(t) + r * interval for t, rep in zip(td["time_ns"], td["repeat"]) for r in range(int(rep))]
    assert tdx == [int(t) for t in th["time_ns"]]
    ed, eh = expand(td), expand(th)
    assert len(ed) == len(eh)
    for x, y in zip(ed, eh):
        assert x[2:] == y[2:], "sample at %d ns differs" % x[0]


def _known_trace(T, H, P, hot_writer_gap=0):
    """Every tile reads the same H lines and writes P lines of its own
    (consecutive lines: no eviction, no full directory set); optionally tile 0
    then writes the H hot lines after a gap that puts it last."""
    hot = (np.uint64(63) << np.uint64(26)) + np.arange(H, dtype=np.uint64) * np.uint64(64)
    parts_a, parts_m = [], []
    for t in range(T):
        own = (np.uint64(t) << np.uint64(26)) + (np.uint64(1) << np.uint64(20)) + np.arange(P, dtype=np.uint64) * np.uint64(64)
        aa, mm = [hot, own], [np.zeros(H, np.uint32), np.ones(P, np.uint32)]
        if hot_writer_gap and t == 0:
            g = np.ones(H, np.uint32)
            g[0] |= np.uint32(hot_writer_gap << 1)
            aa.append(hot)
            mm.append(g)
        parts_a.append(np.concatenate(aa))
        parts_m.append(np.concatenate(mm))
    o = np.concatenate([[0], np.cumsum([len(x) for x in parts_a])]).astype(np.uint64)
    return np.concatenate(parts_a), np.concatenate(parts_m), o


def _replication_text(total, ex1, sh1, ex2, sh2, hist):
    """memory_manager.cc:553-599 for the states of the known-state test (the
    L1 / L2 shared ratio is 0 or 1 there: every degree is an integer)."""
    h = list(hist[1:]) + [0] * (total - (len(hist) - 1))
    rep = [0] * (2 * total + 1)
    rep[1] += ex2 - ex1
    rep[2] += ex1
    cnt = [0] + h
    cnt[1] -= ex2
    ratio = sh1 // sh2 if sh2 else 0
    for k in range(1, total + 1):
        if cnt[k]:
            rep[k + ratio * k] += cnt[k]
    return ("%d, %d, \n%d, %d, \n" % (ex1, sh1, ex2, sh2) + "".join("%d, " % x for x in h) + "\n" +
            "".join("%d, " % x for x in rep[1:]) + "\n\n")


@pytest.mark.gpu
@pytest.mark.parametrize("proto", [C.PROTO_MOSI, C.PROTO_MSI])
@pytest.mark.parametrize("hot_writer", [False, True])
def test_known_state(proto, hot_writer):
    from gpu_util import torch_dev
    torch = torch_dev()
    from graphite_amd import backend as B
    T, H, P = 16, 8, 8
    cfg = C.default_config(T, net_model=HC, protocol=proto)
    a, m, o = _known_trace(T, H, P, 200000 if hot_writer else 0)
    addr, meta = _dev_trace(torch, a, m)
    be = B.Backend(cfg)
    interval = 10 ** 9                                   # (no sampling time inside the run)
    be.stats_trace_configure(ST_NET | ST_REPL, interval, 4)
    be.coherent_run(addr, meta, o, None)
    be.stats_trace_sample(interval)
    tr = be.stats_trace()
    nc = be.noc_counters().astype(np.int64)
    text_n, text_r = be.stats_trace_text(ST_NET), be.stats_trace_text(ST_REPL)
    be.close()
    assert len(tr["time_ns"]) == 1 and tr["time_ns"][0] == interval and tr["repeat"][0] == 1
    ex, sh = (T * P + H, 0) if hot_writer else (T * P, T * H)
    hist = np.zeros(T + 1, np.int64)
    hist[1] = T * P + (H if hot_writer else 0)
    hist[T] = 0 if hot_writer else H
    got = [int(tr[k][0]) for k in ("l1_exclusive", "l1_shared", "l2_exclusive", "l2_shared")]
    print("lines", got, "hist", {i: int(v) for i, v in enumerate(tr["sharer_hist"][0]) if v})
    assert got == [ex, sh, ex, sh]
    assert np.array_equal(tr["sharer_hist"][0].astype(np.int64), hist)
    fl = [int(nc[:, c].sum()) for c in (FS, FB, FR)]
    assert [int(tr[k][0]) for k in ("flits_sent", "flits_broadcasted", "flits_received")] == fl
    total = T + 2
    assert text_n == "%s, %s, %s\n" % tuple("%g" % (x / (total * interval)) for x in fl)
    assert text_r == _replication_text(total, ex, sh, ex, sh, hist)


@pytest.mark.gpu
@pytest.mark.parametrize("proto", [C.PROTO_MOSI, C.PROTO_MSI])
def test_invariants_under_evictions_and_replacements(proto):
    """A small L2 and a small directory: L2 evictions and directory
    replacements both occur.  At the end of the run nothing is in flight, so
    every L2 line is one sharer of its directory entry (the owner is a sharer,
    …mosi/dram_directory_cntlr.cc:404-408) and every exclusive L1 line is
    exclusive in the L2."""
    from gpu_util import torch_dev
    torch = torch_dev()
    from graphite_amd import backend as B
    from oracle import pyoracle as po
    T = 16
    # (a directory of 64 entries a tile back-invalidates every line before an 8 KB L2 fills: 256)
    cfg = C.default_config(T, l1d_size_kb=2, l2_size_kb=8, dir_total_entries=256, dir_assoc=4, protocol=proto,
                           net_model=HBH)
    a, m, o = po.gen_trace(T, 1500, hot_lines=32)
    addr, meta = _dev_trace(torch, a, m)
    be = B.Backend(cfg)
    be.stats_trace_configure(ST_NET | ST_REPL, 10 * cfg.quantum_ns, 1 << 14)
    be.coherent_run(addr, meta, o, None)
    st, cc, ri = be.coherent_stats()
    be.stats_trace_sample(int(ri[C.RUN_INFO.index("final_quantum")] + 2) * cfg.quantum_ns)
    tr = be.stats_trace()
    nc = be.noc_counters().astype(np.int64)
    be.close()
    l2_ev = int(cc[:, 1, C.CACHE_COUNTERS.index("evictions")].sum())
    dir_ev = int(st[:, C.TILE_STATS.index("dir_evictions")].sum())
    print("quanta", int(ri[0]), "L2 evictions", l2_ev, "directory replacements", dir_ev, "samples", len(tr["time_ns"]))
    assert l2_ev > 0 and dir_ev > 0 and ri[C.RUN_INFO.index("quanta")] > 10
    h = tr["sharer_hist"][-1].astype(np.int64)
    l1x, l2x, l2s = int(tr["l1_exclusive"][-1]), int(tr["l2_exclusive"][-1]), int(tr["l2_shared"][-1])
    print("end of run: L1 excl", l1x, "L2 excl", l2x, "L2 shared", l2s, "sum n*hist", int((np.arange(T + 1) * h).sum()))
    assert h[0] == 0 and l2x + l2s > 0
    assert int((np.arange(T + 1) * h).sum()) == l2x + l2s
    assert l1x <= l2x
    # in-run samples: times ascending; with the sample after the run the intervals' flits add up to the run's totals
    assert len(tr["time_ns"]) > 2 and np.all(np.diff(tr["time_ns"].astype(np.int64)) > 0)
    for k, c in (("flits_sent", FS), ("flits_broadcasted", FB), ("flits_received", FR)):
        assert int(tr[k].astype(np.int64).sum()) == int(nc[:, c].sum()), k


@pytest.mark.gpu
def test_errors():
    from gpu_util import torch_dev
    torch = torch_dev()
    from graphite_amd import backend as B
    name = "hc_mosi_16x1"
    cfg, a, m, o, interval = case(name)
    exp, _, _ = stepped_oracle(name)
    assert len(exp) > 2
    addr, meta = _dev_trace(torch, a, m)
    be = B.Backend(cfg)
    with pytest.raises(B.GGError) as e:
        be.stats_trace_configure(ST_NET, cfg.quantum_ns + cfg.quantum_ns // 2, 16)
    assert e.value.code == -1                            # GG_ERR_INVALID
    with pytest.raises(B.GGError) as e:
        be.stats_trace_configure(ST_NET, 0, 16)
    assert e.value.code == -1
    with pytest.raises(B.GGError) as e:                  # a sample buffer above GG_ST_MAX_BUFFER_BYTES (1 GiB)
        be.stats_trace_configure(ST_NET, interval, 1 << 40)
    assert e.value.code == -1
    # a buffer of 2 samples on a run that needs more: an error, not a short series
    be.stats_trace_configure(ST_NET, interval, 2)
    with pytest.raises(B.GGError) as e:
        be.coherent_run(addr, meta, o, None)
    assert e.value.code == -3 and "sample buffer" in str(e.value)
    # run_many refuses a context with a trace configured, and takes it again once the trace is off
    be.stats_trace_configure(ST_NET, interval, 64)
    with pytest.raises(B.GGError) as e:
        B.coherent_run_many([be], [addr], [meta], [o])
    assert e.value.code == -3                            # GG_ERR_UNSUPPORTED
    be.stats_trace_configure(0)
    assert B.coherent_run_many([be], [addr], [meta], [o]) == [0]
    be.close()
    sh = B.Backend(C.default_config(16, protocol=C.PROTO_SHL2_MSI))
    with pytest.raises(B.GGError) as e:
        sh.stats_trace_configure(ST_REPL, interval, 16)
    assert e.value.code == -3
    sh.stats_trace_configure(ST_NET, interval, 16)       # the network statistic has no such limit
    sh.close()
