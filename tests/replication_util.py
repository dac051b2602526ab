"""Shared by tests/test_replication_census.py (CPU) and
tests/test_gpu_replication.py (GPU): the shapes at which the
cache_line_replication samples are pinned, and the oracle's series for them —
the oracle stepped quantum by quantum (drive / next_quantum of
tests/test_stats_trace.py) with OracleCoherent.census() wherever the device
samples.  Each series is computed once per case, shared and read-only."""
import functools

import numpy as np

from graphite_amd import config as C
from test_stats_trace import CASES as TRACE_CASES, case as trace_case, drive, due, FS, FB, FR, HBH, HC

MSI, MOSI = C.PROTO_MSI, C.PROTO_MOSI
LINE_FIELDS = ("l1_exclusive", "l1_shared", "l2_exclusive", "l2_shared")
FLIT_FIELDS = ("flits_sent", "flits_broadcasted", "flits_received")

# A: a small L2 and a small directory in 4 shards: replaced entries whose
# NULLIFY is in flight at most quantum ends, valid entries without a sharer,
# L2 evictions.  B: the same on a 3 x 4 mesh at 1.5 GHz.  C: 8 x 9 tiles (two
# sharer words, 73 bins).  Intervals in quanta.
_A = dict(T=16, N=500, hot=32, K=4, cfg=dict(l1d_size_kb=2, l2_size_kb=8, dir_total_entries=256, dir_assoc=4))
_B = dict(T=12, N=400, hot=16, K=3, net=HBH,
          cfg=dict(frequency_ghz=1.5, l1d_size_kb=1, l1d_assoc=2, l2_size_kb=4, l2_assoc=4, dir_total_entries=192,
                   dir_assoc=4))
_C = dict(T=72, N=100, hot=16, K=8, net=HBH, cfg=dict(frequency_ghz=1.5))
SHAPES = {
    "A_mosi_hbh": dict(_A, net=HBH, proto=MOSI),
    "A_mosi_hc": dict(_A, net=HC, proto=MOSI),
    "A_msi_hbh": dict(_A, net=HBH, proto=MSI),
    "A_msi_hc": dict(_A, net=HC, proto=MSI),
    "B_mosi": dict(_B, proto=MOSI),
    "B_msi": dict(_B, proto=MSI),
    "C_mosi": dict(_C, proto=MOSI),
    "C_msi": dict(_C, proto=MSI),
    # A (MOSI, hop-by-hop) with a BARRIER record after every 100 accesses of each tile
    "F_mosi_hbh_barriers": dict(_A, net=HBH, proto=MOSI, barriers=100),
    # A (MOSI, hop-by-hop) sampled every 4 quanta (the text test, the run after a restore)
    "A_mosi_hbh_i4": dict(_A, net=HBH, proto=MOSI, interval=4),
}
A_AND_B = [n for n in sorted(SHAPES) if n[0] in "AB" and not n.endswith("_i4")]


def with_barriers(a, m, offs, every):
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
def shape(name):
    """(cfg, addr, meta, offsets, interval_ns) of a SHAPES entry or of a case of tests/test_stats_trace.py."""
    if name in TRACE_CASES:
        return trace_case(name)
    from oracle import pyoracle as po
    s = SHAPES[name]
    cfg = C.default_config(s["T"], num_shards=s["K"], net_model=s["net"], protocol=s["proto"], **s["cfg"])
    a, m, o = po.gen_trace(s["T"], s["N"], hot_lines=s["hot"])
    if s.get("barriers"):
        a, m, o = with_barriers(a, m, o, s["barriers"])
    for x in (a, m, o):
        x.setflags(write=False)
    return cfg, a, m, o, s.get("interval", 1) * cfg.quantum_ns


class Series:
    """The oracle's samples of a run: per sample the sampling time, the repeat,
    the flits of the interval, and the census per tile."""

    def __init__(self, T):
        self.T, self.rows = T, []

    def add(self, oc, t, rep, prev):
        nc = oc.net_counters().astype(np.int64)
        cur = np.array([nc[:, FS].sum(), nc[:, FB].sum(), nc[:, FR].sum()])
        self.rows.append((t, rep, cur - prev) + oc.census())
        prev[:] = cur

    def freeze(self, out, nc, quantum_ns):
        r = self.rows
        self.time = np.array([x[0] for x in r], np.uint64)
        self.repeat = np.array([x[1] for x in r], np.uint64)
        self.q = self.time // np.uint64(quantum_ns) - np.uint64(1)      # the quantum whose end the sample shows
        self.flits = np.array([x[2] for x in r], np.uint64).reshape(-1, 3)
        self.lines = np.array([x[3] for x in r], np.uint64).reshape(-1, self.T, 4)
        self.hist = np.array([x[4] for x in r], np.uint64).reshape(-1, self.T, self.T + 1)
        self.pending = np.array([x[5] for x in r], np.uint64).reshape(-1, self.T)
        self.out, self.net = out, nc
        del self.rows
        for x in (self.time, self.repeat, self.q, self.flits, self.lines, self.hist, self.pending, self.out, self.net):
            x.setflags(write=False)
        return self


def stepped_census(cfg, a, m, o, interval_ns, last_only=False):
    """The oracle stepped quantum by quantum (begin / quantum / export /
    import_), a census wherever the device loop samples.  last_only: the last
    sample alone (one census, of the state the run ends in: the last boundary
    hand-over changes none of it)."""
    from coherent_util import OracleEngine
    eng = OracleEngine(cfg, a, m, o)
    s, prev = Series(cfg.num_tiles), np.zeros(3, np.int64)
    if last_only:
        last = []
        drive(eng, cfg, interval_ns, lambda t, rep: last.append((t, rep)))
        s.add(eng.o, last[-1][0], last[-1][1], prev)
    else:
        drive(eng, cfg, interval_ns, lambda t, rep: s.add(eng.o, t, rep, prev))
    return s.freeze(eng.out.copy(), eng.o.net_counters(), cfg.quantum_ns)


def hooked_census(cfg, a, m, o, interval_ns, last_only=False):
    """The same series out of the oracle's whole run (oracle_coh_run with its
    between-quanta hook): the way to sample a trace with BARRIER records, which
    only the whole run releases, and the quick way through a long run."""
    from oracle import pyoracle as po
    oc = po.OracleCoherent(cfg)
    s, prev, last = Series(cfg.num_tiles), np.zeros(3, np.int64), []

    def hook(q, nq):
        d = due(q, nq, cfg.quantum_ns, interval_ns)
        if d and last_only:
            last[:] = [d]
        elif d:
            s.add(oc, d[0], d[1], prev)

    oc.set_quantum_hook(hook)
    out = oc.run(a, m, o)
    oc.set_quantum_hook(None)
    if last_only:
        s.add(oc, last[0][0], last[0][1], prev)
    return s.freeze(out.copy(), oc.net_counters(), cfg.quantum_ns)


@functools.lru_cache(maxsize=None)
def series(name):
    cfg, a, m, o, interval = shape(name)
    barriers = bool((m == np.uint32(C.META_BARRIER)).any())
    return (hooked_census if barriers else stepped_census)(cfg, a, m, o, interval)


def pause_quantum():
    """The pause of the restore test: (quantum to run next, row of the
    every-quantum series of A_mosi_hbh showing the state there) — about a third
    into the run, replaced entries pending, no sample of the 4-quantum trace
    due (the quantum that just ended is q - 1; a sample is due when q * Q is a
    multiple of the interval), and the next quantum the one after (no skip)."""
    s = series("A_mosi_hbh")
    pend = s.pending.sum(axis=1)
    for row in range(len(s.q) // 3, len(s.q) - 1):
        q = int(s.q[row]) + 1
        if pend[row] > 0 and q % 4 != 0 and int(s.q[row + 1]) == q:
            return q, row
    raise AssertionError("no quantum end with pending replaced entries off the sampling grid")


def compare(tr, s, rows=None, tiles=None, what=""):
    """A device trace (Backend.stats_trace()) against the oracle's series (its
    samples `rows`, default all; the census summed over `tiles`, default all):
    sampling time, repeat, the four line counts and bins 1 .. T, sample by
    sample, exactly; the device's bin 0 is 0.  The first difference is named
    by sample, field and tile count."""
    rows = np.arange(len(s.time)) if rows is None else np.asarray(rows)
    tiles = np.arange(s.T) if tiles is None else np.asarray(tiles)
    assert len(tr["time_ns"]) == len(rows), "%s%d samples, expected %d" % (what, len(tr["time_ns"]), len(rows))
    assert np.array_equal(tr["time_ns"], s.time[rows]), what + "sampling times differ"
    assert np.array_equal(tr["repeat"], s.repeat[rows]), what + "repeats differ"
    lines = s.lines[rows][:, tiles].sum(axis=1)
    hist = s.hist[rows][:, tiles].sum(axis=1)
    for k, f in enumerate(LINE_FIELDS):
        bad = np.flatnonzero(tr[f] != lines[:, k])
        assert len(bad) == 0, "%s%s differs first at sample %d (quantum %d): device %d, oracle %d" % (
            what, f, bad[0], s.q[rows][bad[0]], tr[f][bad[0]], lines[bad[0], k])
    got = tr["sharer_hist"]
    bad = np.argwhere(got[:, 1:] != hist[:, 1:])
    assert len(bad) == 0, "%ssharer_hist differs first at sample %d (quantum %d), bin %d: device %d, oracle %d" % (
        what, bad[0][0], s.q[rows][bad[0][0]], bad[0][1] + 1, got[bad[0][0], bad[0][1] + 1], hist[bad[0][0], bad[0][1] + 1])
    assert not got[:, 0].any(), what + "the device counts entries without a sharer"


def replication_text(total, T, tr):
    """cache_line_replication.dat of a trace, …mosi/memory_manager.cc:553-599
    restated over the same fields with the same IEEE doubles; each sample
    written `repeat` times.  With the three deliberate deviations of
    writeCacheLineReplicationTrace (graphite_amd/host/graphite_host.hpp): over
    zero shared L2 lines the ratio is 0 (the reference divides by zero); empty
    bins are skipped; a degree past 2 * total_tiles is dropped, not written
    out of bounds."""
    import math
    out = []
    for i in range(len(tr["time_ns"])):
        ex1, sh1, ex2, sh2 = (int(tr[k][i]) for k in LINE_FIELDS)
        cnt = [0] + [int(x) for x in tr["sharer_hist"][i][1:]] + [0] * (total - T)
        txt = "%d, %d, \n%d, %d, \n" % (ex1, sh1, ex2, sh2) + "".join("%d, " % x for x in cnt[1:]) + "\n"
        rep = [0] * (2 * total + 1)
        rep[1] = (rep[1] + ex2 - ex1) & (2 ** 64 - 1)
        rep[2] += ex1
        cnt[1] = (cnt[1] - ex2) & (2 ** 64 - 1)
        ratio = 1.0 * sh1 / sh2 if sh2 else 0.0
        for n in range(1, total + 1):
            lines = cnt[n]
            if lines == 0:
                continue
            d = ratio * n
            low = int(lines * (math.ceil(d) - d))
            for deg, k in ((int(math.floor(d)), low), (int(math.ceil(d)), lines - low)):
                if n + deg <= 2 * total:
                    rep[n + deg] = (rep[n + deg] + k) & (2 ** 64 - 1)
        txt += "".join("%d, " % x for x in rep[1:]) + "\n\n"
        out.append(txt * int(tr["repeat"][i]))
    return "".join(out)
