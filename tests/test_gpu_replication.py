"""GPU: the cache_line_replication samples of k_stats_scan (gg_stats.hip)
against a census that does not come from it: the oracle's walk of its own
caches and directory slices (popcount of the sharer bits, replaced-entry list
included; pinned to the reference's code by tests/golden/coh_*_census.u64,
tests/test_replication_census.py), and those reference rows directly.

Every comparison is exact: the four line counts and bins 1 .. T of every
sample, the device's bin 0 being 0.  The shapes (tests/replication_util.py)
are the smallest that reach the states a scan can get wrong — replaced
entries whose NULLIFY is still in flight at most quantum ends, thousands of
valid entries without a sharer, two sharer words, tiles parked at a barrier,
samples standing for many sampling times, a rank owning some of the shards, a
directory unpacked by a restore; tests/test_replication_census.py asserts on
the CPU that they do."""
import numpy as np
import pytest

import golden_util as G
import replication_util as R
from graphite_amd import config as C
from test_stats_trace import ST_NET, ST_REPL, due

pytestmark = pytest.mark.gpu


def _device_trace(cfg, a, m, o, interval, max_samples, want_text=False):
    """gg_coherent_run with both statistics traced: (trace, access words, network counters[, replication text])."""
    from gpu_util import torch_dev, to_dev, to_np
    torch = torch_dev()
    from graphite_amd import backend as B
    be = B.Backend(cfg)
    be.stats_trace_configure(ST_NET | ST_REPL, interval, max_samples)
    out = torch.zeros(len(a), dtype=torch.int64, device="cuda")
    be.coherent_run(to_dev(torch, np.array(a), torch.int64), to_dev(torch, np.array(m), torch.int32), o, out)
    res = (be.stats_trace(), to_np(out, np.uint64), be.noc_counters())
    if want_text:
        res += (be.stats_trace_text(ST_REPL),)
    be.close()
    return res


def _flits(tr):
    return np.stack([tr[k] for k in R.FLIT_FIELDS], axis=1)


def _run_and_compare(name):
    cfg, a, m, o, interval = R.shape(name)
    s = R.series(name)
    tr, out, nc = _device_trace(cfg, a, m, o, interval, len(s.time) + 8)
    print(name, "samples", len(tr["time_ns"]), "max repeat", int(s.repeat.max()),
          "with pending replaced entries", int((s.pending.sum(axis=1) > 0).sum()))
    R.compare(tr, s, what=name + ": ")
    assert np.array_equal(_flits(tr), s.flits), "flits of the intervals differ"
    assert np.array_equal(out, s.out), "access words differ from the oracle with the trace on"
    assert np.array_equal(nc, s.net), "network counters differ from the oracle with the trace on"


# A, B, C: every quantum end of the run; D: the cases of tests/test_stats_trace.py
# at their own intervals (4 and 10 quanta, one sample standing for 156 sampling
# times); F: tiles parked at BARRIER records
@pytest.mark.parametrize("name", R.A_AND_B + ["C_mosi", "C_msi"] + sorted(R.TRACE_CASES) + ["F_mosi_hbh_barriers"])
def test_samples_equal_oracle_census(name):
    _run_and_compare(name)


def test_samples_equal_oracle_census_on_hbm_cache_arrays(monkeypatch):
    """E: GG_COH_NO_LDS_CACHE=1.  The variable chooses between the persistent
    launch's two forms, and a run with a trace configured takes the per-step
    launches (cache state always in HBM): it must change nothing here, and
    this is case A_mosi_hbh again with it set."""
    monkeypatch.setenv("GG_COH_NO_LDS_CACHE", "1")
    _run_and_compare("A_mosi_hbh")


# (the n500 cases hold the whole series: most of their rows show replaced entries that still have sharers)
@pytest.mark.parametrize("name,manifest", [("mosi_dir16s4", G.coh_mosi_manifest), ("dir16s4", G.coh_manifest),
                                           ("mosi_dir16s4n500", G.coh_mosi_manifest), ("dir16s4n500", G.coh_manifest),
                                           ("mosi_hot12", G.coh_mosi_manifest), ("shard72f266", G.coh_manifest)])
def test_samples_equal_reference_census_rows(name, manifest):
    """The device against the rows the reference's own code wrote, no oracle in
    between: a sample after every quantum, matched to the rows by quantum."""
    m = manifest()[name]
    cfg, a, meta, o, exp = G.coh_case(name, m)
    T = m["tiles"]
    ref = G.load("coh_%s_census.u64" % name, np.uint64).reshape(-1, 5 + T)
    assert len(ref) == m["census_rows"]
    tr, out, _ = _device_trace(cfg, a, meta, o, cfg.quantum_ns, m["quanta"] + 8)
    assert np.array_equal(out, exp["out"])
    assert len(tr["time_ns"]) == m["quanta"] and np.all(tr["repeat"] == 1)
    got = np.concatenate([(tr["time_ns"] // np.uint64(cfg.quantum_ns) - np.uint64(1))[:, None]] +
                         [tr[k][:, None] for k in R.LINE_FIELDS] + [tr["sharer_hist"][:, 1:]], axis=1)
    if len(ref) == 1:
        got = got[-1:]                                   # a long series: the fixture holds the end of the run
    bad = np.argwhere(got != ref)
    assert len(bad) == 0, "row %d (quantum %d), column %d: device %d, reference %d" % (
        bad[0][0], ref[bad[0][0], 0], bad[0][1], got[tuple(bad[0])], ref[tuple(bad[0])])
    assert not tr["sharer_hist"][:, 0].any()


def test_rank_samples_add_up_to_the_oracle():
    """Case A (MOSI, hop-by-hop) over two contexts on one GPU, each owning two
    of the four shards, driven by the round halves; after every finished round
    with a sampling time due each rank samples its own shards
    (gg_stats_trace_sample).  Each rank's counts are the oracle's census over
    its tiles; summed over the ranks a sample is the single-context oracle's."""
    from gpu_util import torch_dev
    torch = torch_dev()
    from graphite_amd import coherent as CO
    from tests.test_gpu_round import _run_ranks
    name, W = "A_mosi_hbh", 2
    cfg, a, m, o, interval = R.shape(name)
    s = R.series(name)
    T, K = cfg.num_tiles, cfg.num_shards
    traces = []

    def after_round(bes, q, nq, done):
        d = due(q, q + 1 if done else nq, cfg.quantum_ns, interval)
        if d:
            for be in bes:
                be.stats_trace_sample(d[0])
        if done:
            traces.extend(be.stats_trace() for be in bes)

    stats = {"again": 0, "overflow": 0}
    got = _run_ranks(torch, W, K, {"T": T, "net": cfg.net_model, "protocol": cfg.protocol, "config": R.SHAPES[name]["cfg"]},
                     np.array(a), np.array(m), np.array(o), stats,
                     prepare=lambda be: be.stats_trace_configure(ST_NET | ST_REPL, interval, len(s.time) + 8),
                     after_round=after_round)
    assert np.array_equal(got[0], s.out) and np.array_equal(got[2], s.net)
    assert len(traces) == W
    shard = C.shard_map(T, K)
    total = {k: sum(tr[k] for tr in traces) for k in R.LINE_FIELDS + R.FLIT_FIELDS + ("sharer_hist",)}
    for r, tr in enumerate(traces):
        k0, k1 = CO.shard_range(r, W, K)
        tiles = np.flatnonzero((shard >= k0) & (shard < k1))
        assert 0 < len(tiles) < T
        # (a host-called sample stands for one sampling time: the run skips no quantum here, asserted on the CPU)
        R.compare(tr, s, tiles=tiles, what="rank %d: " % r)
    total["time_ns"], total["repeat"] = traces[0]["time_ns"], traces[0]["repeat"]
    R.compare(total, s, what="summed over the ranks: ")
    assert np.array_equal(_flits(total), s.flits), "flits of the intervals, summed over the ranks"


def test_sample_after_a_restore():
    """Case A (MOSI, hop-by-hop), traced every 4 quanta, paused where replaced
    entries still have sharers and no sample is due; the snapshot restored into
    a fresh context, whose directory arrays are unpacked from the slots in use:
    one sample taken there equals the oracle's census at that quantum end, and
    the samples of the whole run equal the oracle's."""
    from gpu_util import torch_dev, to_dev, to_np
    torch = torch_dev()
    from graphite_amd import backend as B
    cfg, a, m, o, interval = R.shape("A_mosi_hbh_i4")
    s4, s1 = R.series("A_mosi_hbh_i4"), R.series("A_mosi_hbh")
    q, row = R.pause_quantum()
    assert s1.pending[row].sum() > 0 and q % 4 != 0
    addr, meta = to_dev(torch, np.array(a), torch.int64), to_dev(torch, np.array(m), torch.int32)
    out = torch.zeros(len(a), dtype=torch.int64, device="cuda")
    be = B.Backend(cfg)
    be.stats_trace_configure(ST_NET | ST_REPL, interval, len(s4.time) + 9)
    be.coherent_begin(addr, meta, o, out)
    assert be.coherent_advance(q) == (q, 0)
    blob = be.coherent_snapshot()
    be.close()
    be = B.Backend(cfg)
    be.coherent_restore(blob, addr, meta, o, out)
    at = q * cfg.quantum_ns                              # the barrier the run stands at: no multiple of the interval
    be.stats_trace_sample(at)
    assert be.coherent_advance()[1] == 1
    tr = be.stats_trace()
    res = to_np(out, np.uint64)
    be.close()
    k = int((s4.time <= np.uint64(at)).sum())            # the samples before the pause travelled in the snapshot
    assert 0 < k < len(s4.time) and int(tr["time_ns"][k]) == at and int(tr["repeat"][k]) == 1
    extra = {f: v[k:k + 1] for f, v in tr.items()}
    R.compare(extra, _at(s1, row, at), what="the sample after the restore (quantum %d ended): " % (q - 1))
    rest = {f: np.delete(v, k, axis=0) for f, v in tr.items()}
    R.compare(rest, s4, what="the run's samples around the restore: ")
    # the extra sample took the flits since the sample before it out of the next interval
    fl, exp = _flits(tr), s4.flits.copy()
    assert np.array_equal(fl[k] + fl[k + 1], exp[k]) and np.array_equal(np.delete(fl, [k, k + 1], axis=0), np.delete(exp, k, axis=0))
    assert np.array_equal(res, s4.out)


class _at:
    """One row of a series as a series of its own, at another sampling time."""

    def __init__(self, s, row, time_ns):
        self.T = s.T
        self.time, self.repeat, self.q = np.array([time_ns], np.uint64), np.array([1], np.uint64), s.q[row:row + 1]
        self.lines, self.hist = s.lines[row:row + 1], s.hist[row:row + 1]


def test_replication_text_is_the_reference_arithmetic():
    """cache_line_replication.dat of case A (MOSI) sampled every 4 quanta
    against …mosi/memory_manager.cc:553-599 restated in Python over the same
    fields (total_tiles = T + 2); the fields are the oracle's, and nearly every
    sample has a non-integer L1 / L2 shared ratio."""
    import math
    name = "A_mosi_hbh_i4"
    cfg, a, m, o, interval = R.shape(name)
    s = R.series(name)
    tr, _, _, text = _device_trace(cfg, a, m, o, interval, len(s.time) + 8, want_text=True)
    R.compare(tr, s, what=name + ": ")
    T = cfg.num_tiles
    degrees = [int(tr["l1_shared"][i]) / int(tr["l2_shared"][i]) * n for i in range(len(tr["time_ns"]))
               for n in range(1, T + 1) if tr["sharer_hist"][i][n] and tr["l2_shared"][i]]
    assert any(d != math.floor(d) for d in degrees), "no non-integer degree in the series"
    assert text == R.replication_text(T + 2, T, tr)
