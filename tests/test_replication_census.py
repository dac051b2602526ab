"""CPU: the oracle's census (oracle_coh_census: cache lines by state, directory
entries by popcount of their sharers, the replaced-entry list included)
against the census rows the reference's own code wrote
(tests/golden/coh_*_census.u64, oracle/ref/coh_harness.cc: under MOSI the
histogram its controllers' updateSharerStats calls kept, a walk under MSI),
and the properties of the shapes the GPU tests of
tests/test_gpu_replication.py sample, asserted here so that none of them can
pass emptily."""
import numpy as np
import pytest

import golden_util as G
import replication_util as R
from graphite_amd import config as C

FIXTURES = [(n, G.coh_manifest) for n in sorted(G.coh_manifest())] + \
           [(n, G.coh_mosi_manifest) for n in sorted(G.coh_mosi_manifest())]


def fixture_rows(name, m):
    """[rows][5 + T]: quantum, L1-D exclusive / shared, L2 exclusive / shared, entries with 1 .. T sharers."""
    T = m["tiles"]
    rows = G.load("coh_%s_census.u64" % name, np.uint64).reshape(-1, 5 + T)
    assert len(rows) == m["census_rows"] and (len(rows) == m["quanta"] or len(rows) == 1)
    return rows


def series_rows(s):
    """An oracle series in the fixture's row form."""
    return np.concatenate([s.q[:, None], s.lines.sum(axis=1), s.hist.sum(axis=1)[:, 1:]], axis=1)


@pytest.mark.parametrize("name,manifest", FIXTURES, ids=[n for n, _ in FIXTURES])
def test_oracle_census_equals_reference_fixture(name, manifest):
    m = manifest()[name]
    assert "census_rows" in m, "every MSI / MOSI fixture case has census rows"
    cfg, a, meta, o, exp = G.coh_case(name, m)
    ref = fixture_rows(name, m)
    # the oracle's whole run with a census between its quanta (the stepped run
    # gives the same series: test_stepped_census_equals_whole_run); of a long
    # series the fixture holds the end of the run, and one census is taken
    s = R.hooked_census(cfg, a, meta, o, cfg.quantum_ns, last_only=len(ref) == 1 and m["quanta"] > 1)
    assert np.array_equal(s.out, exp["out"]), "the oracle's access words differ from the fixture's"
    got = series_rows(s)
    assert len(got) == len(ref) and np.all(s.repeat == 1)
    bad = np.argwhere(got != ref)
    assert len(bad) == 0, "row %d (quantum %d), column %d: oracle %d, reference %d" % (
        bad[0][0], ref[bad[0][0], 0], bad[0][1], got[tuple(bad[0])], ref[tuple(bad[0])])
    if name.endswith("dir16s4n500"):
        # what these two cases are there for: among the rows just compared with
        # the reference's, most show replaced entries that still have sharers
        # (no other fixture has such a row: one shard never ends a quantum with
        # one, the long sharded series keep their last row, where none is left)
        assert len(ref) == m["quanta"] > 500 and (s.pending.sum(axis=1) > 0).sum() > 500


@pytest.mark.parametrize("name,manifest", [("dir16s4n500", G.coh_manifest), ("mosi_dir16s4n500", G.coh_mosi_manifest)])
def test_stepped_oracle_equals_replaced_list_rows(name, manifest):
    """The short sharded small-directory cases through the drive / next_quantum
    loop: every row equals the reference's, and most of the rows compared show
    replaced entries that still have sharers — a census that skipped the
    replaced list would lose them from bins 1 .. T at each such row."""
    m = manifest()[name]
    cfg, a, meta, o, exp = G.coh_case(name, m)
    ref = fixture_rows(name, m)
    s = R.stepped_census(cfg, a, meta, o, cfg.quantum_ns)
    assert len(ref) == m["quanta"] and np.array_equal(series_rows(s), ref)
    assert (s.pending.sum(axis=1) > 0).sum() > 500


@pytest.mark.parametrize("name,manifest", [("dir16s4", G.coh_manifest), ("mosi_dir16s4", G.coh_mosi_manifest)])
def test_sharded_small_directory_fixtures_reach_the_replaced_list(name, manifest):
    """Entries on the replaced list still have sharers at most quantum ends of
    the long cases too; their fixture holds the end of the run only, where
    none is left (the n500 cases hold the rows)."""
    cfg, a, meta, o, exp = G.coh_case(name, manifest()[name])
    s = R.stepped_census(cfg, a, meta, o, cfg.quantum_ns)
    assert (s.pending.sum(axis=1) > 0).sum() > 100
    ref = fixture_rows(name, manifest()[name])
    assert np.array_equal(series_rows(s)[-1:], ref)       # (and the stepped run ends where the fixture does)
    assert s.pending[-1].sum() == 0


def test_census_is_refused_under_shared_l2():
    from oracle import pyoracle as po
    for proto in (C.PROTO_SHL2_MSI, C.PROTO_SHL2_MESI):
        oc = po.OracleCoherent(C.default_config(16, protocol=proto))
        with pytest.raises(RuntimeError):
            oc.census()


@pytest.mark.parametrize("name", ["A_mosi_hbh", "A_msi_hc", "B_mosi", "C_msi", "skipped_boundaries"])
def test_stepped_census_equals_whole_run(name):
    """A census at every sample disturbs nothing: access words and network
    counters of the stepped run equal oracle_coh_run's; and the whole run's
    between-quanta hook gives the same series as the stepped run."""
    from oracle import pyoracle as po
    cfg, a, m, o, interval = R.shape(name)
    s = R.series(name)
    whole = po.OracleCoherent(cfg)
    assert np.array_equal(s.out, whole.run(a, m, o)) and np.array_equal(s.net, whole.net_counters())
    h = R.hooked_census(cfg, a, m, o, interval)
    for f in ("time", "repeat", "flits", "lines", "hist", "pending", "out", "net"):
        assert np.array_equal(getattr(h, f), getattr(s, f)), f


def test_census_of_a_rank_is_its_tiles():
    """A context that owns some of the shards reports its own tiles only."""
    from oracle import pyoracle as po
    cfg, a, m, o, _ = R.shape("A_mosi_hbh")
    own = C.shard_map(16, 4) < 2
    part = po.OracleCoherent(C.default_config(16, num_shards=4, shard_begin=0, shard_end=2, protocol=cfg.protocol))
    part.begin(a, m, o)
    part.quantum(0)
    lines, hist, pend = part.census()
    assert lines[own].sum() > 0 and not lines[~own].any() and not hist[~own].any()


# ---- what the GPU cases reach ---------------------------------------------

@pytest.mark.parametrize("name", R.A_AND_B + ["F_mosi_hbh_barriers"])
def test_small_directory_shapes_reach_the_hard_states(name):
    s = R.series(name)
    L, h = s.lines.sum(axis=1).astype(np.int64), s.hist.sum(axis=1).astype(np.int64)
    pend = s.pending.sum(axis=1)
    print(name, "samples", len(s.time), "with pending replaced entries", int((pend > 0).sum()),
          "most zero-sharer entries", int(h[:, 0].max()))
    assert (pend > 0).sum() >= 100                       # the replaced-list path, at many quantum ends
    assert h[:, 0].max() > 0                             # valid entries without a sharer
    assert np.any((L[:, 3] > 0) & (L[:, 1] % np.maximum(L[:, 3], 1) != 0))   # L1 / L2 shared ratio no integer
    assert np.all(s.repeat == 1) and np.array_equal(np.diff(s.q.astype(np.int64)) > 0, np.ones(len(s.q) - 1, bool))
    if "barriers" in name:
        assert int(((s.out & np.uint64(3)) == C.LVL_SYNC).sum()) == 16 * 4


@pytest.mark.parametrize("name", ["C_mosi", "C_msi"])
def test_two_sharer_words_shape(name):
    cfg, a, m, o, _ = R.shape(name)
    s = R.series(name)
    h = s.hist.sum(axis=1)
    assert cfg.num_tiles == 72 and h.shape[1] == 73
    assert np.flatnonzero(h[:, 1:].sum(axis=0))[-1] + 1 >= 12          # many sharers on an entry
    assert s.lines[:, 64:].sum() > 0                                    # tiles of the second sharer word hold lines


def test_gap_case_has_a_repeat_and_interval_cases_sample_sparsely():
    assert R.series("skipped_boundaries").repeat.max() > 1
    for name in sorted(R.TRACE_CASES):
        cfg, _, _, _, interval = R.shape(name)
        s = R.series(name)
        assert interval > cfg.quantum_ns and len(s.time) > 2 and np.all(s.time % np.uint64(interval) == 0)


def test_restore_case_has_a_pause_with_pending_entries():
    q, row = R.pause_quantum()
    s = R.series("A_mosi_hbh")
    assert s.pending[row].sum() > 0 and int(s.q[row]) + 1 == q and q % 4 != 0


def test_text_case_has_a_non_integer_degree():
    s = R.series("A_mosi_hbh_i4")
    L = s.lines.sum(axis=1).astype(np.int64)
    assert len(s.time) > 100
    assert np.any((L[:, 3] > 0) & (L[:, 1] % np.maximum(L[:, 3], 1) != 0))
