"""The case table of the pairwise sweep (tests/sweep_cases.py) on the CPU: it
covers every allowed pair of levels, holds no forbidden pair, the oracle runs
every row, and the rows provoke what their levels exist to provoke — computed
from the oracle's outputs, so that no row of tests/test_gpu_sweep.py passes
emptily."""
import functools
import math

import numpy as np
import pytest

from graphite_amd import config as C
from tests import sweep_cases as S

CC_EV = C.CACHE_COUNTERS.index("evictions")
OFF_GRID = ("1g5", "2g66", "0g75")
PRIVATE_L2 = ("msi", "mosi")


@functools.lru_cache(maxsize=None)
def oracle(index):
    """What the oracle gives for row `index` (computed once, read-only)."""
    from oracle import pyoracle as po
    cfg, a, m, o = S.build(S.CASES[index])
    oc = po.OracleCoherent(cfg)
    words = oc.run(a, m, o)
    r = dict(words=words, meta=m, offsets=o, stats=oc.tile_stats(), cache=oc.cache_counters(), net=oc.net_counters(),
             info=oc.run_info(), miss_types=oc.miss_types(), cfg=cfg)
    for v in r.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return r


def _info(r, key):
    return int(r["info"][C.RUN_INFO.index(key)])


# ---- the table ------------------------------------------------------------------
def test_every_allowed_pair_is_covered():
    covered = set()
    for c in S.CASES:
        covered |= S.pairs_of(c.labels)
    missing = sorted(S.all_pairs() - covered)
    assert not missing, "%d pairs in no case, first %s" % (len(missing), missing[:8])


def test_no_case_holds_a_forbidden_pair():
    for c in S.CASES:
        for a, b in S.CONSTRAINTS:
            assert S.LEVEL[a][0] != S.LEVEL[b][0]
            assert not (a in c.labels and b in c.labels), (c.id, a, b)


def test_table_is_well_formed():
    assert len({c.labels for c in S.CASES}) == len(S.CASES)
    assert len({c.id for c in S.CASES}) == len(S.CASES)
    for c in S.CASES:
        lines = np.diff(oracle(c.index)["offsets"].astype(np.int64)).max()
        if (S.level(c, "driver"), S.level(c, "quantum")) == ("win", "q10000"):
            cap = 2 * S.MAX_RECORDS             # (the one exception, explained above the table)
        else:
            cap = S.MAX_RECORDS_72 if S.level(c, "mesh") == "8x9k8" else S.MAX_RECORDS
        assert lines <= cap, (c.id, lines)
        if S.level(c, "driver") == "ens":       # its longest instance has 3 n / 2 accesses a tile
            longest = np.diff(S.trace(c, n=3 * c.n // 2)[2].astype(np.int64)).max()
            assert longest <= cap, (c.id, longest)


def test_generator_reproduces_the_table():
    """tools/sweep_pairs.py is deterministic and prints the committed rows."""
    import importlib.util
    import os
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools", "sweep_pairs.py")
    spec = importlib.util.spec_from_file_location("sweep_pairs", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    assert mod.generate() == [c.labels for c in S.CASES]


# ---- the oracle on every case ------------------------------------------------------
@pytest.mark.parametrize("case", S.CASES, ids=[c.id for c in S.CASES])
def test_oracle_runs_the_case(case):
    r = oracle(case.index)
    kind, driver = S.level(case, "trace"), S.level(case, "driver")
    assert len(r["words"]) == int(r["offsets"][-1]) > 0
    if driver in ("legs", "win"):
        assert _info(r, "final_quantum") >= 6
    cont = (r["meta"] & np.uint32(0x80000000) != 0) & (r["meta"] != np.uint32(C.META_BARRIER))
    barriers = r["meta"] == np.uint32(C.META_BARRIER)
    if kind == "multi":
        assert cont.sum() > r["cfg"].num_tiles
    else:
        assert not cont.any()
    if kind == "barr":
        released = ((r["words"] & np.uint64(3)) == np.uint64(C.LVL_SYNC)).sum()
        assert released == barriers.sum() and released > r["cfg"].num_tiles      # more than one release
    else:
        assert not barriers.any()
    if kind == "ragged":
        n = np.diff(r["offsets"].astype(np.int64))
        assert sorted(set(n.tolist())) == sorted(set(S.RAGGED(case.n)))


# ---- the levels that exist to provoke an event ----------------------------------------
def _l2_evictions(r):
    return int(r["cache"][:, 1, CC_EV].sum())


def _dir_evictions(r):
    return int(r["stats"][:, C.TILE_STATS.index("dir_evictions")].sum())


def _contention(r):
    return int(r["net"][:, C.NET_COUNTERS.index("total_contention_ps")].sum())


def _off_grid_latency(r):
    w = r["words"]
    acc = (w & np.uint64(3)) != np.uint64(C.LVL_SYNC)
    return int((((w[acc] >> np.uint64(2)) % np.uint64(1000)) != 0).sum())


EVENTS = {
    "small geometry: L2 evictions": (lambda c: S.level(c, "geometry") == "small", _l2_evictions),
    "small directory under a private L2: directory evictions":
        (lambda c: S.level(c, "directory") in ("d192", "d24") and S.level(c, "protocol") in PRIVATE_L2, _dir_evictions),
    "hop-by-hop with a router queue at 12 tiles or more: contention":
        (lambda c: S.level(c, "net") == "hbh" and S.level(c, "router_queue") != "rqoff"
         and S.config_kw(c)["num_tiles"] >= 12, _contention),
    "more than one shard: boundary messages":
        (lambda c: S.config_kw(c)["num_shards"] > 1, lambda r: _info(r, "boundary_msgs")),
    "miss types on: a miss-type count": (lambda c: S.level(c, "miss_types") != "mt0", lambda r: int(r["miss_types"].sum())),
    "an off-grid clock: a latency that is no multiple of 1000 ps":
        (lambda c: S.level(c, "clock") in OFF_GRID, _off_grid_latency),
}


@pytest.mark.parametrize("event", sorted(EVENTS))
def test_levels_provoke_their_event(event):
    carries, count = EVENTS[event]
    cases = [c for c in S.CASES if carries(c)]
    shown = [c for c in cases if count(oracle(c.index)) > 0]
    print(event, ":", len(shown), "of", len(cases), "cases")
    assert len(shown) >= max(3, math.ceil(2 * len(cases) / 3)), \
        [c.id for c in cases if c not in shown]


def test_l2_miss_types_are_counted_where_tracked():
    for c in S.CASES:
        if S.level(c, "miss_types") == "mt12":
            assert int(oracle(c.index)["miss_types"][:, 1].sum()) > 0, c.id


# ---- the excluded pairs ----------------------------------------------------------------
@pytest.mark.parametrize("proto", [C.PROTO_SHL2_MSI, C.PROTO_SHL2_MESI])
def test_oracle_refuses_shared_l2_with_l2_miss_types(proto):
    from oracle import pyoracle as po
    a, m, o = po.gen_trace(16, 50, hot_lines=8)
    ok = C.default_config(16, protocol=proto, l1d_track_miss_types=1, miss_track_lines=1024)
    po.OracleCoherent(ok).run(a, m, o)                       # L1 miss types alone are accepted
    bad = C.default_config(16, protocol=proto, l1d_track_miss_types=1, l2_track_miss_types=1, miss_track_lines=1024)
    with pytest.raises(RuntimeError):
        po.OracleCoherent(bad).run(a, m, o)


def test_one_shard_does_not_split_over_two_ranks():
    """(round2, one shard): the round's rule K % W == 0 with the ranks' ranges."""
    from graphite_amd import coherent as CO
    assert 1 % 2 != 0
    for c in S.CASES:
        if S.level(c, "driver") == "round2":
            K = S.config_kw(c)["num_shards"]
            ranges = [CO.shard_range(r, 2, K) for r in range(2)]
            assert ranges[0][0] == 0 and ranges[0][1] == ranges[1][0] and ranges[1][1] == K
            assert all(b > a for a, b in ranges), (c.id, ranges)
