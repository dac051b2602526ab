"""The adversarial NoC traffic of tests/noc_traffic.py on the CPU: every case
reaches the branch of gg_noc.hip it is named after (by the numpy predicates
and the thresholds read from the sources), the oracle routes it, and it does
not pass emptily (contention where a queue model is on, >= 90 % of the packets
with dst != src, packets on both sides of every edge).  The GPU comparison of
the same cases is tests/test_gpu_noc_traffic.py."""
import functools

import numpy as np
import pytest

from graphite_amd import config as C
from oracle import pyoracle as po
import netgen_model as M
import noc_traffic as NT

TH = NT.thresholds()


# ---- the thresholds come from the sources ---------------------------------------------------------
def test_thresholds_are_read_from_the_sources():
    for name in NT.THRESHOLD_NAMES + ("kFlitBound",):
        assert TH[name] > 0, name
    assert TH["kPipePk"] <= TH["kSweepPk"], "a chain the pipeline refuses for its size goes past the sweep's body too"
    assert NT.qimg_bytes(100) == TH["HQueueBytes"] + 100 * TH["HNodeBytes"]


def test_missing_threshold_name_fails_loudly(tmp_path):
    text = "constexpr uint32_t kPipePos = 32, kPipeK = 2, kPipeBatch = 256;\nconstexpr size_t kOther = 160 * 1024 - 64;\n"
    assert NT.read_constant("kPipeBatch", (text,)) == 256 and NT.read_constant("kPipePos", (text,)) == 32
    assert NT.read_constant("kOther", (text,)) == 160 * 1024 - 64
    with pytest.raises(KeyError, match="kSweepPk"):
        NT.read_constant("kSweepPk", (text,))
    # a source tree without one of the names: thresholds() as a whole fails
    for f in ("gg_noc.hip", "gg_noc_stage.h", "gg_dev.h"):
        with open(NT.CSRC + "/" + f) as fh:
            (tmp_path / f).write_text(fh.read().replace("kPortPk", "kPortPackets"))
    with pytest.raises(KeyError, match="kPortPk"):
        NT.thresholds(str(tmp_path))


# ---- the predicates on batches small enough to check by hand --------------------------------------
def test_predicates_on_a_hand_made_batch():
    T = 16                                              # 4 x 4: tile = y * 4 + x
    src = np.array([0, 0, 5, 15, 3, 9, 16, 2], np.uint32)
    dst = np.array([3, 12, 5, 0, 1, 11, 1, 99], np.uint32)   # 5 -> 5 is self; 16 and 99 are no tiles
    assert NT.xchain_ids(T, src, dst).tolist() == [1, -1, -1, 6, 0, 5, -1, -1]
    assert NT.ychain_ids(T, src, dst).tolist() == [-1, 1, -1, 0, -1, -1, -1, -1]
    assert NT.per_source(T, src, dst).tolist() == [2, 0, 0, 1, 0, 0, 0, 0, 0, 1, 0, 0, 0, 0, 0, 1]
    assert NT.per_destination(T, src, dst)[[0, 1, 3, 11, 12]].tolist() == [1, 1, 1, 1, 1]
    assert NT.per_xchain(T, src, dst).tolist() == [1, 1, 0, 0, 0, 1, 1, 0]
    assert NT.per_ychain(T, src, dst).tolist() == [1, 1, 0, 0, 0, 0, 0, 0]
    cfg = C.default_config(T, net_model=C.NET_EMESH_HOP_BY_HOP, queue_model_enabled=0)
    # 0 -> 3 at 0 ps and 1 -> 3 at -2000 ps + one hop: both ask (row 0 rightwards, position 1) at 2000 ps
    s2, d2 = np.array([0, 1, 1], np.uint32), np.array([3, 3, 2], np.uint32)
    assert NT.max_equal_time_at_position(cfg, s2, d2, np.array([0, 2000, 2000], np.uint64)) == 3
    assert NT.max_equal_time_at_position(cfg, s2, d2, np.array([0, 2000, 2001], np.uint64)) == 2
    assert NT.max_equal_time_at_position(cfg, s2, d2, np.array([1, 2000, 2002], np.uint64)) == 1
    assert NT.lat_to_ps(2, 1.0) == 2000 and NT.lat_to_ps(2, 1.5) == 1334
    assert NT.max_start_load(T, src, dst) == 1 and NT.max_start_load(T, s2, d2) == 2


# ---- every case of the table -----------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def oracle_answer(name):
    k, cfg = NT.case(name), NT.case_config(name)
    on = po.OracleNoc(cfg)
    out = on.route_tree(*k["batch"])[0] if k["tree"] else on.route(*k["batch"])
    return out, on.counters()


def _all(paths, what):
    return len(paths) > 0 and set(paths.values()) == {what}


def check_reach(name):
    """The case reaches the branch it is named after."""
    k, cfg = NT.case(name), NT.case_config(name)
    T, (src, dst, bits, t), r = k["T"], k["batch"], k["reaches"]
    w, h = NT.mesh(T)
    if k["tree"]:
        nb = int((dst == C.BROADCAST).sum())
        if r == "tree_sync":
            assert nb == T and sorted(src[dst == C.BROADCAST].tolist()) == list(range(T))
            assert len(src) - nb == 200 and len(np.unique(t)) == 1
        else:
            assert (dst[::20] == C.BROADCAST).all() and nb == len(dst[::20]) and (dst[dst != C.BROADCAST] == 0).all()
        return
    px, py = NT.chain_paths(cfg, src, dst, bits)
    kern = NT.chain_kernel(cfg)
    if r == "sweep":
        assert kern == ("sweep", "sweep") and max(w, h) > TH["kPipePos"]
        assert _all(px, "sweep") and _all(py, "sweep")              # the body of chain_sweep, both stages
        if name == "side32x33":
            assert w <= TH["kPipePos"] < h
    elif r in ("sweep_last", "sweep_over"):
        n = TH["kSweepPk"] + (r == "sweep_over")
        assert kern[0] == "sweep" and list(px) == [1] and NT.per_xchain(T, src, dst)[1] == n == len(src)
        assert px[1] == ("sweep" if r == "sweep_last" else "staged")
    elif r == "hbm":
        assert kern == ("hbm", "hbm") and _all(px, "hbm") and _all(py, "hbm")
        if name != "hbm_side100":
            assert max(w, h) <= TH["kPipePos"], "only the list size sends this mesh to k_chain"
        else:
            assert cfg.max_list_size == 100 and cfg.queue_model_type == C.QM_HISTORY_TREE
    elif r in ("pipe_last", "pipe_over"):
        n = TH["kPipePk"] + (r == "pipe_over")
        assert kern[0] == "pipe" and list(px) == [1] and NT.per_xchain(T, src, dst)[1] == n == len(src)
        assert (px[1] == "pipe") == (r == "pipe_last")
    elif r in ("port_last", "port_over"):
        n = TH["kPortPk"] + (r == "port_over")
        ps, pd = NT.per_source(T, src, dst), NT.per_destination(T, src, dst)
        assert ps[1] == n and pd[T - 2] == n
        assert np.delete(ps, 1).max() < TH["kPortPk"] and np.delete(pd, T - 2).max() < TH["kPortPk"]
    elif r == "hot_dst":
        assert NT.per_destination(T, src, dst)[0] > TH["kPortPk"]
        assert set(py) <= {0, 1} and 1 not in py and _all(py, "pipe")      # one loaded Y chain (column 0, downwards)
    elif r == "hot_src":
        assert NT.per_source(T, src, dst)[T - 1] > TH["kPortPk"] and np.count_nonzero(NT.per_source(T, src, dst)) == 1
        assert _all(px, "pipe") and set(px) <= {2 * (h - 1), 2 * (h - 1) + 1}
    elif r == "sync":
        assert len(np.unique(t)) == 1 and _all(px, "pipe") and _all(py, "pipe")
    elif r == "index_bisection":
        assert not cfg.queue_model_enabled and _all(px, "pipe") and _all(py, "pipe")
        assert NT.max_equal_time_at_position(cfg, src, dst, t) > TH["kPipeBatch"]
    elif r == "time_bisection":
        assert _all(px, "pipe") and _all(py, "pipe")
        first = t < (1 << 40)
        assert 0 < first.sum() < len(t)
        # a start pool of the first burst beyond the batch, all of it inside the first slab: the slab width
        # of a chain is about (its time range) / (its packets / 64), here >= 2^40 ps, and the first burst is
        # over after the ~10^7 ps its packets queue for (the oracle's contention below)
        assert NT.max_start_load(T, src, dst, first) > TH["kPipeBatch"]
        xc = NT.xchain_ids(T, src, dst)
        for c in px:
            tc = t[xc == c].astype(np.int64)
            assert (tc.max() - tc.min()) // max(1, len(tc) // 64) >= 1 << 40
        assert int(oracle_answer(name)[0][2][first].max()) < 1 << 36
    elif r in ("unordered", "descending"):
        d = np.diff(t.astype(np.int64))
        assert ((d <= 0).all() and (d < 0).any()) if r == "descending" else 0.4 < (d < 0).mean() < 0.6
    elif r == "ties":
        assert (t % 1000 == 0).all() and int(t.max()) < 400_000_000
        assert len(t) - len(np.unique(t)) > 1000                    # equal times, by the thousand
        zps = NT.lat_to_ps(cfg.router_delay + cfg.link_delay, cfg.frequency_ghz)
        assert (zps == 0) == (name == "cycle_ties_zero_delay")
    elif r == "giant":
        nf = NT.nflits(bits, cfg.flit_width)
        B = TH["kFlitBound"]
        assert (nf == B - 1).sum() == 2 and (nf == B).sum() == 2 and (nf > B).sum() == 0
        xc, yc = NT.xchain_ids(T, src, dst), NT.ychain_ids(T, src, dst)
        for ids, paths in ((xc, px), (yc, py)):
            at, below = set(ids[nf == B].tolist()), set(ids[nf == B - 1].tolist())
            assert -1 not in at | below and not at & below
            assert all(paths[c] == "staged" for c in at) and all(paths[c] == "pipe" for c in below)
            assert sum(v == "pipe" for v in paths.values()) > len(below)
    else:
        raise AssertionError("unknown branch %r" % r)


@pytest.mark.parametrize("name", list(NT.CASES))
def test_case_reaches_its_branch_and_is_not_empty(name):
    k, cfg = NT.case(name), NT.case_config(name)
    src, dst, bits, t = k["batch"]
    check_reach(name)
    (arr, zl, ct), counters = oracle_answer(name)
    assert NT.non_self_fraction(src, dst) >= 0.9
    if cfg.queue_model_enabled:
        assert int(ct.sum()) > 0
    else:
        assert int(ct.sum()) == 0
    uni = (src != dst) & (dst != C.BROADCAST)
    assert (arr[uni] > t[uni]).all()


def test_every_case_stays_in_the_models_domain():
    """No queue delay of any case leaves the range in which cycles -> ps is defined (1000 * cycles < 2^64):
    beyond it the reference's own cast is undefined and the oracle is no reference."""
    K = {n: i for i, n in enumerate(C.NET_COUNTERS)}
    for name in NT.CASES:
        (arr, zl, ct), counters = oracle_answer(name)
        uni = NT.case(name)["batch"][1] != C.BROADCAST
        assert int(ct[uni].max()) < 1 << 53 and int(arr[uni].max()) < 1 << 53, name
        assert int(counters[:, K["router_contention_cycles"]].max()) < 1 << 50, name


def test_all_at_cycle_0_with_the_analytical_model_is_outside_the_domain():
    """Why sync_t0 runs with analytical_enabled = 0.  Four requests at cycle 0 on one port: the first three
    take the head of the first interval, so the fourth lies before it and asks QueueModelMG1 with n = 3,
    sum 11, newest 11: the arrival rate 3 / 11 and the service rate 1 / (11 / 3) differ by one ulp and the
    delay is ~1.8e16 cycles, beyond 2^64 ps.  One request at any later cycle keeps [0, t) at the head."""
    h = po.OracleHistoryTree(1, 100, True)
    assert [h.delay(0, p) for p in (1, 1, 9)] == [0, 1, 2]
    assert h.delay(0, 1) * 1000 >= 1 << 64
    h = po.OracleHistoryTree(1, 100, True)
    assert [h.delay(5, p) for p in (1, 1, 9, 1)] == [0, 1, 2, 11] and h.analytical_requests == 0
    for name in NT.CASES:
        if name.startswith("sync_t0"):
            assert NT.case_config(name).analytical_enabled == 0 and not NT.case(name)["batch"][3].any()
        else:
            assert NT.case_config(name).analytical_enabled == 1


def test_branches_the_table_must_cover():
    """chain_sweep's body, k_chain and the pipeline's index bisection each have a case."""
    reached = {NT.case(n)["reaches"] for n in NT.CASES}
    assert {"sweep", "sweep_last", "hbm", "index_bisection", "time_bisection", "giant"} <= reached


# ---- the synthetic generator's cases (tests/netgen_model.py) ---------------------------------------
SYNC_LARGE = {"8x8": (64, 65536), "32x32": (1024, 1024)}
SYNTH_LOAD1 = [(T, p) for T in (16, 64) for p in ("bit_complement", "shuffle", "nearest_neighbor")]


@functools.lru_cache(maxsize=None)
def sync_large_packets(which):
    """transpose, load 1.0, one packet per tile, all at cycle 0: (cfg, batch)."""
    T, packet_bytes = SYNC_LARGE[which]
    cfg = C.default_config(T, net_model=C.NET_EMESH_HOP_BY_HOP)
    return cfg, M.generate("transpose", T, 1, 1.0, packet_bytes, cfg.frequency_ghz, seed=T)[:4]


@functools.lru_cache(maxsize=None)
def synth_load1(T, pattern):
    cfg = C.default_config(T, net_model=C.NET_EMESH_HOP_BY_HOP)
    return cfg, M.generate(pattern, T, 64, 1.0, 8, cfg.frequency_ghz, seed=T)[:4]


@pytest.mark.parametrize("which", list(SYNC_LARGE))
def test_sync_large_packets_is_the_slab_collapse(which):
    """Every packet of every chain starts at one instant (slab width 1 ps) and the chains drain for far
    longer than the 2^24 steps a 1 ps slab would allow (8 x 8), or for millions of them (32 x 32)."""
    cfg, (src, dst, bits, t) = sync_large_packets(which)
    T = cfg.num_tiles
    w, _ = NT.mesh(T)
    assert len(np.unique(t)) == 1
    # the transpose's diagonal sends to itself: 1 tile in `side`, by construction (8 x 8: 87.5 % travel)
    assert int((src != dst).sum()) == T - w
    nf = NT.nflits(bits, cfg.flit_width)
    assert (nf < TH["kFlitBound"]).all() and (nf == nf[0]).all()
    px, py = NT.chain_paths(cfg, src, dst, bits)
    assert _all(px, "pipe") and _all(py, "pipe")
    assert NT.per_xchain(T, src, dst).max() > 1                      # somebody waits
    ct = po.OracleNoc(cfg).route(src, dst, bits, t)[2]
    assert int(ct.max()) > (1 << 24 if which == "8x8" else 1 << 21)  # ps = steps of a 1 ps slab


@pytest.mark.parametrize("T,pattern", SYNTH_LOAD1)
def test_synth_load1_sends_every_cycle(T, pattern):
    cfg, (src, dst, bits, t) = synth_load1(T, pattern)
    assert (t.reshape(T, 64) == np.arange(64, dtype=np.uint64) * np.uint64(1000)).all()
    # the shuffle's two fixed points (tiles 0 and T - 1) send to themselves: 87.5 % travel at T = 16
    assert set(np.unique(src[src == dst]).tolist()) == ({0, T - 1} if pattern == "shuffle" else set())
    assert int(po.OracleNoc(cfg).route(src, dst, bits, t)[2].sum()) > 0
