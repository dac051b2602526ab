"""The private-cache replay on every geometry of tests/cache_geometry_cases.py,
under every replay_kernel, against the CPU oracle: results, evicted addresses,
counters and final state bit for bit, with the kernel that ran witnessed by its
timer.  Then the quartet on geometries no fixture has, output pointers that
are not 16-byte aligned on the sharded path, and the geometries gg_create
rejects."""
import functools

import numpy as np
import pytest

from graphite_amd import config as C
from graphite_amd import backend as B
from oracle import pyoracle as po
import cache_geometry_cases as G
from gpu_util import torch_dev, to_dev, to_np

pytestmark = pytest.mark.gpu
LRU, RR = C.POLICY_LRU, C.POLICY_ROUND_ROBIN
INV = 0xFFFFFFFFFFFFFFFF
CASES = {c.name: c for c in G.CASES}


def info(li):
    return (li.tag, li.cstate, li.cached_loc)


@functools.lru_cache(maxsize=None)
def reference(name):
    """The oracle's side of a row, computed once: trace, results, evicted
    addresses, counters, and the final LineInfo at both levels of 256 sampled
    trace addresses (the pinned-line phase included) and 64 fresh ones."""
    case = CASES[name]
    addr, meta, offs = G.build_trace(case, 1)
    oc = po.OracleCache(G.config(case))
    res, ev = oc.run(addr, meta, offs, want_evicted=True)
    cnt = oc.counters().copy()
    rng = np.random.default_rng(3)
    tile_of = np.repeat(np.arange(case.tiles), np.diff(offs.astype(np.int64)))
    tail = np.concatenate([np.arange(int(offs[t + 1]) - 2 * case.l2_assoc - 3, int(offs[t + 1]))
                           for t in range(case.tiles) if offs[t + 1] > offs[t]])
    idx = np.concatenate([tail[:64], rng.integers(0, len(addr), 256 - min(64, len(tail)))])
    probes = [(int(tile_of[i]), int(addr[i])) for i in idx] + G.fresh_addresses(case, 64, 5)
    infos = [(info(oc.get_line_info(t, C.L1D, a)), info(oc.get_line_info(t, C.L2, a))) for t, a in probes]
    return case, addr, meta, offs, res, ev, cnt, probes, infos


def replay_in_batches(be, torch, T, addr, meta, offs, chunks=2):
    """Every tile's records in `chunks` consecutive batches (state persists)."""
    n = len(addr)
    res = np.zeros(n, np.uint32)
    ev = np.zeros(n, np.uint64)
    cuts = [[int(offs[t]) + (int(offs[t + 1]) - int(offs[t])) * k // chunks for k in range(chunks + 1)]
            for t in range(T)]
    for k in range(chunks):
        idx = np.concatenate([np.arange(cuts[t][k], cuts[t][k + 1]) for t in range(T)]).astype(np.int64)
        sub_off = np.zeros(T + 1, np.uint64)
        for t in range(T):
            sub_off[t + 1] = sub_off[t] + (cuts[t][k + 1] - cuts[t][k])
        r = torch.zeros(len(idx), dtype=torch.int32, device="cuda")
        e = torch.zeros(len(idx), dtype=torch.int64, device="cuda")
        be.cache_access_batch(to_dev(torch, addr[idx], torch.int64), to_dev(torch, meta[idx], torch.int32), sub_off, r, e)
        torch.cuda.synchronize()
        res[idx] = to_np(r, np.uint32)
        ev[idx] = to_np(e, np.uint64)
    return res, ev


@pytest.mark.parametrize("kern", [0, 1, 2])
@pytest.mark.parametrize("name", list(CASES))
def test_geometry_matches_oracle(name, kern):
    torch = torch_dev()
    case, addr, meta, offs, ref, ref_ev, ref_cnt, probes, ref_infos = reference(name)
    be = B.Backend(G.config(case, replay_kernel=kern))
    be.set_timing(True)
    res, ev = replay_in_batches(be, torch, case.tiles, addr, meta, offs)
    np.testing.assert_array_equal(res, ref)
    np.testing.assert_array_equal(ev, ref_ev)
    np.testing.assert_array_equal(be.cache_counters(), ref_cnt)
    # the path that ran: k_cache_stream exactly for the rows the dispatch rule streams
    streams = kern == 0 and case.stream
    t_stream, t_replay = be.kernel_time_ms("cache_stream"), be.kernel_time_ms("cache_replay")
    print("%s replay_kernel=%d cache_stream %.3f ms cache_replay %.3f ms" % (name, kern, t_stream, t_replay))
    assert (t_stream >= 0) == streams
    assert (t_replay >= 0) == (not streams)
    if kern == 0:                                          # final state (each probe is a launch)
        got = [(info(be.get_line_info(t, C.L1D, a)), info(be.get_line_info(t, C.L2, a))) for t, a in probes]
        assert got == ref_infos
    be.close()


QUARTET_GEOMS = {
    "a1_1": dict(l1d_size_kb=1, l1d_assoc=1, l2_size_kb=8, l2_assoc=8),
    "8_16": dict(l1d_size_kb=4, l1d_assoc=8, l2_size_kb=32, l2_assoc=16),
    "4_2": dict(l1d_size_kb=2, l1d_assoc=4, l2_size_kb=2, l2_assoc=2),
    "4_32": dict(l1d_size_kb=2, l1d_assoc=4, l2_size_kb=32, l2_assoc=32),
    "line128": dict(l1d_size_kb=4, l1d_assoc=4, l2_size_kb=16, l2_assoc=8, line_size=128),
    "rr_lru": dict(l1d_size_kb=2, l1d_assoc=4, l1d_policy=RR, l2_size_kb=8, l2_assoc=8),
    "lru_rr": dict(l1d_size_kb=2, l1d_assoc=4, l2_size_kb=8, l2_assoc=8, l2_policy=RR),
}


def quartet_walk(be, be_info, oc, cfg, level):
    """200 + 12 x assoc seeded operations on the lines of one set of tile 0
    (assoc + max(3, assoc / 2) of them, so inserts evict) and three lines of
    another set of tile 1, on `be` and the oracle `oc` side by side.  Every
    step reads the
    line's LineInfo on both (a get), then with p = 0.15 / 0.2 / 0.5 sets it
    (INVALID with the invalid tag, or a valid state), accesses it, or inserts
    it where absent (accesses it where present).  Returns (sets, accesses,
    failed calls, inserts, evictions) so the caller can see the walk was not
    vacuous."""
    line = cfg.line_size
    assoc = cfg.l1d_assoc if level == C.L1D else cfg.l2_assoc
    sets = (cfg.l1d_size_kb if level == C.L1D else cfg.l2_size_kb) * 1024 // (assoc * line)
    rng = np.random.default_rng(17 + level)
    pool = [(((k + 1) * sets + sets - 1) * line + int(rng.integers(0, line)), 0) for k in range(assoc + max(3, assoc // 2))]
    pool += [((k * sets + sets // 2) * line + int(rng.integers(0, line)), 1) for k in range(3)]
    states = [C.CSTATE_INVALID, C.CSTATE_SHARED, C.CSTATE_MODIFIED]
    n_set = n_acc = n_fail = n_ins = n_ev = 0
    for step in range(200 + 12 * assoc):
        a, t = pool[int(rng.integers(0, len(pool)))]
        tag = a // line
        present = info(oc.get_line_info(t, level, a))
        assert info(be.get_line_info(t, level, a)) == present, step
        assert present[0] in (INV, tag)
        x = rng.random()
        loc = int(rng.choice([C.LOC_INVALID, C.LOC_L1D])) if level == C.L2 else 0
        if x < 0.15:                                       # the get above
            continue
        if x < 0.3:                                        # setCacheLineInfo (fails on an absent line)
            st = int(rng.choice(states))
            li = (INV, st, 0) if st == C.CSTATE_INVALID else (tag, st, loc)
            rc = oc.set_line_info(t, level, a, po.LineInfo(*li))
            assert be.set_line_info(t, level, a, be_info(*li)) == rc, step
            n_set += 1
            n_fail += rc != 0
        elif x < 0.5 or present[0] != INV:                 # accessCacheLine (fails on an absent line)
            wr = bool(rng.integers(0, 2))
            rc = oc.access_line(t, level, a, wr)
            assert be.access_line(t, level, a, wr) == rc, step
            n_acc += 1
            n_fail += rc != 0
        else:                                              # insertCacheLine of an absent line
            li = (tag, int(rng.choice(states[1:])), loc)
            g = be.insert_line(t, level, a, be_info(*li))
            o = oc.insert_line(t, level, a, po.LineInfo(*li))
            assert g[:3] == o[:3] and info(g[3]) == info(o[3]), step
            assert o[0] == 0
            n_ins += 1
            n_ev += o[1]
    for a, t in pool:                                      # final state of every line of the pool
        assert info(be.get_line_info(t, level, a)) == info(oc.get_line_info(t, level, a))
    return n_set, n_acc, n_fail, n_ins, n_ev


@pytest.mark.parametrize("geom", list(QUARTET_GEOMS))
@pytest.mark.parametrize("level", [C.L1D, C.L2])
def test_quartet_matches_oracle(geom, level):
    """The Cache quartet on geometries no reference fixture has, GPU and
    oracle side by side: equal return codes, LineInfo, eviction flag and
    evicted address at every step."""
    torch_dev()
    cfg = C.default_config(2, **QUARTET_GEOMS[geom])
    be = B.Backend(cfg)
    n_set, n_acc, n_fail, n_ins, n_ev = quartet_walk(be, B.LineInfo, po.OracleCache(cfg), cfg, level)
    print("%s level %d: %d sets %d accesses %d failed %d inserts %d evictions" % (geom, level, n_set, n_acc, n_fail, n_ins, n_ev))
    assoc = cfg.l1d_assoc if level == C.L1D else cfg.l2_assoc
    assert n_set >= 20 and n_acc >= 20 and n_fail >= 3 and n_ins > assoc and n_ev >= 3
    be.close()


@pytest.mark.parametrize("aligned", [False, True])
def test_sharded_outputs_unaligned_and_ragged_tail(aligned):
    """k_unshard takes its vector path from the alignment of result / evicted
    and n: results at [1 : n + 1] of guard-filled buffers (4 and 8 bytes off a
    16-byte boundary), and aligned outputs with n off a multiple of 4096 (a
    vector body and a scalar tail).  Guard words on both sides stay untouched."""
    torch = torch_dev()
    T = 4
    cfg = C.default_config(T, replay_kernel=1, l2_size_kb=128)      # 2048 L2 lines under 8192 of footprint: evictions
    lens = [5000, 0, 4096, 3 * 4096 + 1234 - 5000]
    n = sum(lens)
    assert n >= 3 * 4096 and n % 4096
    parts = [po.gen_uniform(t, 11 * t, lens[t], lines_log2=13) for t in range(T)]
    addr = np.concatenate([p[0] for p in parts])
    meta = np.concatenate([p[1] for p in parts])
    offs = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)
    oc = po.OracleCache(cfg)
    ref, ref_ev = oc.run(addr, meta, offs, want_evicted=True)
    assert int(((ref & C.RES_L2_EVICT) != 0).sum()) > 100
    lo = 4 if aligned else 1
    GR, GE = 0x5A5A5A5A, 0x5A5A5A5A5A5A5A5A
    big_r = torch.full((n + 64,), GR, dtype=torch.int32, device="cuda")
    big_e = torch.full((n + 64,), GE, dtype=torch.int64, device="cuda")
    r, e = big_r[lo:lo + n], big_e[lo:lo + n]
    assert (r.data_ptr() % 16 == 0) == aligned and (e.data_ptr() % 16 == 0) == aligned
    be = B.Backend(cfg)
    be.set_timing(True)
    be.cache_access_batch(to_dev(torch, addr, torch.int64), to_dev(torch, meta, torch.int32), offs, r, e)
    torch.cuda.synchronize()
    assert be.kernel_time_ms("cache_unshard") >= 0 and be.kernel_time_ms("cache_stream") < 0
    got_r, got_e = to_np(big_r, np.uint32), to_np(big_e, np.uint64)
    np.testing.assert_array_equal(got_r[lo:lo + n], ref)
    np.testing.assert_array_equal(got_e[lo:lo + n], ref_ev)
    assert np.all(got_r[:lo] == GR) and np.all(got_r[lo + n:] == GR)
    assert np.all(got_e[:lo] == GE) and np.all(got_e[lo + n:] == GE)
    np.testing.assert_array_equal(be.cache_counters(), oc.counters())
    be.close()


REJECTED = [
    ("no_instance", dict(l1d_size_kb=16, l1d_assoc=8, l1d_policy=RR, l2_size_kb=256, l2_assoc=8, l2_policy=RR),
     "no replay kernel instantiated"),
    ("lds_bound", dict(l1d_size_kb=8, l1d_assoc=4, l2_size_kb=512, l2_assoc=8), "too large for the LDS"),       # s2 = 32
    ("l1_sets_2048", dict(l1d_size_kb=512, l1d_assoc=4, l2_size_kb=1024, l2_assoc=8), "more than 1024 L1-D sets"),
    ("l2_fewer_sets", dict(l1d_size_kb=32, l1d_assoc=4, l2_size_kb=32, l2_assoc=8), "L2 sets >= L1-D sets"),
    ("l1_sets_96", dict(l1d_size_kb=24, l1d_assoc=4), "powers of two"),
    ("l1_assoc_16", dict(l1d_size_kb=32, l1d_assoc=16), "associativity beyond 8"),
    ("l2_assoc_64", dict(l2_size_kb=512, l2_assoc=64), "associativity beyond 8"),
]


@pytest.mark.parametrize("name,kw,cause", REJECTED, ids=[r[0] for r in REJECTED])
def test_unsupported_geometry_is_rejected_at_create(name, kw, cause):
    torch = torch_dev()
    with pytest.raises(B.GGError) as ei:
        B.Backend(C.default_config(4, **kw))
    assert ei.value.code == -3                                      # GG_ERR_UNSUPPORTED
    assert cause in str(ei.value)
    # a default-config context created afterwards still works
    T, N = 4, 600
    cfg = C.default_config(T)
    parts = [po.gen_uniform(t, 0, N, lines_log2=12) for t in range(T)]
    addr, meta = np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts])
    offs = np.arange(T + 1, dtype=np.uint64) * np.uint64(N)
    be = B.Backend(cfg)
    r = torch.zeros(T * N, dtype=torch.int32, device="cuda")
    be.cache_access_batch(to_dev(torch, addr, torch.int64), to_dev(torch, meta, torch.int32), offs, r)
    torch.cuda.synchronize()
    np.testing.assert_array_equal(to_np(r, np.uint32), po.OracleCache(cfg).run(addr, meta, offs))
    be.close()
