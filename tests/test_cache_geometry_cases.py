"""The private-cache geometry table (tests/cache_geometry_cases.py) against the
instantiation lists of gg_cache.hip, the checks of gg_create and the oracle.
No GPU: tests/test_gpu_cache_geometry.py runs the rows on the card."""
import functools
import os
import re

import numpy as np
import pytest

from graphite_amd import config as C
from oracle import pyoracle as po
import cache_geometry_cases as G

SRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "graphite_amd", "csrc", "gg_cache.hip")
LRU, RR = C.POLICY_LRU, C.POLICY_ROUND_ROBIN
RES_BITS = ["RES_L1_MISS", "RES_L2_MISS", "RES_L1_INVAL", "RES_L1_EVICT", "RES_L2_EVICT", "RES_L2_EVICT_DIRTY",
            "RES_L2_EVICT_INV_L1", "RES_UPGRADE"]
K_RING = 32              # GG_RING of gg_cache.hip


def instantiations(text=None):
    """{macro: [argument tuples]} of the GG_KERN / GG_LEAN / GG_STREAM /
    GG_STREAM_MT uses in gg_cache.hip (the #define lines take macro parameters,
    not integers, and do not match)."""
    if text is None:
        with open(SRC) as f:
            text = f.read()
    out = {"GG_KERN": [], "GG_LEAN": [], "GG_STREAM": [], "GG_STREAM_MT": []}
    for name, args in re.findall(r"\b(GG_KERN|GG_LEAN|GG_STREAM_MT|GG_STREAM)\(\s*(\d+(?:\s*,\s*\d+)*)\s*\)", text):
        out[name].append(tuple(int(x) for x in args.split(",")))
    return out


def missing_rows(inst, cases):
    """Instantiations no row of `cases` dispatches to."""
    def pol(case):
        return (1 if case.l1d_policy == LRU else 0, 1 if case.l2_policy == LRU else 0)
    missing = []
    for name, entries in inst.items():
        for e in entries:
            rows = [c for c in cases if (c.l1d_assoc, c.l2_assoc) + pol(c) == e[:4]]
            if name in ("GG_STREAM", "GG_STREAM_MT"):
                rows = [c for c in rows if c.u1 == 64 * e[4] and c.stream]
            if not rows:
                missing.append((name, e))
    return missing


def replay_lds_bytes(case):
    """replay_lds_bytes(g, false) of gg_cache.hip: the generic replay's LDS."""
    tq, mw = (case.l2_assoc + 3) // 4, (case.l2_assoc + 7) // 8
    return case.s2 * 64 * (tq * 16 + mw * 8 + (0 if case.l2_policy == LRU else 1))


def stream_lds_bytes(case):
    tq = (case.l2_assoc + 3) // 4
    return (case.s2 * case.u1 * (tq * 16 + (16 if case.l2_assoc > 8 else 8)) + K_RING * case.u1 * 8 +
            case.u1 * 12 + 16 + case.u1 * 8 + case.u1 * 4)


def test_source_lists_parse_to_their_sizes():
    inst = instantiations()
    assert [len(inst[k]) for k in ("GG_KERN", "GG_LEAN", "GG_STREAM", "GG_STREAM_MT")] == [18, 8, 12, 2]
    assert all(len(e) == 4 for e in inst["GG_KERN"] + inst["GG_LEAN"])
    assert all(len(e) == 5 for e in inst["GG_STREAM"] + inst["GG_STREAM_MT"])


def test_every_instantiation_has_a_row():
    assert missing_rows(instantiations(), G.CASES) == []


def test_coverage_check_notices_a_missing_row_and_a_new_instantiation():
    inst = instantiations()
    without = [c for c in G.CASES if c.name != "u256_s8"]
    assert missing_rows(inst, without) == [("GG_STREAM", (4, 8, 1, 1, 4))]
    without = [c for c in G.CASES if c.name != "k8_4_ll"]
    assert missing_rows(inst, without) == [("GG_KERN", (8, 4, 1, 1))]
    with open(SRC) as f:
        text = f.read()
    more = instantiations(text + "\n  GG_KERN(2, 2, 1, 1), GG_STREAM(4, 8, 1, 1, 8),\n")
    assert missing_rows(more, G.CASES) == [("GG_KERN", (2, 2, 1, 1)), ("GG_STREAM", (4, 8, 1, 1, 8))]


def test_names_are_unique_and_required_rows_are_present():
    names = [c.name for c in G.CASES]
    assert len(set(names)) == len(names)
    by = {c.name: c for c in G.CASES}
    lru48 = [c for c in G.CASES if (c.l1d_assoc, c.l2_assoc, c.l1d_policy, c.l2_policy) == (4, 8, LRU, LRU)]
    have = {(c.u1, c.s2, c.stream) for c in lru48}
    # u1 on (4,8,LRU): 64 (ncw 1), 256 with s2 8 (ncw 4) and 16 (LDS fallback), 512, 1024 with s2 1, 1 and 2
    assert {(64, 2, True), (256, 8, True), (256, 16, False), (1024, 1, False)} <= have
    assert {u for u, _, _ in have} >= {1, 2, 64, 128, 256, 512, 1024}
    assert by["u1"].line_size == 256 and (by["u1"].l1d_size_kb, by["u1"].l1d_assoc) == (1, 4)
    # s2 at the ends the 64 KiB bound admits
    assert {(c.l2_assoc, c.s2) for c in G.CASES} >= {(8, 1), (8, 16), (32, 4), (4, 32)}
    for a2, s2 in ((8, 16), (32, 4), (4, 32)):
        c = next(c for c in G.CASES if (c.l2_assoc, c.s2) == (a2, s2))
        assert replay_lds_bytes(c._replace(s2=2 * s2)) > 64 * 1024
    # line sizes 32 and 128, streaming and sharded-only
    assert {(c.line_size, c.stream) for c in G.CASES} >= {(32, True), (32, False), (128, True), (128, False)}
    # u1 < 64: the units do not fill the last wave
    assert all((c.tiles * c.u1) % 64 for c in G.CASES if c.u1 < 64)
    assert all(c.tiles >= 2 for c in G.CASES)            # room for the empty tile


@pytest.mark.parametrize("case", G.CASES, ids=lambda c: c.name)
def test_row_is_valid_and_its_path_follows_the_dispatch_rule(case):
    """The checks gg_create / gg_cache_state_alloc make, restated, and the
    hand-derived `stream` flag against the dispatch rule of gg_cache_run_batch."""
    inst = instantiations()
    l1_sets, l2_sets = G.geometry(case)
    assert l1_sets * case.l1d_assoc * case.line_size == case.l1d_size_kb * 1024
    assert l2_sets * case.l2_assoc * case.line_size == case.l2_size_kb * 1024
    pow2 = lambda n: n > 0 and n & (n - 1) == 0
    assert pow2(case.line_size) and pow2(l1_sets) and pow2(l2_sets)
    assert l2_sets >= l1_sets
    assert l1_sets <= 1024
    assert case.l1d_assoc <= 8 and case.l2_assoc <= 32
    assert (case.u1, case.s2) == (l1_sets, l2_sets // l1_sets)
    key = (case.l1d_assoc, case.l2_assoc, 1 if case.l1d_policy == LRU else 0, 1 if case.l2_policy == LRU else 0)
    assert key in inst["GG_KERN"]
    assert replay_lds_bytes(case) <= 64 * 1024
    has_instance = any(e[:4] == key and e[4] * 64 == case.u1 for e in inst["GG_STREAM"])
    rule = has_instance and stream_lds_bytes(case) <= 160 * 1024 and case.s2 * case.l2_assoc < 255
    assert case.stream == rule
    want_inv = (case.l1d_policy == LRU and case.l1d_assoc >= 2) or case.l2_policy == RR
    assert case.inv_l1 == want_inv
    cfg = G.config(case)
    assert (cfg.num_tiles, cfg.line_size, cfg.l1d_assoc, cfg.l2_policy) == (case.tiles, case.line_size,
                                                                            case.l1d_assoc, case.l2_policy)


def test_lds_fallback_row_is_the_one_the_bound_excludes():
    c = next(c for c in G.CASES if c.name == "u256_s16")
    assert c.s2 * c.u1 * 40 == 160 * 1024 and stream_lds_bytes(c) > 160 * 1024
    assert stream_lds_bytes(next(c for c in G.CASES if c.name == "u256_s8")) <= 160 * 1024


@functools.lru_cache(maxsize=None)
def oracle_run(name):
    case = next(c for c in G.CASES if c.name == name)
    addr, meta, offs = G.build_trace(case, 1)
    res = po.OracleCache(G.config(case)).run(addr, meta, offs)
    return case, addr, meta, offs, res


@pytest.mark.parametrize("case", G.CASES, ids=lambda c: c.name)
def test_trace_shape_and_oracle_result_bits(case):
    """A condition on the inputs: the oracle's result on the row's trace holds
    every RES_* bit (RES_L2_EVICT_INV_L1 exactly where inv_l1 says), so a GPU
    run that equals the oracle has taken every branch of the access step."""
    _, addr, meta, offs, res = oracle_run(case.name)
    lens = np.diff(offs.astype(np.int64))
    assert len(offs) == case.tiles + 1 and int(offs[-1]) == len(addr) == len(meta)
    assert int((lens == 0).sum()) == 1
    assert len(set(lens.tolist())) == case.tiles                    # ragged
    l2_lines = G.geometry(case)[1] * case.l2_assoc
    assert np.all((lens == 0) | ((lens >= 3 * l2_lines) & (lens <= 6 * l2_lines + 2 * case.l2_assoc + 3)))
    tile = np.repeat(np.arange(case.tiles), lens)
    assert np.array_equal(addr >> np.uint64(G.TILE_SHIFT), tile.astype(np.uint64))
    sub = addr & np.uint64(case.line_size - 1)
    assert len(np.unique(sub)) >= min(case.line_size, 32)           # the sub-line offset varies
    # below the compressed-tag range of every geometry (gg_geom::addr_limit)
    assert int(addr.max()) < 0xFFFFFFFF << 10
    for name in RES_BITS:
        n = int(((res & np.uint32(getattr(C, name))) != 0).sum())
        print("%s %s %d" % (case.name, name, n))
        if name == "RES_L2_EVICT_INV_L1" and not case.inv_l1:
            assert n == 0
        else:
            assert n > 0, name


def test_fresh_addresses_are_fresh():
    for case in G.CASES:
        _, addr, _, _, _ = oracle_run(case.name)
        seen = set((addr >> np.uint64(case.line_size.bit_length() - 1)).tolist())
        fresh = G.fresh_addresses(case, 64, 5)
        assert len(fresh) == 64
        assert not any((a >> (case.line_size.bit_length() - 1)) in seen for _, a in fresh)
        assert all(a >> G.TILE_SHIFT == t < case.tiles for t, a in fresh)


@pytest.mark.parametrize("pol1,pol2", [(LRU, RR), (RR, LRU), (RR, RR)])
def test_oracle_round_robin_victim_order(pol1, pol2):
    """The oracle's round-robin victims by hand (RoundRobinReplacementPolicy:
    the index starts at assoc - 1, getReplacementWay returns it and steps it
    down, wrapping to assoc - 1; update() is a no-op), a1 = 4, both levels,
    through the quartet: four fills of one set go to ways 3, 2, 1, 0, so the
    fifth evicts the FIRST line filled, then the second ... whatever was
    accessed in between; LRU evicts the least recently used."""
    cfg = C.default_config(1, l1d_size_kb=4, l1d_assoc=4, l1d_policy=pol1, l2_size_kb=16, l2_assoc=4, l2_policy=pol2)
    oc = po.OracleCache(cfg)
    for level, pol, sets in ((C.L1D, pol1, 16), (C.L2, pol2, 64)):
        line = lambda k: (k * sets + 5) * 64                # lines of set 5
        for k in range(4):
            rc, ev, _, _ = oc.insert_line(0, level, line(k), po.LineInfo(line(k) >> 6, C.CSTATE_SHARED, 0))
            assert (rc, ev) == (0, 0)
        assert oc.access_line(0, level, line(0), False) == 0        # line 0 is now the most recently used
        victims = []
        for k in range(4, 8):
            rc, ev, ea, evi = oc.insert_line(0, level, line(k), po.LineInfo(line(k) >> 6, C.CSTATE_MODIFIED, 0))
            assert (rc, ev) == (0, 1) and evi.tag == ea >> 6 and evi.cstate == C.CSTATE_SHARED
            victims.append(ea)
        if pol == RR:
            assert victims == [line(0), line(1), line(2), line(3)]
        else:
            assert victims == [line(1), line(2), line(3), line(0)]


def test_oracle_round_robin_mixed_replay_by_hand():
    """The mixed-policy rows through the replay: L1-D round-robin over an LRU
    L2 and the reverse, one set, five lines.  Reads of A, B, C, D fill the
    four L1-D ways (round-robin: ways 3, 2, 1, 0); A is read again (an L1-D
    hit: no L2 touch); E conflicts.  Round-robin L1-D: the index is back at
    way 3, so E evicts A (the first filled); LRU L1-D: E evicts B, the least
    recently used.  The L2 (8 lines per set here) evicts nothing."""
    for pol1, first_out in ((RR, 0), (LRU, 1)):
        cfg = C.default_config(1, l1d_size_kb=4, l1d_assoc=4, l1d_policy=pol1, l2_size_kb=8, l2_assoc=8,
                               l2_policy=RR if pol1 == LRU else LRU)
        oc = po.OracleCache(cfg)
        line = lambda k: (k * 16 + 3) * 64                          # 16 sets at both levels: one L2 set per L1-D set
        seq = [0, 1, 2, 3, 0, 4]
        addr = np.array([line(k) for k in seq], np.uint64)
        res = oc.run(addr, np.zeros(len(seq), np.uint32), np.array([0, len(seq)], np.uint64))
        miss = C.RES_L1_MISS | C.RES_L2_MISS
        assert res.tolist() == [miss] * 4 + [0, miss | C.RES_L1_EVICT]
        held = [oc.get_line_info(0, C.L1D, line(k)).tag != 0xFFFFFFFFFFFFFFFF for k in range(5)]
        assert held == [k != first_out for k in range(5)]
        loc = [oc.get_line_info(0, C.L2, line(k)).cached_loc for k in range(5)]
        assert loc == [C.LOC_L1D if k != first_out else C.LOC_INVALID for k in range(5)]
