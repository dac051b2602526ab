"""Private-cache replay geometries: the literal case table and build_trace(case).

One row per geometry the replay must get right: every (L1-D assoc, L2 assoc,
policies) instantiation of gg_cache.hip's kKernels / kLean / kStream tables,
every L1-D set count per tile (u1) from 1 to 1024, the largest L2-sets-per-
L1-D-set ratios (s2) the LDS bound admits, and line sizes off 64.
tests/test_cache_geometry_cases.py checks the table against the instantiation
lists and the oracle; tests/test_gpu_cache_geometry.py runs each row on the GPU
under every replay_kernel.  Plain Python, importable without a GPU.

u1 = l1d_size_kb * 1024 / (l1d_assoc * line_size); L2 sets likewise;
s2 = L2 sets / u1.  Both are written out per row (the CPU test recomputes them).

`stream` is derived BY HAND from the dispatch rule of gg_cache_run_batch, not
computed: under replay_kernel = 0 k_cache_stream runs iff kStream holds
(a1, a2, policies) with ncw * 64 == u1, stream_lds_bytes <= 160 KiB and
s2 * a2 < 255 (the per-tile length bound never binds here).  Everything else,
and every row under replay_kernel 1 / 2, takes the sharded pipeline
(k_cache_replay, or k_cache_replay_lean where kLean holds the geometry and
replay_kernel != 1).

`inv_l1`: whether the trace reaches RES_L2_EVICT_INV_L1 (an L2 eviction of a
line the L1-D holds).  True wherever the L1-D is LRU with a1 >= 2, or the L2 is
round-robin; a round-robin (FIFO) L1-D or a one-way L1-D under an LRU L2 never
holds the L2's least recently used line.
"""
import collections

import numpy as np

from graphite_amd import config as C
from oracle import pyoracle as po

LRU, RR = C.POLICY_LRU, C.POLICY_ROUND_ROBIN

Case = collections.namedtuple(
    "Case", "name tiles l1d_size_kb l1d_assoc l1d_policy l2_size_kb l2_assoc l2_policy line_size u1 s2 stream inv_l1")

# Tile counts: 5 where u1 < 64 (tiles * u1 off a multiple of 64: the last
# replay wave is partly idle), fewer tiles for the two largest L2s.
CASES = [
    # ---- one row per kKernels entry; those also in kStream at u1 = 128 (ncw 2) ----
    #    name          T  L1kb a1 pol1  L2kb a2 pol2 line   u1  s2  stream inv_l1
    Case("k4_8_ll",     6,  32, 4, LRU,  128,  8, LRU,  64,  128,  2, True,  True),
    Case("k4_8_rr",     6,  32, 4, RR,   128,  8, RR,   64,  128,  2, True,  True),
    Case("k4_8_lr",     6,  32, 4, LRU,  128,  8, RR,   64,  128,  2, True,  True),
    Case("k4_8_rl",     6,  32, 4, RR,   128,  8, LRU,  64,  128,  2, True,  False),
    Case("k4_16_ll",    6,  32, 4, LRU,  256, 16, LRU,  64,  128,  2, True,  True),
    Case("k4_16_rr",    6,  32, 4, RR,   256, 16, RR,   64,  128,  2, True,  True),
    Case("k4_16_lr",    6,  32, 4, LRU,  256, 16, RR,   64,  128,  2, False, True),    # no stream instance
    Case("k4_16_rl",    6,  32, 4, RR,   256, 16, LRU,  64,  128,  2, False, False),   # no stream instance
    Case("k4_4_ll",     6,  32, 4, LRU,   64,  4, LRU,  64,  128,  2, True,  True),
    Case("k2_4_ll",     6,  16, 2, LRU,   64,  4, LRU,  64,  128,  2, True,  True),
    Case("k2_8_ll",     6,  16, 2, LRU,  128,  8, LRU,  64,  128,  2, True,  True),
    Case("k2_16_ll",    5,   4, 2, LRU,   64, 16, LRU,  64,   32,  2, False, True),
    Case("k8_8_ll",     5,  16, 8, LRU,   64,  8, LRU,  64,   32,  4, False, True),
    Case("k8_16_ll",    5,  16, 8, LRU,  128, 16, LRU,  64,   32,  4, False, True),
    Case("k8_4_ll",     5,   8, 8, LRU,   16,  4, LRU,  64,   16,  4, False, True),
    Case("k1_8_ll",     6,   4, 1, LRU,   64,  8, LRU,  64,   64,  2, False, False),   # A1 = 1
    Case("k4_2_ll",     6,  32, 4, LRU,   64,  2, LRU,  64,  128,  4, True,  True),    # s2 * a2 > a1, or the L1-D never evicts
    Case("k4_32_ll",    5,   8, 4, LRU,  256, 32, LRU,  64,   32,  4, False, True),    # mw = 4; s2 = 4 is a2 = 32's largest
    # ---- u1 on the (4, 8, LRU, LRU) instance ----
    Case("u64",         6,  16, 4, LRU,   64,  8, LRU,  64,   64,  2, True,  True),    # stream, ncw 1
    Case("u256_s8",     4,  64, 4, LRU, 1024,  8, LRU,  64,  256,  8, True,  True),    # stream, ncw 4 (150 KiB of LDS)
    Case("u256_s16",    3,  64, 4, LRU, 2048,  8, LRU,  64,  256, 16, False, True),    # instance exists, LDS > 160 KiB
    Case("u512",        6, 128, 4, LRU,  256,  8, LRU,  64,  512,  1, False, True),
    Case("u1024_s1",    6, 256, 4, LRU,  512,  8, LRU,  64, 1024,  1, False, True),
    Case("u1",          5,   1, 4, LRU,    8,  8, LRU, 256,    1,  4, False, True),
    Case("u2",          5,   2, 4, LRU,   16,  8, LRU, 256,    2,  4, False, True),
    # ---- s2 at its ends (s2 = 4 on a2 = 32 is k4_32_ll) ----
    Case("s1_a8",       6,  32, 4, LRU,   64,  8, LRU,  64,  128,  1, True,  True),
    Case("s16_a8",      6,  16, 4, LRU,  512,  8, LRU,  64,   64, 16, True,  True),    # stream, ncw 1, s2 * a2 = 128
    Case("s32_a4",      5,   8, 4, LRU,  256,  4, LRU,  64,   32, 32, False, True),
    # ---- line sizes off 64: a streaming and a sharded-only geometry each ----
    Case("line32_st",   6,  16, 4, LRU,   64,  8, LRU,  32,  128,  2, True,  True),
    Case("line128_st",  6,  64, 4, LRU,  256,  8, LRU, 128,  128,  2, True,  True),
    Case("line32_sh",   5,   8, 8, LRU,   32,  8, LRU,  32,   32,  4, False, True),
    Case("line128_sh",  5,   8, 2, LRU,  128, 16, LRU, 128,   32,  2, False, True),
]

TILE_SHIFT = 32          # tile id in the address bits above every line of the trace
PIN_TAG = 64             # L2 tags of the pinned-line phase: above the uniform footprint's (< 2 * a2 <= 64)
FRESH_TAG = 200          # L2 tags no trace touches (fresh_addresses)


def overrides(case):
    return dict(l1d_size_kb=case.l1d_size_kb, l1d_assoc=case.l1d_assoc, l1d_policy=case.l1d_policy,
                l2_size_kb=case.l2_size_kb, l2_assoc=case.l2_assoc, l2_policy=case.l2_policy,
                line_size=case.line_size)


def config(case, **kw):
    return C.default_config(case.tiles, **overrides(case), **kw)


def geometry(case):
    """(L1-D sets, L2 sets) as gg_create computes them (integer division)."""
    return (case.l1d_size_kb * 1024 // (case.l1d_assoc * case.line_size),
            case.l2_size_kb * 1024 // (case.l2_assoc * case.line_size))


def build_trace(case, seed):
    """(addr, meta, offs) for the row, tile-major.

    Uniform part, per tile: gen_uniform over 2x the L2's lines, 3x..6x the L2's
    line count in records (ragged; one tile empty), re-addressed to the row's
    line size with a sub-line byte offset per record and the tile id at
    TILE_SHIFT.  Pinned-line phase, appended to every non-empty tile, in one L2
    set: read H, then for each of a2 + 1 fresh conflicting lines access it
    (every other one a WRITE) and read H again.  The reads of H hit the L1-D,
    so they never touch the L2's replacement state: H ages to the L2's victim
    while the L1-D holds it (RES_L2_EVICT_INV_L1)."""
    rng = np.random.default_rng(seed)
    _, l2_sets = geometry(case)
    l2_lines = l2_sets * case.l2_assoc
    lines_log2 = (2 * l2_lines).bit_length() - 1
    empty = int(rng.integers(0, case.tiles))
    addrs, metas, lens = [], [], []
    for t in range(case.tiles):
        if t == empty:
            lens.append(0)
            continue
        n = int(rng.integers(3 * l2_lines, 6 * l2_lines + 1))
        a, m = po.gen_uniform(t, int(rng.integers(0, 1000)), n, lines_log2=lines_log2)
        line = (a >> np.uint64(6)) & np.uint64((1 << lines_log2) - 1)
        s = (7 * t + 3) % l2_sets
        pin = [(PIN_TAG * l2_sets + s, 0)]
        for i in range(case.l2_assoc + 1):
            pin += [((PIN_TAG + 1 + i) * l2_sets + s, i & 1), (PIN_TAG * l2_sets + s, 0)]
        line = np.concatenate([line, np.array([p[0] for p in pin], np.uint64)])
        m = np.concatenate([m, np.array([C.META_WRITE if p[1] else 0 for p in pin], np.uint32)])
        sub = rng.integers(0, case.line_size, len(line)).astype(np.uint64)
        addrs.append((np.uint64(t) << np.uint64(TILE_SHIFT)) | (line * np.uint64(case.line_size) + sub))
        metas.append(m)
        lens.append(len(line))
    offs = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)
    return np.concatenate(addrs), np.concatenate(metas), offs


def fresh_addresses(case, count, seed):
    """(tile, addr) pairs no build_trace of the row touches."""
    rng = np.random.default_rng(seed)
    _, l2_sets = geometry(case)
    out = []
    for k in range(count):
        t = int(rng.integers(0, case.tiles))
        line = (FRESH_TAG + k) * l2_sets + int(rng.integers(0, l2_sets))
        out.append((t, (t << TILE_SHIFT) | (line * case.line_size + int(rng.integers(0, case.line_size)))))
    return out
