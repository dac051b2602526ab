#!/usr/bin/env python3
"""Print an all-pairs case table for tests/sweep_cases.py.

A deterministic greedy covering array over sweep_cases.FACTORS: every pair of
levels of two different factors that sweep_cases.CONSTRAINTS allows gets into
at least one row.  Each row is the best of CANDIDATES candidates; a candidate
starts from an uncovered pair and takes, factor by factor in a shuffled order
(random.Random(SEED)), the level that covers the most uncovered pairs with the
levels it has.  Rows that are in the committed table already keep their
records per tile; new rows get a default by mesh, to be tuned by hand against
the conditions of tests/test_sweep_cases.py.

Beside CONSTRAINTS (what the product refuses) the generator steers by steer():
combinations of three and more levels that are valid runs but could not meet
a condition the tests assert within the trace lengths allowed (a window needs
2 + quantum / L1-D data time records, gg_coh_window.hip:71-72; a run in legs
needs six quanta; a tile's miss-type table holds miss_track_lines addresses).
steer() excludes no pair.

    python tools/sweep_pairs.py            # prints the rows of CASES_TEXT
"""
import itertools
import math
import os
import random
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tests import sweep_cases as S  # noqa: E402

SEED, CANDIDATES = 1, 60
DEFAULT_N = {"2x3k2": 600, "3x4k3": 500, "4x4k4": 400, "4x5k5": 300, "8x9k8": 100, "4x4k1": 400}


def _kw(label, key, default):
    return S.LEVEL[label][1].get(key, default)


MISS_TABLE_RECORDS = 1000                 # miss_track_lines = 1024 addresses a tile: nearly every record a new line


def window_records(clock, cycles, quantum, mesh):
    """The records a tile of a windowed row needs for two hand-overs that are
    not its last.  A window holds 2 + (next barrier - tile clock) / L1-D data
    time records and 8 more; a tile that waits for a message from another
    shard, or through quanta shorter than a miss, is some quanta behind the
    barrier, so its window is some quanta long."""
    lat = math.ceil(_kw(cycles, "l1d_data_cycles", 1) * 1000.0 / _kw(clock, "frequency_ghz", 1.0))
    need = 2 + 8 + math.ceil(_kw(quantum, "quantum_ns", 1000) * 1000.0 / lat)
    behind = 1.5 if _kw(mesh, "num_shards", 1) == 1 and quantum != "q100" else 4
    return int(behind * need)


def record_cap(row):
    cap = S.MAX_RECORDS_72 if row["mesh"] == "8x9k8" else S.MAX_RECORDS
    if row["driver"] == "win" and row["quantum"] == "q10000":
        cap *= 2                          # (see the note above the table)
    if row["miss_types"] not in (None, "mt0"):
        cap = min(cap, MISS_TABLE_RECORDS)
    return cap


def default_n(r):
    """Accesses per tile of a new row: short, a windowed row long enough for
    two hand-overs that are not its last, all within the caps."""
    row = dict(zip(S.NAMES, r))
    kind, driver = row["trace"], row["driver"]
    cap = record_cap(row)
    recs = min(cap, DEFAULT_N[row["mesh"]])
    if driver == "win":
        recs = min(cap, max(recs, window_records(row["clock"], row["cycles"], row["quantum"], row["mesh"])))
    if driver == "ens":                   # the longest instance has 3 n / 2
        recs = min(recs, cap * 2 // 3)
    if kind == "multi":                   # about 2.4 lines an access, up to 2.8 over a short tile
        return recs * 5 // 14
    if kind == "barr":
        return recs * S.BARRIER_EVERY // (S.BARRIER_EVERY + 1)
    return recs


def steer(row):
    """row: factor -> label or None.  False when no completion of the None
    entries can meet the tests' conditions."""
    d = row["driver"]
    if d == "win":
        fs = ("clock", "cycles", "quantum", "mesh", "miss_types")
        opts = [[row[f]] if row[f] else [l for l, _ in S.FACTORS[f]] for f in fs]
        if not any(window_records(*c[:4]) <= record_cap(dict(zip(fs, c), driver=d)) for c in itertools.product(*opts)):
            return False
    if d in ("legs", "win") and row["quantum"] == "q10000" and row["mesh"] == "8x9k8":
        return False                      # 150 records a tile end in fewer than six quanta of 10 000 ns
    return True


def ok(row):
    labs = [l for l in row.values() if l]
    return all(S.allowed(a, b) for a, b in itertools.combinations(labs, 2)) and steer(row)


def candidate(rng, seed_pair, uncovered):
    row = dict.fromkeys(S.NAMES)
    for lab in seed_pair:
        row[S.LEVEL[lab][0]] = lab
    if not ok(row):
        return None
    rest = [f for f in S.NAMES if row[f] is None]
    rng.shuffle(rest)
    for f in rest:
        best, best_gain = None, -1
        for lab, _ in S.FACTORS[f]:
            row[f] = lab
            if ok(row):
                gain = sum(1 for o in row.values() if o and o != lab and
                           ((o, lab) in uncovered or (lab, o) in uncovered))
                if gain > best_gain:
                    best, best_gain = lab, gain
        row[f] = best
        if best is None:
            return None
    return tuple(row[f] for f in S.NAMES)


def generate():
    rng = random.Random(SEED)
    uncovered = set(S.all_pairs())
    rows = []
    while uncovered:
        seeds = sorted(uncovered)
        best, best_gain = None, 0
        for i in range(CANDIDATES):
            c = candidate(rng, seeds[(i * 7919) % len(seeds)], uncovered)
            if c:
                gain = len(S.pairs_of(c) & uncovered)
                if gain > best_gain:
                    best, best_gain = c, gain
        if best is None:
            raise SystemExit("no row covers any of %d pairs, e.g. %s" % (len(uncovered), seeds[:5]))
        rows.append(best)
        uncovered -= S.pairs_of(best)
    return rows


def main():
    known = {c.labels: c.n for c in S.CASES}
    width = [max(len(l) for l, _ in S.FACTORS[f]) for f in S.NAMES]
    for r in generate():
        n = known.get(r, default_n(r))
        print("%5d  %s" % (n, " ".join(l.ljust(w) for l, w in zip(r, width)).rstrip()))


if __name__ == "__main__":
    main()
