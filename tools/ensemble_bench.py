#!/usr/bin/env python3
"""Ensemble timing: coherent_run_many over n contexts against n back-to-back
coherent_run calls on the same contexts, in one process.

usage: ensemble_bench.py T RECORDS_PER_TILE N [--hbh] [--shards K] [--repeats R]
                         [--stats-trace INTERVAL_NS [--statistics BITS]] [--legs N]

Builds n contexts of T tiles (hop counter, or --hbh: emesh_hop_by_hop over K
logical shards, default 8) with distinct hotspot traces (hot_lines and
hot_frac256 vary with the instance), runs each leg once to warm up and R = 5
times timed (host wall clock around the calls, device synchronised), and
prints one JSON line: the median and the spread (max - min) of each leg in
ms, their ratio, and whether both legs left identical access words.  The
sequential leg is the yardstick: it is gg_coherent_run as it stands (the
persistent kernel up to 64 tiles, per-step launches above).

--stats-trace INTERVAL_NS configures a statistics trace on every context
(--statistics: GG_ST_* bits, default 3 = network_utilization and
cache_line_replication), so the sequential leg is the traced gg_coherent_run
and the ensemble leg is coherent_begin per context, then
coherent_advance_many (coherent_run_many refuses a traced context).  --legs N
cuts the ensemble leg into N calls of coherent_advance_many, the stops at
k / N of each instance's own final quantum (--legs 1: the same driver, one
call).  With either option the JSON line also carries the option values, the
samples taken, the slots the longest instance needs (its steps + quanta: the
ensemble spends a launch per step and one per quantum end) and whether the
samples of both legs are identical; without them the output is unchanged."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("tiles", type=int)
    ap.add_argument("records", type=int)
    ap.add_argument("n", type=int)
    ap.add_argument("--hbh", action="store_true")
    ap.add_argument("--shards", type=int, default=None)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--stats-trace", type=int, default=0, metavar="INTERVAL_NS")
    ap.add_argument("--statistics", type=int, default=3)
    ap.add_argument("--legs", type=int, default=0)
    a = ap.parse_args()
    import torch
    from graphite_amd import backend as B
    from graphite_amd import config as C
    T, N, n = a.tiles, a.records, a.n
    net = C.NET_EMESH_HOP_BY_HOP if a.hbh else C.NET_EMESH_HOP_COUNTER
    K = a.shards if a.shards is not None else (8 if a.hbh else 1)
    offs = np.arange(T + 1, dtype=np.uint64) * np.uint64(N)
    bes, addrs, metas, outs = [], [], [], []
    for i in range(n):
        bes.append(B.Backend(C.default_config(T, num_shards=K, net_model=net)))
        addr = torch.empty(T * N, dtype=torch.int64, device="cuda")
        meta = torch.empty(T * N, dtype=torch.int32, device="cuda")
        B.gen_hotspot_trace(addr, meta, 0, T, N, hot_lines=16 + 8 * (i % 8), hot_frac256=40 + 5 * (i % 16))
        addrs.append(addr); metas.append(meta)
        outs.append(torch.zeros(T * N, dtype=torch.int64, device="cuda"))
    offsets = [offs] * n

    def sequential():
        for be, ad, me, out in zip(bes, addrs, metas, outs):
            be.coherent_run(ad, me, offs, out)

    def ensemble():
        B.coherent_run_many(bes, addrs, metas, offsets, outs)

    advance = a.stats_trace > 0 or a.legs > 0              # the ensemble leg through begin + advance_many
    legs = max(a.legs, 1)
    final = []
    if advance:
        # an untraced run of each first: the final quanta (the stops, the sample buffers' sizes)
        sequential()
        ri = [be.coherent_stats()[2] for be in bes]
        final = [int(r[C.RUN_INFO.index("final_quantum")]) for r in ri]
        slots = max(int(r[C.RUN_INFO.index("steps")]) + int(r[C.RUN_INFO.index("quanta")]) for r in ri)
        if a.stats_trace:
            for be, F in zip(bes, final):
                be.stats_trace_configure(a.statistics, a.stats_trace,
                                         (F + 1) * be.cfg.quantum_ns // a.stats_trace + 8)

    def ensemble_legs():
        for be, ad, me, out in zip(bes, addrs, metas, outs):
            be.coherent_begin(ad, me, offs, out)
        for k in range(1, legs + 1):
            r = B.coherent_advance_many(bes, None if k == legs else [k * F // legs for F in final])
        assert all(d == 1 for _, d in r), r

    def samples():
        return [be.stats_trace() for be in bes] if a.stats_trace else []

    def timed(fn):
        ms = []
        for r in range(a.repeats + 1):                     # the first run warms up
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            if r:
                ms.append((time.perf_counter() - t0) * 1e3)
        return ms

    seq = timed(sequential)
    words = [o.clone() for o in outs]
    steps = [int(be.coherent_stats()[2][C.RUN_INFO.index("steps")]) for be in bes]
    seq_samples = samples()
    ens = timed(ensemble_legs if advance else ensemble)
    same = all(bool(torch.equal(w, o)) for w, o in zip(words, outs))
    med = statistics.median
    extra = {}
    if advance:
        ens_samples = samples()
        extra = {"stats_trace_ns": a.stats_trace, "statistics": a.statistics if a.stats_trace else 0, "legs": legs,
                 "slots_longest_instance": slots,
                 "samples": sum(len(t["time_ns"]) for t in ens_samples),
                 "identical_samples": all(sorted(x) == sorted(y) and all(np.array_equal(x[k], y[k]) for k in x)
                                          for x, y in zip(seq_samples, ens_samples))}
    print(json.dumps({
        "tool": "ensemble_bench", "tiles": T, "records_per_tile": N, "n": n,
        "net": "emesh_hop_by_hop" if a.hbh else "emesh_hop_counter", "shards": K, "repeats": a.repeats,
        "steps_min": min(steps), "steps_max": max(steps),
        "sequential_ms_median": round(med(seq), 3), "sequential_ms_spread": round(max(seq) - min(seq), 3),
        "ensemble_ms_median": round(med(ens), 3), "ensemble_ms_spread": round(max(ens) - min(ens), 3),
        "sequential_over_ensemble": round(med(seq) / med(ens), 3),
        "sequential_ms": [round(x, 3) for x in seq], "ensemble_ms": [round(x, 3) for x in ens],
        "identical_access_words": same, **extra}), flush=True)
    for be in bes:
        be.close()
    return 0 if same and extra.get("identical_samples", True) else 1


if __name__ == "__main__":
    sys.exit(main())
