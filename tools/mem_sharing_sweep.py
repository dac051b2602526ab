#!/usr/bin/env python3
"""Degree-of-sharing sweep of the synthetic memory benchmark:
one input file of the reference's synthetic_memory.cc and one caching protocol,
degree of sharing 1, 2, 4, ..., T (its -ns option).  Every point generates its
own trace (gg_gen_memory_traffic) for a context of its own; all points then run
in one gg_coherent_run_many call (the contexts share one configuration, so they
are launch-compatible; if the call rejects the set, or with --loop, they run
one by one through gg_coherent_run) and each is reduced on the device
(gg_mem_latency_stats).

Prints a table: max tile clock, L2 miss ratio and mean latency by level per
degree; with --json one JSON line per point instead.  Then one line with the
wall time of the run step ("run_ms": the median over --reps passes after an
untimed one, a host clock between two device synchronisations); with
--compare-loop also "loop_ms", the same contexts, reset, one by one in the
same process.  Results are not verified here (tests/test_gpu_memgen.py does
that).

--time-generator: instead of the sweep, the input as it is: plan, fill, the
coherent run they feed and the reduction, each timed on its own in the same
process, warm, the median of --reps passes; one JSON line with the ratios.
"""
import argparse
import ctypes
import json
import math
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

PROTOCOLS = ["msi", "mosi", "shl2_msi", "shl2_mesi"]
NETS = ["magic", "hop_counter", "hop_by_hop"]


def main():
    from graphite_amd import config as C
    from graphite_amd import backend as B
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("input", help="a synthetic_memory input file (tests/golden/synthetic_memory/input.64)")
    ap.add_argument("--protocol", default="msi", choices=PROTOCOLS)
    ap.add_argument("--net", default="hop_by_hop", choices=NETS)
    ap.add_argument("--tiles", type=int, default=0, help="0: the file's thread count")
    ap.add_argument("--instructions", type=int, default=0, help="0: the file's instructions per tile")
    ap.add_argument("--degrees", default="", help="comma-separated; default 1, 2, 4, ..., tiles")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--loop", action="store_true", help="run the points one by one")
    ap.add_argument("--compare-loop", action="store_true", help="also time the one-by-one loop")
    ap.add_argument("--json", action="store_true")
    ap.add_argument("--time-generator", action="store_true")
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("mem_sharing_sweep: no GPU (there is no CPU path)")

    base = C.MemTrafficParams.from_input_file(args.input)
    T = args.tiles or base.num_threads
    base = base.replace(num_threads=T, instructions_per_tile=args.instructions or base.instructions_per_tile)
    cfg = C.default_config(T, protocol=PROTOCOLS.index(args.protocol), net_model=NETS.index(args.net))
    cycle_ps = math.ceil(1000.0 / cfg.frequency_ghz)

    def clock(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r = fn()
        torch.cuda.synchronize()
        return r, time.perf_counter() - t0

    if args.time_generator:
        L = B.load()
        offs, total = np.zeros(T + 1, np.uint64), ctypes.c_uint64(0)
        po = offs.ctypes.data_as(ctypes.c_void_p)

        def plan():
            B._check(L.gg_gen_memory_traffic(ctypes.byref(base), T, cfg.line_size, po, ctypes.byref(total), None, None, 0,
                                             None, None, B._stream(None)))
        plan()
        n = int(total.value)
        addr = torch.zeros(n, dtype=torch.int64, device="cuda")
        meta = torch.zeros(n, dtype=torch.int32, device="cuda")
        out = torch.zeros(n, dtype=torch.int64, device="cuda")

        def both():                                       # the fill call repeats the plan
            B._check(L.gg_gen_memory_traffic(ctypes.byref(base), T, cfg.line_size, None, None, B._ptr(addr), B._ptr(meta),
                                             n, None, None, B._stream(None)))
        be = B.Backend(cfg)
        times = {"plan": [], "plan_and_fill": [], "run": [], "reduce": []}
        for k in range(args.reps + 1):
            be.reset()
            t = {"plan": clock(plan)[1], "plan_and_fill": clock(both)[1],
                 "run": clock(lambda: be.coherent_run(addr, meta, offs, out))[1],
                 "reduce": clock(lambda: B.mem_latency_stats(meta, out))[1]}
            if k:
                for name in times:
                    times[name].append(t[name])
        be.close()
        med = {name: float(np.median(v)) * 1e3 for name, v in times.items()}
        fill = med["plan_and_fill"] - med["plan"]
        print(json.dumps({"input": os.path.basename(args.input), "tiles": T, "protocol": args.protocol, "net": args.net,
                          "instructions_per_tile": int(base.instructions_per_tile), "records": n, "reps": args.reps,
                          "plan_ms": med["plan"], "fill_ms": fill, "run_ms": med["run"], "reduce_ms": med["reduce"],
                          "plan_over_run": med["plan"] / med["run"], "fill_over_run": fill / med["run"],
                          "reduce_over_run": med["reduce"] / med["run"],
                          "all_ms": {name: [x * 1e3 for x in v] for name, v in times.items()}}), flush=True)
        return

    degrees = [int(x) for x in args.degrees.split(",")] if args.degrees else \
        [1 << k for k in range(T.bit_length()) if 1 << k <= T]
    traces = [B.gen_memory_traffic(base.replace(degree_of_sharing=d), T, cfg.line_size) for d in degrees]
    bes = [B.Backend(cfg) for _ in degrees]                  # a context per point
    outs = [torch.zeros(t[0].numel(), dtype=torch.int64, device="cuda") for t in traces]

    def run_many():
        B.coherent_run_many(bes, [t[0] for t in traces], [t[1] for t in traces], [t[2] for t in traces], outs)

    def run_loop():
        for be, t, o in zip(bes, traces, outs):
            be.coherent_run(t[0], t[1], t[2], o)

    def points():
        res = []
        for be, t, o in zip(bes, traces, outs):
            s = B.mem_latency_stats(t[1], o)
            clock_ps = be.coherent_stats()[0][:, 0] + t[3].cpu().numpy().view(np.uint64) * np.uint64(cycle_ps)
            res.append((s, int(clock_ps.max())))
        return res

    many = not args.loop
    if many:
        try:
            run_many()
        except B.GGError as e:
            if e.statuses is not None and any(e.statuses):
                raise                                     # an instance failed: the loop would fail too
            print("mem_sharing_sweep: gg_coherent_run_many rejects the set (%s); running one by one" % e, file=sys.stderr)
            many = False
    timed = {"run_ms": [], "loop_ms": []}
    result = None
    for name, fn in (("run_ms", run_many if many else run_loop), ("loop_ms", run_loop if args.compare_loop and many else None)):
        for k in range((args.reps + 1) if fn else 0):
            for be in bes:
                be.reset()
            timed[name].append(clock(fn)[1])
            got = points()
            if result is None:
                result = got
            elif any(not np.array_equal(a[0], b[0]) or a[1] != b[1] for a, b in zip(got, result)):
                sys.exit("mem_sharing_sweep: two passes disagree")
    for be in bes:
        be.close()

    mean = lambda s, n: float(s) / float(n) if n else 0.0
    if not args.json:
        print("%s, %d tiles, %s, %s" % (os.path.basename(args.input), T, args.protocol, args.net))
        print("%7s %9s %16s %9s %10s %10s %12s" % ("degree", "records", "max clock (ns)", "L2 miss", "L1 (ps)", "L2 (ps)",
                                                   "miss (ps)"))
    for d, (s, clk) in zip(degrees, result):
        row = {"degree": d, "records": int(s[C.MLS_RECORDS]), "max_tile_clock_ns": math.ceil(clk / 1000.0),
               "l2_miss_ratio": mean(s[C.MLS_L2_MISSES], s[C.MLS_RECORDS]),
               "mean_l1_ps": mean(s[C.MLS_L1_LATENCY_PS], s[C.MLS_L1_HITS]),
               "mean_l2_ps": mean(s[C.MLS_L2_LATENCY_PS], s[C.MLS_L2_HITS]),
               "mean_l2_miss_ps": mean(s[C.MLS_L2_MISS_LATENCY_PS], s[C.MLS_L2_MISSES])}
        if args.json:
            row.update({"input": os.path.basename(args.input), "tiles": T, "protocol": args.protocol, "net": args.net,
                        "stats": {f: int(s[i]) for i, f in enumerate(C.MLS_FIELDS)}})
            print(json.dumps(row), flush=True)
        else:
            print("%7d %9d %16d %9.4f %10.1f %10.1f %12.1f" % (d, row["records"], row["max_tile_clock_ns"],
                                                              row["l2_miss_ratio"], row["mean_l1_ps"], row["mean_l2_ps"],
                                                              row["mean_l2_miss_ps"]))
    line = {"input": os.path.basename(args.input), "tiles": T, "protocol": args.protocol, "net": args.net,
            "points": len(degrees), "many": many, "reps": args.reps,
            "run_ms": float(np.median(timed["run_ms"][1:])) * 1e3, "run_ms_all": [x * 1e3 for x in timed["run_ms"][1:]]}
    if timed["loop_ms"]:
        line.update({"loop_ms": float(np.median(timed["loop_ms"][1:])) * 1e3,
                     "loop_ms_all": [x * 1e3 for x in timed["loop_ms"][1:]]})
    print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
