#!/usr/bin/env python3
"""Load-latency sweep of the synthetic network benchmark: the
six traffic patterns of the reference's synthetic_network.cc x offered loads x
network models (emesh_hop_counter, emesh_hop_by_hop, atac), every point
generated (gg_gen_network_traffic), routed (gg_noc_route_batch) and reduced
(gg_noc_latency_stats) on the device.

One JSON line per point: the reduction's words, the means derived from them
and the wall time of the three steps, each timed on its own with a host clock
between two device synchronisations (the generator and the reduction
synchronise themselves).  A point gets a fresh context.  Its first pass is
untimed (code load, allocations); every timed pass starts from gg_reset, which
zeroes the NoC counters and re-initialises every router queue, ATAC's included
(gg_noc_reset, gg_noc.hip), so each pass routes the batch from the same empty
state and the reported statistics are those of one batch.  The times are the
medians over --reps passes.  Results are not verified here
(tests/test_gpu_netgen.py does that).

--many: all points of one (tile count, model) run in one
gg_noc_synthetic_run_many call per pass, each point on a context of its own.
The per-point lines carry the same statistics and means (the same points give
the same figures with and without --many) and no step times; one more line per
(tile count, model) gives the wall time of the whole sweep, "sweep_ms", the
median over --reps passes after an untimed one.  With --compare-loop that line
also has "loop_ms": the same contexts, reset, through gg_noc_synthetic_run one
by one in the same process.  ATAC points keep the one-by-one path.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

MODELS = ["hop_counter", "hop_by_hop", "atac"]


def main():
    from graphite_amd import config as C
    from graphite_amd import backend as B
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--tiles", default="64,1024", help="comma-separated tile counts")
    ap.add_argument("--patterns", default=",".join(B.TRAFFIC_PATTERNS))
    ap.add_argument("--loads", default="0.005,0.01,0.02,0.05,0.1,0.3",
                    help="packets / tile / cycle (a default packet is 9 flits of 64 bits)")
    ap.add_argument("--models", default=",".join(MODELS))
    ap.add_argument("--packets", type=int, default=256, help="packets per tile (-N)")
    ap.add_argument("--packet-bytes", type=int, default=8)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--atac-cluster-size", type=int, default=0, help="0: 4 below 256 tiles, else 16")
    ap.add_argument("--many", action="store_true", help="one gg_noc_synthetic_run_many call per (tiles, model) and pass")
    ap.add_argument("--compare-loop", action="store_true", help="with --many: also time the one-by-one loop")
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("noc_load_sweep: no GPU (there is no CPU path)")
    dev = "cuda:0"
    net = {"hop_counter": C.NET_EMESH_HOP_COUNTER, "hop_by_hop": C.NET_EMESH_HOP_BY_HOP, "atac": C.NET_ATAC}

    def clock(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r = fn()
        torch.cuda.synchronize()
        return r, time.perf_counter() - t0

    def point_line(T, model, p, f, s, extra):
        pk = max(int(s[B.NLS_PACKETS]), 1)
        one = 1000.0 / f
        d = {"tiles": T, "model": model, "pattern": B.TRAFFIC_PATTERNS[p.pattern], "offered_load": p.offered_load,
             "packets_per_tile": args.packets, "packet_bytes": args.packet_bytes, "seed": args.seed,
             "stats": {f_: int(s[i]) for i, f_ in enumerate(B.NLS_FIELDS)},
             "latency_hist": {str(b): int(c) for b, c in enumerate(s[B.NLS_HIST:]) if c},
             "mean_latency_cycles": float(s[B.NLS_LATENCY_PS]) / pk / one,
             "mean_zero_load_cycles": float(s[B.NLS_ZERO_LOAD_PS]) / pk / one,
             "mean_contention_cycles": float(s[B.NLS_CONTENTION_PS]) / pk / one,
             "max_latency_cycles": float(s[B.NLS_MAX_LATENCY_PS]) / one}
        d.update(extra)
        print(json.dumps(d), flush=True)

    def sweep_many(T, model):
        cfg = C.default_config(T, net_model=net[model])
        params = [B.TrafficParams(pattern, args.packet_bytes, float(load), args.packets, args.seed)
                  for pattern in args.patterns.split(",") for load in args.loads.split(",")]
        bes = [B.Backend(cfg) for _ in params]               # a fresh context per point
        many, loop = [], []
        for k in range(args.reps + 1):
            for be in bes:
                be.reset()
            stats, t = clock(lambda: B.noc_synthetic_run_many(bes, params))
            if k:
                many.append(t)
        for k in range((args.reps + 1) if args.compare_loop else 0):
            for be in bes:
                be.reset()
            one, t = clock(lambda: [be.noc_synthetic_run(p) for be, p in zip(bes, params)])
            if k:
                loop.append(t)
            if not all(np.array_equal(a, b) for a, b in zip(one, stats)):
                sys.exit("noc_load_sweep: the loop and the --many call disagree")
        for be in bes:
            be.close()
        for p, s in zip(params, stats):
            point_line(T, model, p, cfg.frequency_ghz, s, {"reps": args.reps, "many": True})
        line = {"tiles": T, "model": model, "points": len(params), "packets_per_tile": args.packets,
                "sweep_ms": float(np.median(many)) * 1e3, "sweep_ms_all": [x * 1e3 for x in many], "reps": args.reps}
        if loop:
            line.update({"loop_ms": float(np.median(loop)) * 1e3, "loop_ms_all": [x * 1e3 for x in loop]})
        print(json.dumps(line), flush=True)

    for T in [int(x) for x in args.tiles.split(",")]:
        n = T * args.packets
        ins = [torch.zeros(n, dtype=torch.int32, device=dev) for _ in range(3)] + \
              [torch.zeros(n, dtype=torch.int64, device=dev)]
        outs = [torch.zeros(n, dtype=torch.int64, device=dev) for _ in range(3)]
        for model in args.models.split(","):
            if args.many and model != "atac":
                sweep_many(T, model)
                continue
            for pattern in args.patterns.split(","):
                for load in [float(x) for x in args.loads.split(",")]:
                    cfg = C.default_config(T, net_model=net[model])
                    be = B.Backend(cfg)                                  # a fresh context per point
                    if model == "atac":
                        be.noc_set_atac(C.AtacParams(cluster_size=args.atac_cluster_size or (4 if T < 256 else 16)))
                    p = B.TrafficParams(pattern, args.packet_bytes, load, args.packets, args.seed)
                    passes = []
                    for k in range(args.reps + 1):
                        be.reset()
                        _, tg = clock(lambda: B.gen_network_traffic(p, T, cfg.frequency_ghz, *ins))
                        _, tr = clock(lambda: be.noc_route_batch(*ins, *outs))
                        s, ts = clock(lambda: B.noc_latency_stats(*ins, *outs))
                        if k:
                            passes.append((tg, tr, ts))
                    be.close()
                    med = [float(np.median([x[i] for x in passes])) for i in range(3)]
                    point_line(T, model, p, cfg.frequency_ghz, s,
                               {"generate_ms": med[0] * 1e3, "route_ms": med[1] * 1e3, "reduce_ms": med[2] * 1e3,
                                "reps": args.reps})


if __name__ == "__main__":
    main()
