#!/usr/bin/env python3
"""ATAC batch rate (gg_noc_route_batch / gg_noc_route_tree on a NET_ATAC
context): bench.py's noc.hop_by_hop packets — 262 144 uniform-random 584-bit
packets on 1024 tiles, injection times ~50 ps apart — on clusters of 16, once
as unicasts and once with 2 % of them broadcast, and the emesh_hop_by_hop
batch rate on the same packets in the same session as context.

Every figure is warm: one untimed batch first, then the median of three
batches, each routed from reset queues and timed with device events around
the call.  A last batch with the context's stage timers on gives the time per
stage (noc_atac_enet / _access_point / _send_hub / _receive).  Prints one JSON
line.  Results are not verified here (tests/test_gpu_atac.py does that).
"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

STAGES = ["noc_atac", "noc_atac_enet", "noc_atac_access_point", "noc_atac_send_hub", "noc_atac_receive"]


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--tiles", type=int, default=1024)
    ap.add_argument("--packets", type=int, default=262144)
    ap.add_argument("--cluster-size", type=int, default=16)
    ap.add_argument("--reps", type=int, default=3)
    args = ap.parse_args()
    import torch
    from graphite_amd import config as C
    from graphite_amd import backend as B
    dev = "cuda:0"
    T, n = args.tiles, args.packets
    rng = np.random.default_rng(7)                                # bench.py noc_section's packets
    src = rng.integers(0, T, n).astype(np.uint32)
    dst = rng.integers(0, T, n).astype(np.uint32)
    bits = np.full(n, C.shmem_modeled_bits(T, True), np.uint32)
    t = np.sort(rng.integers(0, 50 * n, n)).astype(np.uint64)
    bdst = dst.copy()
    bdst[np.random.default_rng(8).random(n) < 0.02] = C.BROADCAST
    d = lambda x: torch.from_numpy(x.view(np.int64 if x.dtype == np.uint64 else np.int32)).to(dev)

    def measure(be, dsts, stages):
        nb = int((dsts == C.BROADCAST).sum())
        ins = [d(src), d(dsts), d(bits), d(t)]
        outs = [torch.zeros(n, dtype=torch.int64, device=dev) for _ in range(3)]
        bouts = [torch.zeros(nb * T, dtype=torch.int64, device=dev) for _ in range(3)]

        def once():
            be.reset()
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            if nb:
                be.noc_route_tree(*ins, *outs, *bouts, nb)
            else:
                be.noc_route_batch(*ins, *outs)
            e1.record()
            torch.cuda.synchronize()
            return e0.elapsed_time(e1) / 1e3

        once()                                                    # warm-up: allocations, code load
        times = sorted(once() for _ in range(args.reps))
        dt = times[len(times) // 2]
        deliveries = (n - nb) + nb * T
        r = {"packets": n, "broadcasts": nb, "seconds_median": dt, "seconds_all": times,
             "packets_per_s": n / dt, "deliveries_per_s": deliveries / dt}
        if stages:
            be.set_timing(True)
            once()
            r["stage_ms"] = {k: be.kernel_time_ms(k) for k in STAGES}
            be.set_timing(False)
        return r

    res = {"tiles": T, "cluster_size": args.cluster_size, "reps": args.reps}
    be = B.Backend(C.default_config(T, net_model=C.NET_ATAC))
    be.noc_set_atac(C.AtacParams(cluster_size=args.cluster_size))
    res["atac_unicast"] = measure(be, dst, True)
    res["atac_2pct_broadcast"] = measure(be, bdst, True)
    be.close()
    hb = B.Backend(C.default_config(T, net_model=C.NET_EMESH_HOP_BY_HOP))
    res["emesh_hop_by_hop_same_packets"] = measure(hb, dst, False)
    hb.close()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
