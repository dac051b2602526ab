"""Cost of the statistics trace (gg_stats_trace_*) on the headline workload
(1024 tiles x 256 hotspot accesses, emesh_hop_by_hop, 8 shards, as bench.py):
whole runs (host clock around a run ending in a synchronise, 2 warm-up + RUNS
timed) with the trace off, with the scan launched every slot but no sample
due (interval 1e9 ns), and with samples every 10 000 ns (the reference's
default interval); then SCANS forced scans of the end-of-run state through
gg_stats_trace_sample, whose time is launch + synchronise, not kernel time:
the kernel's own time comes from a kernel trace of this script
(COST_SCAN_ONLY=1 skips the timed runs), read by tools/stats_trace_scan_times.py.

  python tools/stats_trace_cost.py                 -> one JSON line per measurement
  COST_SCAN_ONLY=1 rocprofv3 --kernel-trace -d DIR -o run --output-format csv -- python tools/stats_trace_cost.py
  python tools/stats_trace_scan_times.py DIR/.../run_kernel_trace.csv 50
"""
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from graphite_amd import backend as B      # noqa: E402
from graphite_amd import config as C       # noqa: E402

T, N, H, K = 1024, 256, 256, 8
RUNS = int(os.environ.get("COST_RUNS", "5"))
SCANS = int(os.environ.get("COST_SCANS", "50"))
cfg = C.default_config(T, num_shards=K, net_model=C.NET_EMESH_HOP_BY_HOP)
be = B.Backend(cfg)
addr = torch.empty(T * N, dtype=torch.int64, device="cuda")
meta = torch.empty(T * N, dtype=torch.int32, device="cuda")
B.gen_hotspot_trace(addr, meta, 0, T, N, hot_lines=H)
offs = np.arange(T + 1, dtype=np.uint64) * np.uint64(N)
out = torch.zeros(T * N, dtype=torch.int64, device="cuda")


def timed(label, stats, interval, runs=RUNS):
    be.stats_trace_configure(stats, interval, 1 << 12)
    for _ in range(2):
        be.coherent_run(addr, meta, offs, out)
    torch.cuda.synchronize()
    ts = []
    for _ in range(runs):
        t0 = time.perf_counter()
        be.coherent_run(addr, meta, offs, out)
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    n = len(be.stats_trace()["time_ns"]) if stats else 0
    r = {"label": label, "ms_per_run": ts, "median_ms": float(np.median(ts)), "samples": n}
    print(json.dumps(r), flush=True)
    return r


res = []
if os.environ.get("COST_SCAN_ONLY") != "1":
    res.append(timed("trace off", 0, 0))
    ref = out.clone()
    res.append(timed("scan launches, no sample due (interval 1e9 ns)", 3, 10 ** 9))
    assert torch.equal(out, ref)
    res.append(timed("network_utilization, 10000 ns", 1, 10000))
    res.append(timed("both statistics, 10000 ns", 3, 10000))
    assert torch.equal(out, ref)
    res.append(timed("trace off again", 0, 0))
# the scan alone on the end-of-run state: gg_stats_trace_sample = launch + sync
be.stats_trace_configure(3, 10 ** 9, SCANS + 8)
be.coherent_run(addr, meta, offs, out)
torch.cuda.synchronize()
t0 = time.perf_counter()
for i in range(SCANS):
    be.stats_trace_sample(10 ** 9 * (i + 1))
dt = (time.perf_counter() - t0) / SCANS
tr = be.stats_trace()
E = 16384                                    # directory entries per tile (auto sizing at 1024 tiles)
per_tile = E * 16 + 128 * 4 + 1024 * 8        # directory entries + L1-D meta + L2 meta bytes
r = {"label": "gg_stats_trace_sample: host time per call (launch + synchronise), not kernel time",
     "us_per_call": dt * 1e6, "bytes_read_per_scan": T * per_tile,
     "last": {k: int(tr[k][-1]) for k in ("l1_exclusive", "l1_shared", "l2_exclusive", "l2_shared")},
     "hist_nonzero_bins": int((tr["sharer_hist"][-1] > 0).sum()), "hist_max_sharers": int(np.nonzero(tr["sharer_hist"][-1])[0].max())}
print(json.dumps(r), flush=True)
res.append(r)
if os.environ.get("COST_OUT"):
    json.dump(res, open(os.environ["COST_OUT"], "w"), indent=1)
be.close()
