"""Cost of miss-type tracking (gg_cache_track_miss_types) on the bench's
`private` workload (1024 tiles x 2^20 configs[1] uniform-random accesses,
default geometry, streaming replay): accesses/s with both caches tracked
against the same library with tracking off.  Whole replays from a reset state
(host clock around a batch ending in a synchronise), 2 warm-ups + RUNS timed,
median.  Every line of a tile is touched, so each (tile, L1-D set) holds
32768 / 128 = 256 distinct lines: COST_LINES (default 65536) gives 512 slots
per unit, a load factor of one half at the end of the run.

  python tools/modep_miss_types_cost.py                  -> one JSON line per measurement
  python tools/modep_miss_types_cost.py --resource-usage -> the tracking kernels' registers / LDS / scratch
                                                            (compiles gg_cache.hip; needs no GPU)
"""
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

if "--resource-usage" in sys.argv:
    table = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "resource_usage.py"), "gg_cache"],
                           capture_output=True, text=True, check=True).stdout.splitlines()
    print("\n".join(table[:2] + [r for r in table[2:] if ", true>`" in r and ("k_cache_stream<" in r or
                                                                                "k_cache_replay<" in r or "k_quartet<" in r)]))
    sys.exit(0)

import torch                               # noqa: E402
from graphite_amd import backend as B      # noqa: E402
from graphite_amd import config as C       # noqa: E402

T = int(os.environ.get("COST_TILES", "1024"))
N = int(os.environ.get("COST_PER_TILE", str(1 << 20)))
RUNS = int(os.environ.get("COST_RUNS", "5"))
LINES = int(os.environ.get("COST_LINES", "65536"))
n = T * N
addr = torch.empty(n, dtype=torch.int64, device="cuda")
meta = torch.empty(n, dtype=torch.int32, device="cuda")
result = torch.empty(n, dtype=torch.int32, device="cuda")
B.gen_uniform_trace(addr, meta, 0, T, N)
offs = np.arange(T + 1, dtype=np.uint64) * np.uint64(N)


def timed(label, track, replay_kernel=0):
    cfg = C.default_config(T, replay_kernel=replay_kernel, l1i_track_miss_types=track, l2_track_miss_types=track)
    be = B.Backend(cfg)
    if track:
        be.cache_track_miss_types(LINES)
    ts = []
    for it in range(2 + RUNS):
        be.reset()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        be.cache_access_batch(addr, meta, offs, result, None)
        torch.cuda.synchronize()
        if it >= 2:
            ts.append(time.perf_counter() - t0)
    cc = be.cache_counters()                 # (also reports a full table)
    r = {"label": label, "seconds": ts, "median_s": float(np.median(ts)), "accesses_per_s": n / float(np.median(ts)),
         "l1d_misses": int(cc[:, 0, C.CACHE_COUNTERS.index("misses")].sum()),
         "l2_misses": int(cc[:, 1, C.CACHE_COUNTERS.index("misses")].sum())}
    if track:
        mt = be.cache_miss_types()
        assert (mt.sum(axis=2) == cc[:, :, C.CACHE_COUNTERS.index("misses")]).all()
        r["miss_types_l1d"] = [int(x) for x in mt[:, 0].sum(axis=0)]
        r["miss_types_l2"] = [int(x) for x in mt[:, 1].sum(axis=0)]
    print(json.dumps(r), flush=True)
    be.close()
    return r, result.clone()


res = []
off, ref = timed("tracking off (streaming replay)", 0)
on, got = timed("both caches tracked, %d lines (streaming tracking instance)" % LINES, 1)
assert torch.equal(ref, got)                 # tracking changes no result word
gen, got = timed("both caches tracked, %d lines (sharded generic tracking kernel)" % LINES, 1, replay_kernel=1)
assert torch.equal(ref, got)
off2, _ = timed("tracking off again", 0)
base = 0.5 * (off["accesses_per_s"] + off2["accesses_per_s"])
summary = {"label": "ratio tracked / untracked accesses per second", "streaming": on["accesses_per_s"] / base,
           "generic": gen["accesses_per_s"] / base,
           "table_bytes": T * 2 * LINES * 8, "misses_per_access_l1d": on["l1d_misses"] / n,
           "misses_per_access_l2": on["l2_misses"] / n}
print(json.dumps(summary), flush=True)
res = [off, on, gen, off2, summary]
if os.environ.get("COST_OUT"):
    json.dump(res, open(os.environ["COST_OUT"], "w"), indent=1)
