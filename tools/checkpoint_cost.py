"""Cost of a snapshot and a restore (gg_coherent_snapshot / _restore, DESIGN.md
§4i) on the bench's headline run (configs[3]: 1024 tiles x 256 accesses, 256
hot lines, 8 shards, emesh_hop_by_hop) paused near its middle quantum.

  python tools/checkpoint_cost.py          -> JSON lines: the snapshot's bytes by section; wall time of
                                              snapshot and of restore (host clock around a call that ends
                                              in a synchronise, 2 warm-ups + COST_RUNS timed, median); the
                                              device-to-host rate of a pageable copy of the same size and
                                              what the dense directory arrays would take at that rate
  python tools/checkpoint_cost.py --once   -> one snapshot only (for a kernel trace in a run of its own:
                                              rocprofv3 --kernel-trace --stats -- python tools/checkpoint_cost.py --once;
                                              the pack kernels are k_snap_count / k_snap_scan / k_snap_pack)
"""
import json
import os
import struct
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch                               # noqa: E402
from graphite_amd import backend as B      # noqa: E402
from graphite_amd import config as C       # noqa: E402

T = int(os.environ.get("COST_TILES", "1024"))
N = int(os.environ.get("COST_PER_TILE", "256"))
H = int(os.environ.get("COST_HOT_LINES", "256"))
K = int(os.environ.get("COST_SHARDS", "8"))
RUNS = int(os.environ.get("COST_RUNS", "5"))
FINAL = C.RUN_INFO.index("final_quantum")


def sections(blob):
    magic, version, n, total, csum = struct.unpack_from("<QIIQQ", blob, 0)
    out = []
    for i in range(n):
        name, kind, rec, off, size, records = struct.unpack_from("<16sIIQQQ", blob, 32 + 48 * i)
        out.append((name.split(b"\0")[0].decode(), kind, size, records))
    return out


def median(xs):
    return float(np.median(np.asarray(xs)))


cfg = C.default_config(T, num_shards=K, net_model=C.NET_EMESH_HOP_BY_HOP)
n = T * N
addr = torch.empty(n, dtype=torch.int64, device="cuda")
meta = torch.empty(n, dtype=torch.int32, device="cuda")
out = torch.zeros(n, dtype=torch.int64, device="cuda")
B.gen_hotspot_trace(addr, meta, 0, T, N, hot_lines=H)
offs = np.arange(T + 1, dtype=np.uint64) * np.uint64(N)

be = B.Backend(cfg)
be.coherent_run(addr, meta, offs, out)
F = int(be.coherent_stats()[2][FINAL])
be.coherent_begin(addr, meta, offs, out)
nq, done = be.coherent_advance(F // 2)
torch.cuda.synchronize()
assert done == 0

if "--once" in sys.argv:
    blob = be.coherent_snapshot()
    print(json.dumps({"paused_at": nq, "final_quantum": F, "bytes": int(len(blob))}))
    sys.exit(0)

ts, blob = [], None
for it in range(2 + RUNS):
    t0 = time.perf_counter()
    blob = be.coherent_snapshot()
    torch.cuda.synchronize()
    if it >= 2:
        ts.append(time.perf_counter() - t0)
secs = sections(bytes(blob[:32 + 48 * 256]))
W = (T + 63) // 64
E = 2 * cfg.l2_size_kb * 1024 // 64
dense_dir = T * E * (16 + 8 * W)
print(json.dumps({"paused_at": nq, "final_quantum": F, "snapshot_bytes": int(len(blob)),
                  "sections": {s[0]: s[2] for s in secs if s[2]},
                  "packed_records": {s[0]: s[3] for s in secs if s[1] == 1},
                  "dense_directory_bytes": dense_dir}))
print(json.dumps({"snapshot_s_median": median(ts), "snapshot_s_all": ts}))

tr = []
for it in range(2 + RUNS):
    t0 = time.perf_counter()
    be.coherent_restore(blob, addr, meta, offs, out)
    torch.cuda.synchronize()
    if it >= 2:
        tr.append(time.perf_counter() - t0)
print(json.dumps({"restore_s_median": median(tr), "restore_s_all": tr}))

# the dense alternative: the directory arrays over the device-to-host copy rate
# of this box (a pageable host buffer, as the snapshot's)
probe = torch.empty(256 << 20, dtype=torch.uint8, device="cuda")
host = np.empty(probe.numel(), np.uint8)
ht = torch.from_numpy(host)
tc = []
for it in range(2 + RUNS):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    ht.copy_(probe)
    torch.cuda.synchronize()
    if it >= 2:
        tc.append(time.perf_counter() - t0)
rate = probe.numel() / median(tc)
print(json.dumps({"d2h_bytes_per_s": rate, "dense_directory_copy_s": dense_dir / rate,
                  "snapshot_bytes_over_dense": len(blob) / dense_dir}))

# the continuation still ends as the uninterrupted run does
ref = out.clone()
be.coherent_restore(blob, addr, meta, offs, out)
assert be.coherent_advance()[1] == 1
torch.cuda.synchronize()
assert torch.equal(ref, out), "the restored run differs from the uninterrupted one"
be.close()
