"""Kernel times from a rocprofv3 --kernel-trace CSV of tools/stats_trace_cost.py
(COST_SCAN_ONLY=1): per kernel the launches, total, mean and median; for
k_stats_scan the N longest launches apart (the N forced scans of the
end-of-run state; every other launch of it returned at once) with the rate
over the bytes a scan reads at 1024 tiles.

  python tools/stats_trace_scan_times.py KERNEL_TRACE.csv N
"""
import collections
import csv
import sys

f, n = sys.argv[1], int(sys.argv[2])
d = collections.defaultdict(list)
for r in csv.DictReader(open(f)):
    d[r["Kernel_Name"]].append(int(r["End_Timestamp"]) - int(r["Start_Timestamp"]))
for k, v in sorted(d.items(), key=lambda x: -sum(x[1])):
    v.sort()
    print("%-60s n %6d total %10.3f ms mean %8.2f us median %8.2f us"
          % (k[:60], len(v), sum(v) / 1e6, sum(v) / len(v) / 1e3, v[len(v) // 2] / 1e3))
s = sorted(x for k, v in d.items() if "k_stats_scan" in k for x in v)
top, rest = s[-n:], s[:-n]
BYTES = 1024 * (16384 * 16 + 128 * 4 + 1024 * 8)     # directory entries + L1-D + L2 meta bytes of 1024 tiles
print("k_stats_scan, the %d longest (forced scans): mean %.2f us min %.2f max %.2f -> %.0f GB/s over %d bytes read"
      % (n, sum(top) / len(top) / 1e3, top[0] / 1e3, top[-1] / 1e3, BYTES / (sum(top) / len(top)), BYTES))
if rest:
    print("k_stats_scan, the others (early return): n %d total %.3f ms mean %.2f us median %.2f us"
          % (len(rest), sum(rest) / 1e6, sum(rest) / len(rest) / 1e3, rest[len(rest) // 2] / 1e3))
