#!/usr/bin/env python3
"""Summary of tools/profile_shade_records.sh's output directory: per k_shade instance the calls and time of the
--kernel-trace --stats pass and every counter of the PMC passes, summed over dispatches, with the ratios the record
moves are judged by (vector-L1 -> L2 requests per path-round, L2 hit share, vector-L1 busy share)."""
import csv
import glob
import os
import re
import sys
from collections import defaultdict

out = sys.argv[1]


def short(name):
    m = re.search(r"k_shade<(\w+), (\d+), (\w+)(?:, (\w+))?>", name)
    if not m:
        return None
    return "k_shade<%s,%s,%s%s>" % (m.group(1), m.group(2), m.group(3), "," + m.group(4) if m.group(4) else "")


def find(pattern):
    return sorted(glob.glob(os.path.join(out, pattern), recursive=True))


print(f"# shade-kernel record traffic: {os.path.basename(out)}")
time_ns = {}
for path in find("stats/**/*kernel_stats.csv"):
    for r in csv.DictReader(open(path)):
        k = short(r["Name"])
        if k:
            time_ns[k] = float(r["TotalDurationNs"])
            print(f"{k:32s} calls {r['Calls']:>6s}  total {float(r['TotalDurationNs']) / 1e6:10.2f} ms  {float(r['Percentage']):5.2f} % of kernel time")
acc = defaultdict(lambda: defaultdict(float))
for grp in ("l1_l2", "l2", "l1_busy"):
    for path in find(f"{grp}/**/*counter_collection.csv"):
        for r in csv.DictReader(open(path)):
            k = short(r["Kernel_Name"])
            if k:
                acc[k][r["Counter_Name"]] += float(r["Counter_Value"])
                # one record per path and dispatch lane: Grid_Size is the threads launched, an upper bound of the queue
                if grp == "l1_l2" and r["Counter_Name"] == "TCP_TCC_READ_REQ_sum":
                    acc[k]["threads_launched"] += float(r.get("Grid_Size", 0) or 0)
for k in sorted(acc):
    c = acc[k]
    print(f"\n## {k}")
    for name in sorted(c):
        print(f"  {name:32s} {c[name]:.6g}")
    rd, wr, req = c.get("TCP_TCC_READ_REQ_sum"), c.get("TCP_TCC_WRITE_REQ_sum"), c.get("TCC_REQ_sum")
    hit, miss = c.get("TCC_HIT_sum"), c.get("TCC_MISS_sum")
    if rd is not None and wr is not None and k in time_ns:
        print(f"  vector L1 -> L2: {rd / time_ns[k]:.2f} G read req/s, {wr / time_ns[k]:.2f} G write req/s (un-profiled kernel time of the stats pass)")
    if rd is not None and wr is not None and c.get("threads_launched"):
        print(f"  per launched thread (>= one per path-round): {rd / c['threads_launched']:.2f} read + {wr / c['threads_launched']:.2f} write requests")
    if req and k in time_ns:
        print(f"  L2 requests: {req / time_ns[k]:.2f} G/s")
    if hit is not None and miss is not None and hit + miss > 0:
        print(f"  L2 hit share: {hit / (hit + miss):.3f}")
    if c.get("TCP_GATE_EN1_sum"):
        print(f"  vector L1 busy share (TCP_GATE_EN2 / TCP_GATE_EN1): {c.get('TCP_GATE_EN2_sum', 0) / c['TCP_GATE_EN1_sum']:.3f}")
