#!/usr/bin/env python3
"""The fused (downsample.0 + conv3) launches against the launches they replace, from two rocprofv3 kernel traces of the same
one-stream bench command (f16x2, batch 1): one of a build that runs the pairs as two launches, one of a build that fuses.
  rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python3 bench.py --full --frames 8 --precision f16x2 \
      --batch 1 --streams 1 --steps 12 --warmup 3 --no-bf16-leg --no-f32-leg --no-cpu-baseline --no-parity --no-autotune --no-op-events
  python scripts/fused_pair_table.py DIR_TWO_LAUNCHES DIR_FUSED
A forward is the launches from an ingest to the next upsample_argmax; forwards of the most common length are kept and their
first three dropped (warm-up).  The plan's launch order is fixed (nbc_plan.cpp): per stage-entry bottleneck conv1, conv2,
downsample.0, conv3, so in the two-launch trace the pair of stage s is the s-th (1x1 without ReLU, identity 1x1) couple --
found here by position: the launch in front of each launch that the fused trace replaces by a kVarDualBranch one."""
import csv
import glob
import os
import statistics
import sys


def forwards(d):
    path = glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True)[0]
    rows = [r for r in csv.DictReader(open(path)) if "nbc::" in r["Kernel_Name"]]
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    out, cur = [], None
    for r in rows:
        if "ingest" in r["Kernel_Name"]:
            cur = []
        if cur is not None:
            cur.append(r)
            if "upsample_argmax" in r["Kernel_Name"]:
                out.append(cur)
                cur = None
    n = statistics.mode(len(f) for f in out)
    return [f for f in out if len(f) == n][3:], n


def us(r):
    return (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3


def med(fw, k):
    return statistics.median(us(f[k]) for f in fw)


two, n2 = forwards(sys.argv[1])
one, n1 = forwards(sys.argv[2])
print("launches per forward: %d (two launches per pair), %d (fused); forwards used: %d, %d" % (n2, n1, len(two), len(one)))
tot2 = statistics.median(sum(us(r) for r in f) for f in two)
tot1 = statistics.median(sum(us(r) for r in f) for f in one)
wall2 = statistics.median((int(f[-1]["End_Timestamp"]) - int(f[0]["Start_Timestamp"])) / 1e3 for f in two)
wall1 = statistics.median((int(f[-1]["End_Timestamp"]) - int(f[0]["Start_Timestamp"])) / 1e3 for f in one)
print("sum of kernel durations per forward, median: %.1f us -> %.1f us (%+.1f us); first start to last end: %.1f us -> %.1f us (%+.1f us)"
      % (tot2, tot1, tot1 - tot2, wall2, wall1, wall1 - wall2))
fused = [k for k, r in enumerate(one[0]) if "ELi16ELb0E" in r["Kernel_Name"] or ", 16, false>" in r["Kernel_Name"]]
print("fused launches at positions", fused)
saved = 0.0
for s, k in enumerate(fused):
    k2 = k + s + 1                       # the same conv3 in the two-launch trace: one more launch in front per earlier pair
    d, c3, f = med(two, k2 - 1), med(two, k2), med(one, k)
    saved += d + c3 - f
    print("pair %d: downsample.0 %.1f us (grid %s) + conv3 %.1f us (grid %s) = %.1f us  ->  fused %.1f us (grid %s): %+.1f us"
          % (s + 1, d, two[0][k2 - 1]["Grid_Size_X"], c3, two[0][k2]["Grid_Size_X"], d + c3, f, one[0][k]["Grid_Size_X"], f - d - c3))
print("the three pairs together: %+.1f us per forward" % -saved)
rest2 = tot2 - sum(med(two, k + s + 1) + med(two, k + s) for s, k in enumerate(fused))
rest1 = tot1 - sum(med(one, k) for k in fused)
print("every other launch together: %.1f us -> %.1f us" % (rest2, rest1))
