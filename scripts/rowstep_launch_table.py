#!/usr/bin/env python3
"""Medians per row-step launch (tile 20: layer3 / layer4 conv2 and classifier.0, in plan order) and the forward's kernel sum
from rocprofv3 kernel traces of the one-stream bench command (f16x2, batch 1; the command: scripts/fused_pair_table.py):
  python scripts/rowstep_launch_table.py DIR [DIR ...]
A forward is the launches from an ingest to the next upsample_argmax; forwards of the most common length are kept and their
first three dropped (warm-up)."""
import csv, glob, os, statistics, sys
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
                out.append(cur); cur = None
    n = statistics.mode(len(f) for f in out)
    return [f for f in out if len(f) == n][3:], n
us = lambda r: (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3
names = ["layer3.%d.conv2" % i for i in range(6)] + ["layer4.%d.conv2" % i for i in range(3)] + ["classifier.0"]
for d in sys.argv[1:]:
    fw, n = forwards(d)
    pos = [k for k, r in enumerate(fw[0]) if "conv3x3_rowstep_kernel<2, 1, 2, 2>" in r["Kernel_Name"] or "rowstep_kernelILi2ELi1ELi2ELi2E" in r["Kernel_Name"]]
    tot = statistics.median(sum(us(r) for r in f) for f in fw)
    wall = statistics.median((int(f[-1]["End_Timestamp"]) - int(f[0]["Start_Timestamp"])) / 1e3 for f in fw)
    print("%s: %d launches per forward, %d forwards; kernel sum %.1f us, first start to last end %.1f us" % (d, n, len(fw), tot, wall))
    s = 0.0
    for nm, k in zip(names, pos):
        m = statistics.median(us(f[k]) for f in fw); s += m
        print("  %-16s grid %6s  median %.1f us  min %.1f" % (nm, fw[0][k]["Grid_Size_X"], m, min(us(f[k]) for f in fw)))
    print("  row-step launches together %.1f us (%d of them)" % (s, len(pos)))
