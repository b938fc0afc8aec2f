#!/usr/bin/env python3
"""Medians per row-step launch (tile 19: layer2.1-3 conv2; tile 20: layer3 / layer4 conv2 and classifier.0, in plan order) and
the forward's kernel sum from rocprofv3 kernel traces of the one-stream bench command (f16x2, batch 1; the command:
scripts/fused_pair_table.py):
  python scripts/rowstep_launch_table.py DIR [DIR ...]
  python scripts/rowstep_launch_table.py --against PARENT_A PARENT_B NEW    every launch of the forward side by side: the medians of
      two runs of the parent's build, their difference (the parent's own run-to-run spread), the median of the new build's run
      against the parents' mean, and a mark where a launch is slower than both parent runs by more than their difference
A forward is the launches from an ingest to the next upsample_argmax; forwards of the most common length are kept and their
first three dropped (warm-up)."""
import csv, glob, os, re, statistics, sys
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
is_rowstep = lambda r: "conv3x3_rowstep_kernel" in r["Kernel_Name"]
names = ["layer2.%d.conv2" % i for i in range(1, 4)] + ["layer3.%d.conv2" % i for i in range(6)] + ["layer4.%d.conv2" % i for i in range(3)] + ["classifier.0"]
def short(r):
    m = re.search(r"nbc::(?:\(anonymous namespace\)::)?(\w+)(<[^>]*>)?", r["Kernel_Name"])
    return (m.group(1) + (m.group(2) or "")) if m else r["Kernel_Name"][:40]
if len(sys.argv) > 1 and sys.argv[1] == "--against":
    (fa, na), (fb, nb), (fn, nn) = (forwards(d) for d in sys.argv[2:5])
    assert na == nb == nn, (na, nb, nn)
    med = lambda fw, k: statistics.median(us(f[k]) for f in fw)
    rs = iter(names)
    print("launch  kernel                                         parent a  parent b  |a - b|      new   new - parents' mean")
    slower, sums = [], [0.0, 0.0, 0.0]
    for k in range(na):
        a, b, c = med(fa, k), med(fb, k), med(fn, k)
        row = is_rowstep(fa[0][k])
        label = next(rs) if row and na == 55 else ""
        mark = ""
        if c > max(a, b) + abs(a - b):
            mark = "  slower beyond the parents' spread"
            if not row:
                slower.append(k)
        for i, v in enumerate((a, b, c)):
            sums[i] += v
        print("%4d    %-46s %8.1f  %8.1f  %7.1f  %8.1f  %+8.1f us  %s%s" % (k, short(fa[0][k])[:46], a, b, abs(a - b), c, c - (a + b) / 2, label, mark))
    print("sum of the medians: parent a %.1f, parent b %.1f, new %.1f us; launches outside the row-step kernel slower beyond the spread: %s" % (
        sums[0], sums[1], sums[2], slower or "none"))
    sys.exit(0)
for d in sys.argv[1:]:
    fw, n = forwards(d)
    pos = [k for k, r in enumerate(fw[0]) if is_rowstep(r)]
    tot = statistics.median(sum(us(r) for r in f) for f in fw)
    wall = statistics.median((int(f[-1]["End_Timestamp"]) - int(f[0]["Start_Timestamp"])) / 1e3 for f in fw)
    print("%s: %d launches per forward, %d forwards; kernel sum %.1f us, first start to last end %.1f us" % (d, n, len(fw), tot, wall))
    s = 0.0
    for nm, k in zip(names[-len(pos):], pos):
        m = statistics.median(us(f[k]) for f in fw); s += m
        print("  %-16s grid %6s  median %.1f us  min %.1f" % (nm, fw[0][k]["Grid_Size_X"], m, min(us(f[k]) for f in fw)))
    print("  row-step launches together %.1f us (%d of them)" % (s, len(pos)))
