#!/usr/bin/env python3
"""Timing of the dataset-statistics path (csrc/dataset_stats.hip, neuralbarkcalculator_amd/stats.py) on one GPU.
usage: python scripts/time_stats.py kernels
           launch loops of nbc_image_moments and nbc_target_counts at 1024x1024 x batch 2 and x batch 8, and of
           nbc_image_moments on one 4096x4096 frame: WARM + REPS launches per case, in this order, each case rotating over
           enough distinct buffers (more than 256 MB together) that no launch finds its input in the caches.  Prints
           device-event times of whole loops; run it under `rocprofv3 --kernel-trace --stats -d DIR -- python ...` for
           per-launch kernel times, then
       python scripts/time_stats.py parse DIR
           medians and spread per case from the kernel trace under DIR (its CSV or its database; cases told apart by
           launch order)
       python scripts/time_stats.py folder [n_images=1000]
           stats_folder on the synthetic labelled folder of scripts/time_evaluate.py, twice, and evaluate_folder (f16x2) once
           on the same folder for comparison; the stage profile of stats_folder (r.prof) is printed by NBC_FOLDER_PROFILE=1"""
import csv
import glob
import os
import shutil
import sys
import tempfile
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

WARM, REPS = 10, 200
CASES = [("image_moments", 2, 1024, 1024), ("image_moments", 8, 1024, 1024), ("image_moments", 1, 4096, 4096),
         ("target_counts", 2, 1024, 1024), ("target_counts", 8, 1024, 1024)]
HBM_BYTES_PER_S = 6.29e12


def case_bytes(kind, n, h, w):
    return n * h * w * (3 if kind == "image_moments" else 1)


def kernels():
    import torch
    from neuralbarkcalculator_amd import stats as st
    dev = torch.device("cuda", 0)
    for kind, n, h, w in CASES:
        nbytes = case_bytes(kind, n, h, w)
        shape = (n, h, w, 3) if kind == "image_moments" else (n, h, w)
        bufs = [torch.randint(0, 256, shape, dtype=torch.uint8, device=dev) for _ in range(max(2, (320 << 20) // nbytes + 1))]
        fn = st.image_moments if kind == "image_moments" else st.target_counts
        for i in range(WARM):
            fn(bufs[i % len(bufs)])
        torch.cuda.synchronize()
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        for i in range(REPS):
            fn(bufs[i % len(bufs)])
        t1.record()
        torch.cuda.synchronize()
        print("%s %dx%dx%d: %d bytes, %d buffers, loop of %d calls (memset + kernel + launch gaps) %.2f us per call; "
              "byte bound %.2f us" % (kind, n, h, w, nbytes, len(bufs), REPS, t0.elapsed_time(t1) * 1e3 / REPS,
                                      nbytes / HBM_BYTES_PER_S * 1e6), flush=True)
        del bufs
        torch.cuda.empty_cache()


def parse(folder):
    import numpy as np
    rows = []
    for path in glob.glob(os.path.join(folder, "**", "*kernel_trace.csv"), recursive=True):
        with open(path) as f:
            rows += list(csv.DictReader(f))
    for path in glob.glob(os.path.join(folder, "**", "*_results.db"), recursive=True):      # rocprofv3's default output
        import sqlite3
        with sqlite3.connect(path) as db:
            rows += [{"Kernel_Name": n, "Start_Timestamp": a, "End_Timestamp": b}
                     for n, a, b in db.execute("select name, start, end from kernels")]
    for kernel in ("image_moments_kernel", "target_counts_kernel"):
        mine = sorted((int(r["Start_Timestamp"]), int(r["End_Timestamp"])) for r in rows if kernel in r["Kernel_Name"])
        cases = [c for c in CASES if c[0] + "_kernel" == kernel]
        print("%s: %d launches in the trace (%d expected)" % (kernel, len(mine), len(cases) * (WARM + REPS)))
        for j, (kind, n, h, w) in enumerate(cases):
            part = mine[j * (WARM + REPS) + WARM: (j + 1) * (WARM + REPS)]
            if len(part) != REPS:
                continue
            us = np.array([(b - a) / 1e3 for a, b in part])
            nbytes = case_bytes(kind, n, h, w)
            print("  %dx%dx%d: median %.2f us (p10 %.2f, p90 %.2f, min %.2f, %d launches), byte bound %.2f us, "
                  "%.2f TB/s at the median" % (n, h, w, np.median(us), np.percentile(us, 10), np.percentile(us, 90), us.min(),
                                               len(us), nbytes / HBM_BYTES_PER_S * 1e6, nbytes / np.median(us) / 1e6))


def folder(n):
    from time_evaluate import make_folder
    from neuralbarkcalculator_amd import evaluate as ev, predict as drv, stats as st
    root = tempfile.mkdtemp(prefix="nbc_stats_")
    try:
        t0 = time.perf_counter()
        ckpt = make_folder(root, n)
        print(f"folder of {n} synthetic 1024x1024 .bmp samples with grey .png duals made in {time.perf_counter() - t0:.1f} s; "
              f"host workers {drv._host_workers()}, cores available {len(os.sched_getaffinity(0))}", flush=True)
        os.environ["NBC_FOLDER_PROFILE"] = "1"
        for what in ("stats", "evaluate", "stats"):
            shutil.rmtree(os.path.join(root, "results"), ignore_errors=True)
            t0 = time.perf_counter()
            run = st.stats_folder(root, device_index=0) if what == "stats" else \
                ev.evaluate_folder(root, ckpt, precision="f16x2", device_index=0)
            dt = time.perf_counter() - t0
            print(f"{what}: {n} images end to end in {dt:.2f} s = {n / dt:.1f} images/s (setup {run['setup_s']:.2f} s "
                  f"included); steady loop {run['images_per_s_loop']:.1f} images/s", flush=True)
            if what == "stats":
                print("  " + st.format_summary(run["summary"]).replace("\n", "\n  "), flush=True)
    finally:
        shutil.rmtree(root, ignore_errors=True)


if __name__ == "__main__":
    mode = sys.argv[1] if len(sys.argv) > 1 else ""
    if mode == "kernels":
        kernels()
    elif mode == "parse":
        parse(sys.argv[2])
    elif mode == "folder":
        folder(int(sys.argv[2]) if len(sys.argv) > 2 else 1000)
    else:
        raise SystemExit(__doc__)
