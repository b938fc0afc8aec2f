#!/usr/bin/env python3
"""Timing of the cross-entropy sums of `evaluate --ce` (csrc/pixel_ce.hip) on one GPU.
usage: python scripts/time_pixel_ce.py kernels
           launch loops of nbc_pixel_cross_entropy at 1024x1024 x batch 2 and x batch 8, each followed by the same loop of
           nbc_lovasz_softmax on the same inputs (its lovasz_keys kernel reads the same bytes: the yardstick): WARM + REPS
           calls per loop, rotating over enough distinct inputs (more than 256 MB together) that no launch finds its input
           in the caches.  Prints device-event times of whole loops; run it under
           `rocprofv3 --kernel-trace --stats -d DIR -- python ...` for per-launch kernel times, then
       python scripts/time_pixel_ce.py parse DIR
           medians and spread per kernel and case from the kernel trace under DIR (cases told apart by launch order)
       python scripts/time_pixel_ce.py --folder N [--precision f16x2]
           evaluate_folder on a synthetic folder of N 1024x1024 samples (scripts/time_evaluate.py's) with ce off / on
           alternated, twice each, then with loss and with loss + ce, twice each: images/s in the loop, best against best"""
import csv
import glob
import os
import shutil
import sys
import tempfile
import time

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, ".."))
sys.path.insert(0, HERE)

WARM, REPS = 10, 200
CASES = [(2, 1024, 1024), (8, 1024, 1024)]
KERNELS = ("pixel_ce_partial", "pixel_ce_finish", "lovasz_keys")
HBM_BYTES_PER_S = 6.29e12


def case_bytes(n, h, w):
    return n * h * w * 13                           # three f32 planes and one target byte per pixel


def kernels():
    import torch
    from neuralbarkcalculator_amd import _lib
    lib = _lib.load()
    dev = torch.device("cuda", 0)
    stream = torch.cuda.current_stream(dev)
    gen = torch.Generator(device=dev).manual_seed(0)
    for n, h, w in CASES:
        nbytes = case_bytes(n, h, w)
        count = max(2, (320 << 20) // nbytes + 1)
        inputs = [(torch.randn((n, 3, h, w), generator=gen, device=dev) * 3,
                   torch.randint(0, 256, (n, h, w), dtype=torch.uint8, device=dev, generator=gen)) for _ in range(count)]
        need = lib.nbc_pixel_ce_workspace_bytes(n, h, w)
        ws = torch.empty(need, dtype=torch.uint8, device=dev)
        sums = torch.empty((n, 3, 3), dtype=torch.float64, device=dev)
        counts = torch.empty((n, 3, 3), dtype=torch.int64, device=dev)
        lneed = lib.nbc_lovasz_workspace_bytes(n, h, w)
        lws = torch.empty(lneed, dtype=torch.uint8, device=dev)
        terms = torch.empty((n, 3), dtype=torch.float64, device=dev)
        fg = torch.empty((n, 3), dtype=torch.int64, device=dev)

        def ce(i):
            lg, tg = inputs[i % count]
            _lib.check(lib.nbc_pixel_cross_entropy(lg.data_ptr(), tg.data_ptr(), n, h, w, ws.data_ptr(), need, sums.data_ptr(),
                                                   counts.data_ptr(), stream.cuda_stream), "nbc_pixel_cross_entropy")

        def lovasz(i):
            lg, tg = inputs[i % count]
            _lib.check(lib.nbc_lovasz_softmax(lg.data_ptr(), tg.data_ptr(), n, h, w, lws.data_ptr(), lneed, terms.data_ptr(),
                                              fg.data_ptr(), stream.cuda_stream), "nbc_lovasz_softmax")

        for name, fn in (("nbc_pixel_cross_entropy", ce), ("nbc_lovasz_softmax", lovasz)):
            for i in range(WARM):
                fn(i)
            torch.cuda.synchronize()
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            for i in range(REPS):
                fn(i)
            t1.record()
            torch.cuda.synchronize()
            print("%s %dx%dx%d: %d input bytes, %d inputs, loop of %d calls (kernels + launch gaps) %.2f us per call; "
                  "byte bound of the inputs %.2f us" % (name, n, h, w, nbytes, count, REPS, t0.elapsed_time(t1) * 1e3 / REPS,
                                                        nbytes / HBM_BYTES_PER_S * 1e6), flush=True)
        print("  cross_entropy of image 0 of the last call: %r" % (float(sums[0].sum().cpu()) / (h * w)), flush=True)
        del inputs, ws, lws
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
    for kernel in KERNELS:
        mine = sorted((int(r["Start_Timestamp"]), int(r["End_Timestamp"])) for r in rows if kernel in r["Kernel_Name"])
        print("%s: %d launches in the trace (%d expected)" % (kernel, len(mine), len(CASES) * (WARM + REPS)))
        for j, (n, h, w) in enumerate(CASES):
            part = mine[j * (WARM + REPS) + WARM: (j + 1) * (WARM + REPS)]
            if len(part) != REPS:
                continue
            us = np.array([(b - a) / 1e3 for a, b in part])
            print("  %dx%dx%d: median %.2f us (p10 %.2f, p90 %.2f, min %.2f, %d launches), byte bound of the inputs %.2f us"
                  % (n, h, w, np.median(us), np.percentile(us, 10), np.percentile(us, 90), us.min(), len(us),
                     case_bytes(n, h, w) / HBM_BYTES_PER_S * 1e6))


def folder(n, precision):
    from neuralbarkcalculator_amd import evaluate as ev
    import time_evaluate
    root = tempfile.mkdtemp(prefix="nbc_pixel_ce_")
    try:
        ckpt = time_evaluate.make_folder(root, n)
        rates = {}
        for pair in (((False, False), (False, True)), ((True, False), (True, True))):
            for rep in range(2):
                for loss, ce in pair:
                    shutil.rmtree(os.path.join(root, "results"), ignore_errors=True)
                    t0 = time.perf_counter()
                    st = ev.evaluate_folder(root, ckpt, precision=precision, device_index=0, loss=loss, ce=ce)
                    dt = time.perf_counter() - t0
                    rates.setdefault((loss, ce), []).append(st["images_per_s_loop"])
                    print(f"evaluate {precision} loss={loss} ce={ce} run {rep}: {n} images in {dt:.2f} s end to end; steady "
                          f"loop {st['images_per_s_loop']:.1f} images/s", flush=True)
                    if ce:
                        print("  " + ev.format_summary(st["summary"]).splitlines()[-1], flush=True)
        best = {k: max(v) for k, v in rates.items()}
        print(f"evaluate {precision}: loop {best[(False, False)]:.1f} images/s without --ce, {best[(False, True)]:.1f} with "
              f"({100 * best[(False, True)] / best[(False, False)]:.1f} %); {best[(True, False)]:.1f} with --loss, "
              f"{best[(True, True)]:.1f} with --loss --ce ({100 * best[(True, True)] / best[(True, False)]:.1f} %)", flush=True)
    finally:
        shutil.rmtree(root, ignore_errors=True)


if __name__ == "__main__":
    args = sys.argv[1:]
    if args[:1] == ["kernels"]:
        kernels()
    elif args[:1] == ["parse"] and len(args) == 2:
        parse(args[1])
    elif args[:1] == ["--folder"] and len(args) >= 2:
        folder(int(args[1]), args[args.index("--precision") + 1] if "--precision" in args else "f16x2")
    else:
        raise SystemExit(__doc__)
