#!/usr/bin/env python3
"""Timing of the softmax census of `evaluate --calibration` (csrc/softmax_census.hip) on one GPU.
usage: python scripts/time_calibration.py kernels
           launch loops of nbc_softmax_census (target and confidence plane on) at 1024x1024 x batch 2 and x batch 8, each
           followed by the same loop of nbc_pixel_cross_entropy on the same inputs (it reads the same 13 bytes per pixel and
           does three exp and a log where the census does three exp and three divisions: the yardstick): WARM + REPS calls
           per loop, rotating over enough distinct inputs (more than 256 MB together) that no launch finds its input in the
           caches.  Two kinds of logits per shape: "spread" (normal x 3: every bin of the histograms is hit) and "confident"
           (one class leads by about 10 on every pixel, class 0 on nine pixels of ten: what a trained network gives, nearly
           every probability in bin 0 or 255).  Prints device-event times of whole loops; run it under
           `rocprofv3 --kernel-trace --stats -d DIR -- python ...` for per-launch kernel times, then
       python scripts/time_calibration.py parse DIR
           medians and spread per kernel and case from the kernel trace under DIR (cases told apart by launch order)
       python scripts/time_calibration.py --folder N [--precision f16x2]
           evaluate_folder on a synthetic folder of N 1024x1024 samples (scripts/time_evaluate.py's) plain, with ce and with
           calibration, alternated, twice each: images/s in the loop, best against best"""
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

WARM, REPS = 10, 100
CASES = [(kind, n, 1024, 1024) for n in (2, 8) for kind in ("spread", "confident")]
KERNELS = ("census_partial", "census_finish", "pixel_ce_partial", "pixel_ce_finish")
HBM_BYTES_PER_S = 6.29e12


def case_bytes(n, h, w):
    return n * h * w * 13                           # three f32 planes and one target byte per pixel


def make_logits(torch, kind, n, h, w, gen, dev):
    x = torch.randn((n, 3, h, w), generator=gen, device=dev) * 3
    if kind == "confident":
        lead = torch.randint(0, 20, (n, 1, h, w), device=dev, generator=gen)
        lead = torch.where(lead < 18, 0, lead - 17)                       # 90 % class 0, 5 % each of the others
        x = x / 3 + 10.0 * (torch.arange(3, device=dev).view(1, 3, 1, 1) == lead)
    return x.contiguous()


def kernels():
    import torch
    from neuralbarkcalculator_amd import _lib
    lib = _lib.load()
    dev = torch.device("cuda", 0)
    stream = torch.cuda.current_stream(dev)
    gen = torch.Generator(device=dev).manual_seed(0)
    for kind, n, h, w in CASES:
        nbytes = case_bytes(n, h, w)
        count = max(2, (320 << 20) // nbytes + 1)
        inputs = [(make_logits(torch, kind, n, h, w, gen, dev),
                   torch.randint(0, 256, (n, h, w), dtype=torch.uint8, device=dev, generator=gen)) for _ in range(count)]
        need = lib.nbc_pixel_ce_workspace_bytes(n, h, w)
        ws = torch.empty(need, dtype=torch.uint8, device=dev)
        sums = torch.empty((n, 3, 3), dtype=torch.float64, device=dev)
        counts = torch.empty((n, 3, 3), dtype=torch.int64, device=dev)
        cneed = lib.nbc_softmax_census_workspace_bytes(n, h, w)
        cws = torch.empty(cneed, dtype=torch.uint8, device=dev)
        rows = torch.empty((n, _lib.CENSUS_WORDS), dtype=torch.int64, device=dev)
        plane = torch.empty((n, h, w), dtype=torch.uint8, device=dev)

        def census(i):
            lg, tg = inputs[i % count]
            _lib.check(lib.nbc_softmax_census(lg.data_ptr(), tg.data_ptr(), n, h, w, cws.data_ptr(), cneed, rows.data_ptr(),
                                              plane.data_ptr(), stream.cuda_stream), "nbc_softmax_census")

        def ce(i):
            lg, tg = inputs[i % count]
            _lib.check(lib.nbc_pixel_cross_entropy(lg.data_ptr(), tg.data_ptr(), n, h, w, ws.data_ptr(), need, sums.data_ptr(),
                                                   counts.data_ptr(), stream.cuda_stream), "nbc_pixel_cross_entropy")

        for name, fn in (("nbc_softmax_census", census), ("nbc_pixel_cross_entropy", ce)):
            for i in range(WARM):
                fn(i)
            torch.cuda.synchronize()
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            for i in range(REPS):
                fn(i)
            t1.record()
            torch.cuda.synchronize()
            print("%s %s %dx%dx%d: %d input bytes, %d inputs, loop of %d calls (kernels + launch gaps) %.2f us per call; "
                  "byte bound of the inputs %.2f us" % (name, kind, n, h, w, nbytes, count, REPS, t0.elapsed_time(t1) * 1e3 / REPS,
                                                        nbytes / HBM_BYTES_PER_S * 1e6), flush=True)
        r = rows[0].cpu().numpy()
        ends = int(r[0:_lib.CENSUS_R:256].sum() + r[255:_lib.CENSUS_R:256].sum())
        print("  image 0 of the last call: %d of its %d histogram entries in bins 0 and 255, %d hits of %d pixels"
              % (ends, int(r[:_lib.CENSUS_R].sum()), int(r[_lib.CENSUS_R + 256: _lib.CENSUS_RS].sum()), h * w), flush=True)
        del inputs, ws, cws
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
        for j, (kind, n, h, w) in enumerate(CASES):
            part = mine[j * (WARM + REPS) + WARM: (j + 1) * (WARM + REPS)]
            if len(part) != REPS:
                continue
            us = np.array([(b - a) / 1e3 for a, b in part])
            print("  %s %dx%dx%d: median %.2f us (p10 %.2f, p90 %.2f, min %.2f, %d launches), byte bound of the inputs %.2f us"
                  % (kind, n, h, w, np.median(us), np.percentile(us, 10), np.percentile(us, 90), us.min(), len(us),
                     case_bytes(n, h, w) / HBM_BYTES_PER_S * 1e6))


def folder(n, precision):
    from neuralbarkcalculator_amd import evaluate as ev
    import time_evaluate
    root = tempfile.mkdtemp(prefix="nbc_calibration_")
    try:
        ckpt = time_evaluate.make_folder(root, n)
        rates = {}
        modes = (("plain", {}), ("ce", dict(ce=True)), ("calibration", dict(calibration=True)))
        for rep in range(2):
            for name, kw in modes:
                shutil.rmtree(os.path.join(root, "results"), ignore_errors=True)
                t0 = time.perf_counter()
                st = ev.evaluate_folder(root, ckpt, precision=precision, device_index=0, **kw)
                dt = time.perf_counter() - t0
                rates.setdefault(name, []).append(st["images_per_s_loop"])
                print(f"evaluate {precision} {name} run {rep}: {n} images in {dt:.2f} s end to end; steady loop "
                      f"{st['images_per_s_loop']:.1f} images/s", flush=True)
                if name == "calibration":
                    print("  " + [ln for ln in ev.format_summary(st["summary"]).splitlines() if ln.startswith("calibration")][0], flush=True)
        best = {k: max(v) for k, v in rates.items()}
        print(f"evaluate {precision}: loop {best['plain']:.1f} images/s plain, {best['ce']:.1f} with --ce "
              f"({100 * best['ce'] / best['plain']:.1f} %), {best['calibration']:.1f} with --calibration "
              f"({100 * best['calibration'] / best['plain']:.1f} %)", flush=True)
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
