#!/usr/bin/env python3
"""The colour-jitter views of `predict --jitter` / `evaluate --jitter` on one GPU.
  --kernels     the two entry points alone, by device events over back-to-back calls at 1024 x 1024 into buffers allocated
                once: nbc_jitter_views on a uint8 frame with the "training" set (five views, no contrast pass) and with a
                contrast view added (six views, one grey-sum pass), nbc_views_mean on the 128 x 128 logits of five views --
                with the bytes each moves and the rate that makes
  --calls       FCNResNet50.predict_labels_jitter("training") against predict_labels on the same box, per precision, at the
                folder driver's default batch (1; 2 in bf16), with remove_small_zones: the call per image over V x the plain
                call per image, with and without the views' own figures (return_views), and the share of the new kernels
  --folder N    predict_folder on a synthetic folder of N 1024 x 1024 samples (scripts/time_evaluate.py's folder) without
                and with jitter = training, alternated, twice each: images/s end to end and in the loop
usage: python scripts/time_jitter.py [--kernels] [--calls] [--folder N] [--precision fp32 f16x2 bf16]"""
import argparse
import os
import shutil
import sys
import tempfile
import time

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, ".."))
sys.path.insert(0, HERE)
import numpy as np
import torch

from neuralbarkcalculator_amd import _lib, synth
from neuralbarkcalculator_amd.model import JITTER_TRAINING, FCNResNet50, resolve_jitter_views

HW = 1024
V = len(JITTER_TRAINING)


def _timed(call, reps):
    for _ in range(3):
        call()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        call()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps


def time_kernels(n=1, reps=200):
    """{name: ms} of the kernels for n images of 1024 x 1024."""
    dev = torch.device("cuda", 0)
    lib = _lib.load()
    u8 = torch.from_numpy(np.stack([synth.make_frame(3 + i, HW, HW) for i in range(n)])).to(dev)
    px = n * HW * HW
    stream = torch.cuda.current_stream().cuda_stream
    out = {}
    for name, views, passes in (("nbc_jitter_views training", JITTER_TRAINING, 0),
                                ("nbc_jitter_views training + (1, 1.2, 1)", JITTER_TRAINING + ((1.0, 1.2, 1.0),), 1)):
        f = resolve_jitter_views(views)
        v = len(f)
        stack = torch.empty((v * n, HW, HW, 3), dtype=torch.uint8, device=dev)
        ws = torch.empty((v * n,), dtype=torch.int64, device=dev)
        call = lambda: _lib.check(lib.nbc_jitter_views(u8.data_ptr(), n, HW, HW, f.ctypes.data, v, stack.data_ptr(), ws.data_ptr(), stream))
        ms = _timed(call, reps)
        nbytes = px * 3 * (1 + v + passes)
        out[name] = ms
        print(f"{name}: {n} x {HW}x{HW}, {v} views: {1e3 * ms:.1f} us per call over {reps} calls, {nbytes / 2**20:.1f} MiB moved = "
              f"{nbytes / ms / 1e9:.2f} TB/s", flush=True)
    low = torch.randn((V * n, 3, HW // 8, HW // 8), device=dev)
    mean = torch.empty((n, 3, HW // 8, HW // 8), device=dev)
    ms = _timed(lambda: _lib.check(lib.nbc_views_mean(low.data_ptr(), n, V, HW // 8, HW // 8, mean.data_ptr(), stream)), reps)
    nbytes = n * 3 * (HW // 8) ** 2 * 4 * (V + 1)
    out["nbc_views_mean"] = ms
    print(f"nbc_views_mean: {n} x 3 x {HW // 8}x{HW // 8}, {V} views: {1e3 * ms:.1f} us per call over {reps} calls, "
          f"{nbytes / 2**20:.2f} MiB moved = {nbytes / ms / 1e9:.3f} TB/s (a launch, not a stream: the size is the product's)", flush=True)
    return out


def time_calls(precisions, reps=20):
    dev = torch.device("cuda", 0)
    sd = synth.make_state_dict("trained_like", seed=7)
    for precision in precisions:
        n = 2 if precision == "bf16" else 1
        kern = time_kernels(n, reps=50)
        model = FCNResNet50(precision).load_state_dict(sd).to(dev)
        x = torch.from_numpy(np.stack([synth.make_frame(3 + i, HW, HW) for i in range(n)])).to(dev)
        kw = dict(labels_dtype=torch.uint8, small_zones=True)
        results = {"plain": [], "jitter": [], "full": []}
        for _ in range(2):                               # alternated: the box is shared
            results["plain"].append(_timed(lambda: model.predict_labels(x, **kw), reps))
            results["jitter"].append(_timed(lambda: model.predict_labels_jitter(x, "training", **kw), reps))
            results["full"].append(_timed(lambda: model.predict_labels_jitter(x, "training", return_views=True, **kw), reps))
        plain, jit, full = (min(results[k]) for k in ("plain", "jitter", "full"))
        new = kern["nbc_jitter_views training"] + kern["nbc_views_mean"]
        print(f"{precision} batch {n}: predict_labels {plain / n:.3f} ms per image ({1e3 * n / plain:.1f} images/s); "
              f"predict_labels_jitter training {jit / n:.3f} ms per image ({1e3 * n / jit:.1f} images/s) = {jit / (V * plain):.3f} x "
              f"(V x the plain call); with the views' own figures {full / n:.3f} ms per image ({1e3 * n / full:.1f} images/s) = "
              f"{full / (V * plain):.3f} x; the new kernels' share: {100 * new / jit:.2f} % of the call; both runs: "
              f"{', '.join('%s %s' % (k, ['%.3f' % t for t in ts]) for k, ts in results.items())} ms", flush=True)


def time_folder(n, precision):
    from neuralbarkcalculator_amd import predict as drv
    import time_evaluate
    root = tempfile.mkdtemp(prefix="nbc_jitter_")
    try:
        ckpt = time_evaluate.make_folder(root, n)
        shutil.rmtree(os.path.join(root, "duals"), ignore_errors=True)
        modes = [None, "training"]
        loop, e2e = {t: [] for t in modes}, {t: [] for t in modes}
        for rep in range(2):
            for t in modes:
                shutil.rmtree(os.path.join(root, "results"), ignore_errors=True)
                shutil.rmtree(os.path.join(root, "processed"), ignore_errors=True)
                t0 = time.perf_counter()
                st = drv.predict_folder(root, ckpt, precision=precision, device_index=0, jitter=t)
                dt = time.perf_counter() - t0
                loop[t].append(st["images_per_s_loop"])
                e2e[t].append(n / dt)
                print(f"predict {precision} jitter={t} run {rep}: {n} images end to end in {dt:.2f} s = {n / dt:.1f} images/s (setup "
                      f"{st['setup_s']:.2f} s included, batch {st['batch']}); steady loop {st['images_per_s_loop']:.1f} images/s", flush=True)
        for t in modes:
            print(f"predict {precision} jitter={t}: best loop {max(loop[t]):.1f} images/s ({100 * max(loop[t]) / max(loop[None]):.1f} % of "
                  f"none), best end to end {max(e2e[t]):.1f} images/s", flush=True)
    finally:
        shutil.rmtree(root, ignore_errors=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--kernels", action="store_true")
    ap.add_argument("--calls", action="store_true")
    ap.add_argument("--folder", type=int, default=0)
    ap.add_argument("--precision", nargs="+", default=["f16x2"])
    args = ap.parse_args()
    if args.kernels:
        time_kernels()
    if args.calls:
        time_calls(args.precision)
    if args.folder:
        for precision in args.precision:
            time_folder(args.folder, precision)


if __name__ == "__main__":
    main()
