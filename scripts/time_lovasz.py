#!/usr/bin/env python3
"""The Lovasz-Softmax loss of `evaluate --loss` on one GPU.
  --kernels     nbc_lovasz_softmax alone on 1024x1024 batches of 2 (random logits, all three classes present), timed with
                device events over back-to-back calls on one stream: ms per call and per image (run it under
                `rocprofv3 --kernel-trace --stats` for the per-kernel split)
  --folder N    evaluate_folder with and without loss=True on a synthetic folder of N 1024x1024 samples
                (scripts/time_evaluate.py's folder), alternated, twice each: images/s in the loop
usage: python scripts/time_lovasz.py [--kernels] [--folder N] [--precision f16x2]"""
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

from neuralbarkcalculator_amd import _lib


def time_kernels(reps=50, n=2, hw=1024):
    lib = _lib.load()
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(0)
    logits = torch.from_numpy((rng.normal(size=(n, 3, hw, hw)) * 3).astype(np.float32)).to(dev)
    grey = torch.from_numpy(rng.integers(0, 256, size=(n, hw, hw), dtype=np.uint8)).to(dev)
    need = lib.nbc_lovasz_workspace_bytes(n, hw, hw)
    ws = torch.empty(need, dtype=torch.uint8, device=dev)
    terms = torch.empty((n, 3), dtype=torch.float64, device=dev)
    counts = torch.empty((n, 3), dtype=torch.int64, device=dev)
    stream = torch.cuda.current_stream(dev)

    def call():
        _lib.check(lib.nbc_lovasz_softmax(logits.data_ptr(), grey.data_ptr(), n, hw, hw, ws.data_ptr(), need, terms.data_ptr(),
                                          counts.data_ptr(), stream.cuda_stream), "nbc_lovasz_softmax")
    for _ in range(5):
        call()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        call()
    b.record()
    torch.cuda.synchronize()
    ms = a.elapsed_time(b) / reps
    moved = n * 3 * hw * hw * 4 * (1 + 4 * 3 + 2) + n * hw * hw * (3 * 4 + 1)   # keys, 4 x (hist, scatter r + w), scan; inputs
    print(f"nbc_lovasz_softmax {n}x{hw}x{hw}: {ms:.4f} ms per call, {ms / n:.4f} ms per image over {reps} calls; "
          f"~{moved / 1e6:.0f} MB moved per call ({moved / ms / 1e6:.0f} GB/s); workspace {need / 2**20:.1f} MiB; "
          f"terms {terms.cpu().numpy().round(6).tolist()}", flush=True)


def time_folder(n, precision):
    from neuralbarkcalculator_amd import evaluate as ev
    import time_evaluate
    root = tempfile.mkdtemp(prefix="nbc_lovasz_")
    try:
        ckpt = time_evaluate.make_folder(root, n)
        rates = {False: [], True: []}
        for rep in range(2):
            for loss in (False, True):
                shutil.rmtree(os.path.join(root, "results"), ignore_errors=True)
                t0 = time.perf_counter()
                st = ev.evaluate_folder(root, ckpt, precision=precision, device_index=0, loss=loss)
                dt = time.perf_counter() - t0
                rates[loss].append(st["images_per_s_loop"])
                print(f"evaluate {precision} loss={loss} run {rep}: {n} images in {dt:.2f} s end to end; steady loop "
                      f"{st['images_per_s_loop']:.1f} images/s", flush=True)
                if loss:
                    print("  " + ev.format_summary(st["summary"]).splitlines()[-1], flush=True)
        best = {k: max(v) for k, v in rates.items()}
        print(f"evaluate {precision}: loop {best[False]:.1f} images/s without --loss, {best[True]:.1f} with "
              f"({100 * best[True] / best[False]:.1f} %)", flush=True)
    finally:
        shutil.rmtree(root, ignore_errors=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--kernels", action="store_true")
    ap.add_argument("--folder", type=int, default=0)
    ap.add_argument("--precision", default="f16x2")
    args = ap.parse_args()
    if args.kernels:
        time_kernels()
    if args.folder:
        time_folder(args.folder, args.precision)


if __name__ == "__main__":
    main()
