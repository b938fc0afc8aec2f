#!/usr/bin/env python3
"""The contour distances of `evaluate --contours` on one GPU.
  kernel        FCNResNet50.contour_distances (nbc_contour_distances) by device events over back-to-back calls on a batch of
                eight 1024x1024 blob maps: against independent blob maps (far contours, long row scans) and against a copy
                moved by (3, -2) pixels (what a good checkpoint next to its masks looks like, short scans); beside it
                contours.contours_cpu on this host, and the bytes the three passes move at least.  `--case NAME` keeps one
                case for a `rocprofv3 --kernel-trace --stats` run, where the launches are contour_mark_kernel,
                column_distance_kernel, row_min_kernel and contour_finish_kernel.
  folder [N]    evaluate_folder on a synthetic labelled folder of N 1024x1024 samples (scripts/time_evaluate.py's folder, the
                duals made from a predict run's label PNGs as scripts/time_zone_match.py makes them, then moved by (3, -2)
                pixels) without and with contours, alternated, twice each: images/s end to end and in the loop.
usage: python scripts/time_contours.py kernel [--case independent|shifted] | folder [N] [--precision f16x2]"""
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

from neuralbarkcalculator_amd import contours, synth
from neuralbarkcalculator_amd.model import FCNResNet50

GREY = np.array([0, 127, 255], dtype=np.uint8)


def blobs(rng, n, h, w, smooth=4, size=15):
    """Class maps of smooth zones some tens of pixels across: thresholded box-filtered noise."""
    from scipy import ndimage
    out = np.empty((n, h, w), dtype=np.uint8)
    for i in range(n):
        f = rng.standard_normal((h, w))
        for _ in range(smooth):
            f = ndimage.uniform_filter(f, size, mode="nearest")
        f /= f.std()
        out[i] = np.where(f > 0.9, 2, np.where(f > 0.0, 1, 0))
    return out


def _window(call, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        call()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps


def time_kernel(only=None, reps=50, rounds=5, n=8, side=1024):
    dev = torch.device("cuda", 0)
    model = FCNResNet50("f16x2").load_state_dict(synth.make_state_dict("trained_like", seed=7)).to(dev)
    rng = np.random.default_rng(0)
    out = blobs(rng, n, side, side)
    cases = {"independent": blobs(rng, n, side, side), "shifted": np.roll(out, (3, -2), axis=(1, 2))}
    labels = torch.from_numpy(out).to(dev)
    # the least traffic: contour_mark reads two bytes and writes one per pixel; column_distance reads the mark and writes the
    # four u16 distances on the way down, and reads both and writes the distances again on the way up; row_min reads both
    floor_bytes = n * side * side * ((2 + 1) + (1 + 8) + (1 + 8 + 8) + (1 + 8))
    for name, tgt in cases.items():
        if only not in (None, name):
            continue
        grey = torch.from_numpy(GREY[tgt]).to(dev)
        t0 = time.perf_counter()
        want = contours.contours_cpu(out, GREY[tgt])
        cpu_ms = 1e3 * (time.perf_counter() - t0)
        rows, sum_d = (t.cpu().numpy() for t in model.contour_distances(labels, grey))
        ok = np.array_equal(rows, want[0]) and bool(np.all(np.abs(sum_d - want[1]) <= (want[0][:, :, 0] + 2) * 2.0 ** -52 * want[1]))
        head = want[0][:, :, :contours.HEAD].sum(axis=0)

        def call():
            model.contour_distances(labels, grey)
        for _ in range(3):
            call()
        torch.cuda.synchronize()
        ms = [_window(call, reps) for _ in range(rounds)]
        med = float(np.median(ms))
        print(f"{n}x{side}x{side} blob maps against {name} ones: {int(head[:, 0].sum())} source contour pixels "
              f"({100 * head[:, 0].sum() / (4 * n * side * side):.2f} % per set), mean distance "
              f"{want[1].sum() / max(1, head[:, 0].sum()):.2f} px, largest d2 {int(want[0][:, :, 3].max())}; equal to contours_cpu: {ok}",
              flush=True)
        print(f"contour_distances {1e3 * med:.1f} us per call ({1e3 * med / n:.1f} per image; windows {1e3 * min(ms):.1f} .. "
              f"{1e3 * max(ms):.1f}; {rounds} windows of {reps} calls, median); at least {floor_bytes / 1e6:.0f} MB moved = "
              f"{floor_bytes / (med * 1e-3) / 1e12:.2f} TB/s of it; contours.contours_cpu {cpu_ms:.0f} ms ({cpu_ms / n:.0f} per image)",
              flush=True)


def _shift_duals(root):
    from PIL import Image
    top = os.path.join(root, "duals")
    for wood in sorted(os.listdir(top)):
        for name in sorted(os.listdir(os.path.join(top, wood))):
            path = os.path.join(top, wood, name)
            Image.fromarray(np.roll(np.asarray(Image.open(path)), (3, -2), axis=(0, 1)), mode="L").save(path)


def time_folder(n, precision):
    from neuralbarkcalculator_amd import evaluate as drv
    import time_evaluate
    import time_zone_match
    root = tempfile.mkdtemp(prefix="nbc_contours_")
    try:
        ckpt = time_evaluate.make_folder(root, n)
        time_zone_match._realistic_duals(root, ckpt, precision)
        _shift_duals(root)
        loop, e2e = {False: [], True: []}, {False: [], True: []}
        for rep in range(2):
            for flag in (False, True):
                shutil.rmtree(os.path.join(root, "results"), ignore_errors=True)
                t0 = time.perf_counter()
                st = drv.evaluate_folder(root, ckpt, precision=precision, device_index=0, **(dict(contours=True) if flag else {}))
                dt = time.perf_counter() - t0
                loop[flag].append(st["images_per_s_loop"])
                e2e[flag].append(n / dt)
                note = ""
                if flag:
                    c = st["summary"]["contours"]
                    note = "; " + ", ".join(f"{k} F1 {c[k]['f1']}, mean {c[k]['mean_distance_mm']} mm" for k in ("Bark", "Node"))
                print(f"evaluate {precision} contours={int(flag)} run {rep}: {n} images ({st['summary']['images_evaluated']} evaluated) "
                      f"end to end in {dt:.2f} s = {n / dt:.1f} images/s "
                      f"(setup {st['setup_s']:.2f} s included); steady loop {st['images_per_s_loop']:.1f} images/s{note}", flush=True)
        for flag in (False, True):
            print(f"evaluate {precision} contours={int(flag)}: best loop {max(loop[flag]):.1f} images/s "
                  f"({100 * max(loop[flag]) / max(loop[False]):.1f} % of the run without), best end to end {max(e2e[flag]):.1f} images/s",
                  flush=True)
    finally:
        shutil.rmtree(root, ignore_errors=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("what", choices=["kernel", "folder"])
    ap.add_argument("n", type=int, nargs="?", default=96, help="folder: the number of samples")
    ap.add_argument("--precision", default="f16x2")
    ap.add_argument("--case", choices=["independent", "shifted"], default=None, help="kernel: only this case")
    args = ap.parse_args()
    if args.what == "kernel":
        time_kernel(args.case)
    else:
        time_folder(args.n, args.precision)


if __name__ == "__main__":
    main()
