#!/usr/bin/env python3
"""The zone inventory of `predict --zones` on one GPU.
  --kernels     FCNResNet50.label_zones (nbc_label_zones, seven launches) by device events over back-to-back calls, beside
                remove_small_zones on the same maps and zones.zones_cpu on this host: 1024x1024 and 520x1024 maps, batches of
                1 and 8, `blobs()`-style maps (thresholded smoothed noise plus salt: a few hundred zones of every size), the
                label maps of the network on synthetic frames, and the two extremes (all one zone; salt only).  Under
                `rocprofv3 --kernel-trace --stats` the launches are zone_tile_kernel, border_rows / _cols_kernel<ClassPlane>,
                count_roots / scan_roots / assign_roots_kernel and accumulate_kernel.
  --folder N    predict_folder on a synthetic folder of N 1024x1024 samples (scripts/time_evaluate.py's folder) without and
                with zones, alternated, twice each: images/s end to end and in the loop.
usage: python scripts/time_zones.py [--kernels [--case 'blobs 1x1024x1024']] [--folder N] [--precision f16x2]"""
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

from neuralbarkcalculator_amd import synth, zones
from neuralbarkcalculator_amd.model import FCNResNet50


def blobs(seed, n, h, w, p_bg, smooth):
    """Random class maps with zones of every size: thresholded smoothed noise plus salt (tests/test_gpu_zones.py's generator)."""
    rng = np.random.default_rng(seed)
    f = rng.standard_normal((n, h, w))
    for _ in range(smooth):
        f = (f + np.roll(f, 1, 1) + np.roll(f, -1, 1) + np.roll(f, 1, 2) + np.roll(f, -1, 2)) / 5.0
    q = np.quantile(f, [p_bg, p_bg + (1 - p_bg) * 0.6])
    lab = np.where(f < q[0], 0, np.where(f < q[1], 1, 2)).astype(np.uint8)
    salt = rng.random((n, h, w)) < 0.01
    lab[salt] = rng.integers(0, 3, size=int(salt.sum()), dtype=np.uint8)
    return lab


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


def time_kernels(reps=50, only=None):
    dev = torch.device("cuda", 0)
    model = FCNResNet50("f16x2").load_state_dict(synth.make_state_dict("trained_like", seed=7)).to(dev)
    def network_labels():
        x = torch.from_numpy(np.stack([synth.make_input(60 + k, 1024, 1024) for k in range(2)])).to(dev)
        return model.predict_labels(x, labels_dtype=torch.uint8, small_zones=True)[0].cpu().numpy()

    def salt():
        rng = np.random.default_rng(1)
        return (rng.random((1, 1024, 1024)) < 0.05).astype(np.uint8) * rng.integers(1, 3, (1, 1024, 1024)).astype(np.uint8)
    cases = [("blobs %dx%dx%d" % (n, h, w), lambda n=n, h=h, w=w: blobs(n + h, n, h, w, 0.6, 6))
             for n, h, w in ((1, 1024, 1024), (8, 1024, 1024), (1, 520, 1024), (8, 520, 1024))]
    cases += [("network labels 2x1024x1024", network_labels), ("one zone 1x1024x1024", lambda: np.ones((1, 1024, 1024), np.uint8)),
              ("salt 1x1024x1024", salt)]
    for name, make in cases:
        if only and only not in name:
            continue
        lab = make()
        n = lab.shape[0]
        t0 = time.perf_counter()
        want = zones.zones_cpu(lab)
        cpu_ms = 1e3 * (time.perf_counter() - t0)
        most = max(len(z) for z in want)
        cap = max(1024, most)
        t = torch.from_numpy(lab).to(dev)
        rows, num = model.label_zones(t, cap=cap)
        torch.cuda.synchronize()
        rows, num = rows.cpu().numpy(), num.cpu().numpy()
        ok = all(int(num[i]) == len(want[i]) and np.array_equal(rows[i, :len(want[i])], want[i]) for i in range(n))
        ms = _timed(lambda: model.label_zones(t, cap=cap), reps)
        scratch = t.clone()
        rz = _timed(lambda: model.remove_small_zones(scratch), reps)      # idempotent after its first call: the same work
        print(f"{name}: {most} zones at most per image, label_zones {1e3 * ms:.1f} us per call ({1e3 * ms / n:.1f} per map), "
              f"remove_small_zones {1e3 * rz:.1f} us per call ({1e3 * rz / n:.1f} per map), ratio {ms / rz:.2f}; zones_cpu "
              f"{cpu_ms:.1f} ms ({cpu_ms / n:.1f} per map); equal to zones_cpu: {ok}", flush=True)


def time_folder(n, precision):
    from neuralbarkcalculator_amd import predict as drv
    import time_evaluate
    root = tempfile.mkdtemp(prefix="nbc_zones_")
    try:
        ckpt = time_evaluate.make_folder(root, n)
        shutil.rmtree(os.path.join(root, "duals"), ignore_errors=True)
        loop, e2e = {False: [], True: []}, {False: [], True: []}
        for rep in range(2):
            for flag in (False, True):
                shutil.rmtree(os.path.join(root, "results"), ignore_errors=True)
                shutil.rmtree(os.path.join(root, "processed"), ignore_errors=True)
                t0 = time.perf_counter()
                st = drv.predict_folder(root, ckpt, precision=precision, device_index=0, zones=flag)
                dt = time.perf_counter() - t0
                loop[flag].append(st["images_per_s_loop"])
                e2e[flag].append(n / dt)
                note = ""
                if flag:
                    lines = sum(1 for _ in open(os.path.join(root, "results", "zones.csv"))) - 1
                    note = f"; {lines} zone rows, {st['zones_host_fallbacks']} host fallbacks, gather and report {st['zones_report_s']:.2f} s"
                print(f"predict {precision} zones={int(flag)} run {rep}: {n} images end to end in {dt:.2f} s = {n / dt:.1f} images/s "
                      f"(setup {st['setup_s']:.2f} s included); steady loop {st['images_per_s_loop']:.1f} images/s{note}", flush=True)
        for flag in (False, True):
            print(f"predict {precision} zones={int(flag)}: best loop {max(loop[flag]):.1f} images/s "
                  f"({100 * max(loop[flag]) / max(loop[False]):.1f} % of the run without), best end to end {max(e2e[flag]):.1f} images/s",
                  flush=True)
    finally:
        shutil.rmtree(root, ignore_errors=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--kernels", action="store_true")
    ap.add_argument("--folder", type=int, default=0)
    ap.add_argument("--precision", default="f16x2")
    ap.add_argument("--case", default=None, help="--kernels: only the cases whose name contains this (for a kernel trace)")
    args = ap.parse_args()
    if args.kernels:
        time_kernels(only=args.case)
    if args.folder:
        time_folder(args.folder, args.precision)


if __name__ == "__main__":
    main()
