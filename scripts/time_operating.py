#!/usr/bin/env python3
"""Timing of the operating-point sweep of `evaluate --operating_points` (csrc/offset_sweep.hip) and of `--logit_offsets` on
one GPU.
usage: python scripts/time_operating.py --kernels
           launch loops of nbc_offset_sweep at 1024x1024 x batch 1, 2 and 8, on the default 33 x 33 grid and on a 1 x 1 grid,
           each followed by the same loop of nbc_softmax_census (target on, no plane) on the same buffers (it reads the same
           13 bytes per pixel: the yardstick): WARM + REPS calls per loop, rotating over enough distinct inputs (more than
           256 MB together) that no launch finds its input in the caches.  Two kinds of logits per shape, scripts/
           time_calibration.py's: "spread" (normal x 3: the switch indices spread over the table) and "confident" (one class
           leads by about 10 on every pixel, class 0 on nine pixels of ten: what a trained network gives, nearly every pixel
           of a wave in one LDS word per i).  Then the forward (predict_labels, f16x2, 1024x1024 x batch 2) with and without
           logit offsets, alternated.  Prints device-event times of whole loops.
       python scripts/time_operating.py --folder N [--precision f16x2]
           evaluate_folder on a synthetic folder of N 1024x1024 samples (scripts/time_evaluate.py's) plain, with
           --operating_points and with --logit_offsets, alternated, twice each: images/s in the loop, best against best"""
import os
import shutil
import sys
import tempfile
import time

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, ".."))
sys.path.insert(0, HERE)

WARM, REPS = 10, 100
CASES = [(kind, n, 1024, 1024) for n in (1, 2, 8) for kind in ("spread", "confident")]
HBM_BYTES_PER_S = 6.29e12


def kernels():
    import numpy as np
    import torch
    from neuralbarkcalculator_amd import _lib, operating as op, synth
    from neuralbarkcalculator_amd.model import FCNResNet50
    from time_calibration import case_bytes, make_logits
    lib = _lib.load()
    dev = torch.device("cuda", 0)
    stream = torch.cuda.current_stream(dev)
    gen = torch.Generator(device=dev).manual_seed(0)
    fp = _lib.C.POINTER(_lib.C.c_float)
    full = np.ascontiguousarray(op.parse_grid(op.DEFAULT_GRID))
    one = np.zeros(1, np.float32)
    for kind, n, h, w in CASES:
        nbytes = case_bytes(n, h, w)
        count = max(2, (320 << 20) // nbytes + 1)
        inputs = [(make_logits(torch, kind, n, h, w, gen, dev),
                   torch.randint(0, 256, (n, h, w), dtype=torch.uint8, device=dev, generator=gen)) for _ in range(count)]
        need = lib.nbc_offset_sweep_workspace_bytes(n, h, w, 33, 33)
        ws = torch.empty(need, dtype=torch.uint8, device=dev)
        conf = torch.empty((n, 33, 33, 3, 3), dtype=torch.int64, device=dev)
        cneed = lib.nbc_softmax_census_workspace_bytes(n, h, w)
        cws = torch.empty(cneed, dtype=torch.uint8, device=dev)
        rows = torch.empty((n, _lib.CENSUS_WORDS), dtype=torch.int64, device=dev)

        def sweep(grid):
            def fn(i):
                lg, tg = inputs[i % count]
                _lib.check(lib.nbc_offset_sweep(lg.data_ptr(), tg.data_ptr(), n, h, w, grid.ctypes.data_as(fp), grid.size,
                                                grid.ctypes.data_as(fp), grid.size, ws.data_ptr(), need, conf.data_ptr(),
                                                stream.cuda_stream), "nbc_offset_sweep")
            return fn

        def census(i):
            lg, tg = inputs[i % count]
            _lib.check(lib.nbc_softmax_census(lg.data_ptr(), tg.data_ptr(), n, h, w, cws.data_ptr(), cneed, rows.data_ptr(), None,
                                              stream.cuda_stream), "nbc_softmax_census")

        for name, fn in (("nbc_offset_sweep 33x33", sweep(full)), ("nbc_offset_sweep 1x1", sweep(one)), ("nbc_softmax_census", census)):
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
        del inputs, ws, cws
        torch.cuda.empty_cache()

    # the forward with and without offsets: the offset kernels do two more additions per pixel
    sd = synth.make_state_dict("trained_like", seed=7)
    m = FCNResNet50("f16x2").load_state_dict(sd).to(dev)
    x = torch.from_numpy(np.stack([synth.make_input(3, 1024, 1024)] * 2)).to(dev)
    best = {}
    for rep in range(3):
        for name, pair in (("plain", (0.0, 0.0)), ("offsets", (-1.5, -5.5))):
            m.set_logit_offsets(*pair)
            for _ in range(3):
                m.predict_labels(x, labels_dtype=torch.uint8)
            torch.cuda.synchronize()
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            for _ in range(20):
                m.predict_labels(x, labels_dtype=torch.uint8)
            t1.record()
            torch.cuda.synchronize()
            ms = t0.elapsed_time(t1) / 20
            best[name] = min(best.get(name, ms), ms)
            print("forward f16x2 2x1024x1024 %s run %d: %.3f ms per forward" % (name, rep, ms), flush=True)
    print("forward f16x2 2x1024x1024: best %.3f ms plain, %.3f ms with --logit_offsets (%.1f %%)"
          % (best["plain"], best["offsets"], 100 * best["offsets"] / best["plain"]), flush=True)


def folder(n, precision):
    from neuralbarkcalculator_amd import evaluate as ev
    import time_evaluate
    root = tempfile.mkdtemp(prefix="nbc_operating_")
    try:
        ckpt = time_evaluate.make_folder(root, n)
        rates = {}
        modes = (("plain", {}), ("operating_points", dict(operating_points=True)), ("logit_offsets", dict(logit_offsets=(-1.5, -5.5))))
        for rep in range(2):
            for name, kw in modes:
                shutil.rmtree(os.path.join(root, "results"), ignore_errors=True)
                t0 = time.perf_counter()
                st = ev.evaluate_folder(root, ckpt, precision=precision, device_index=0, **kw)
                dt = time.perf_counter() - t0
                rates.setdefault(name, []).append(st["images_per_s_loop"])
                print(f"evaluate {precision} {name} run {rep}: {n} images in {dt:.2f} s end to end; steady loop "
                      f"{st['images_per_s_loop']:.1f} images/s", flush=True)
                if name == "operating_points":
                    print("  " + "\n  ".join(ln for ln in ev.format_summary(st["summary"]).splitlines() if ln.startswith("operating point")),
                          flush=True)
        best = {k: max(v) for k, v in rates.items()}
        print(f"evaluate {precision}: loop {best['plain']:.1f} images/s plain, {best['operating_points']:.1f} with --operating_points "
              f"({100 * best['operating_points'] / best['plain']:.1f} %), {best['logit_offsets']:.1f} with --logit_offsets "
              f"({100 * best['logit_offsets'] / best['plain']:.1f} %)", flush=True)
    finally:
        shutil.rmtree(root, ignore_errors=True)


if __name__ == "__main__":
    args = sys.argv[1:]
    if args[:1] == ["--kernels"]:
        kernels()
    elif args[:1] == ["--folder"] and len(args) >= 2:
        folder(int(args[1]), args[args.index("--precision") + 1] if "--precision" in args else "f16x2")
    else:
        raise SystemExit(__doc__)
