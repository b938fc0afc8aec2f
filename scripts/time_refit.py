#!/usr/bin/env python3
"""Timing of the classifier.4 refit (csrc/head_refit.hip, neuralbarkcalculator_amd/refit.py) on one GPU.
usage: python scripts/time_refit.py --kernels [N]
           at 1, 2 and 8 x 1024x1024 (or at N alone), in fp32 and f16x2: launch loops (WARM + REPS calls, device events around the loop) of the
           forward, nbc_head_logits, nbc_upsample_argmax, nbc_pixel_cross_entropy, nbc_ce_gradient and nbc_head_gradient, all in
           this process on the features of the same forward, each beside the bytes it must move at the streaming rate; then
           nbc_lovasz_softmax and nbc_lovasz_gradient (Lovasz alone, and mixed with the table) on the same buffers.  Run it
           under `rocprofv3 --kernel-trace --stats -d DIR -- python ...` for per-launch kernel times, then
       python scripts/time_refit.py parse DIR
           medians per kernel from the kernel trace under DIR (every launch of the run pooled: trace one batch size)
       python scripts/time_refit.py --folder N [--precision f16x2] [--loss ce|lovasz|mixed]
           refit_folder on a synthetic folder of N 1024x1024 samples (scripts/time_evaluate.py's): seconds per objective
           evaluation and for a refit of 20 evaluations"""
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

WARM, REPS = 5, 50
BATCHES = (1, 2, 8)
H = W = 1024
KERNELS = ("head_theta_scale", "head1x1_kernel", "ce_pixel_gradient", "ce_col_adjoint", "ce_row_adjoint", "head_grad_partial",
           "head_grad_finish", "pixel_ce_partial", "upsample_argmax", "lovasz_keys", "lovasz_hist", "lovasz_scan", "lovasz_scatter",
           "lovasz_tile_fg", "lovasz_partial", "lovasz_fg_prefix", "lovasz_pixel_gradient")
HBM_BYTES_PER_S = 6.29e12


def byte_bounds(n, precision, h=H // 8, w=W // 8):
    """The bytes each call must move, from its shapes."""
    P, cells, eb = H * W, h * w, (2 if precision == "bf16" else 4)
    return {"head_logits": n * cells * (512 * eb + 12), "upsample_argmax": n * (12 * cells + 13 * P),
            "pixel_cross_entropy": n * 13 * P, "ce_gradient": n * ((13 + 24) * P + 24 * P + 24 * H * w + 24 * H * w + 24 * cells),
            "ce_gradient.pixel": n * (13 + 24) * P, "ce_gradient.columns": n * (24 * P + 24 * H * w),
            "ce_gradient.rows": n * (24 * H * w + 24 * cells), "head_gradient": n * cells * (512 * eb + 24),
            # beyond nbc_lovasz_softmax: the copy of the keys (12 + 12), the prefix pass (12 + 12), the pixel pass (13 + 12 in,
            # 24 out, its searches apart), the two adjoint passes
            "lovasz_gradient - lovasz_softmax": n * ((24 + 24 + 49) * P + 24 * P + 48 * H * w + 24 * cells)}


def loop(fn):
    import torch
    for _ in range(WARM):
        fn()
    torch.cuda.synchronize()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(REPS):
        fn()
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1) * 1e3 / REPS


def kernels(batches=BATCHES):
    import numpy as np
    import torch
    from neuralbarkcalculator_amd import refit, synth
    from neuralbarkcalculator_amd.model import FCNResNet50
    dev = torch.device("cuda", 0)
    sd = synth.make_state_dict("trained_like", seed=7)
    theta = torch.from_numpy(refit.theta_of(sd)).to(dev)
    T = refit.table_of("weighted_ce")
    for precision in ("fp32", "f16x2"):
        m = FCNResNet50(precision).load_state_dict(sd).to(dev)
        for n in batches:
            x = torch.from_numpy(np.stack([synth.make_frame(i, H, W) for i in range(n)])).to(dev)
            tgt = x[..., 1].contiguous()
            m.lowres_logits(x)
            low = m.head_logits(theta)
            _, _, full = m.upsample_argmax(low, (H, W), labels_dtype=torch.uint8, return_logits=True)
            gl = m.ce_gradient(full, tgt, low.shape[2:], T)
            us = {"forward": loop(lambda: m.lowres_logits(x))}
            m.lowres_logits(x)
            us["head_logits"] = loop(lambda: m.head_logits(theta))
            us["upsample_argmax"] = loop(lambda: m.upsample_argmax(low, (H, W), labels_dtype=torch.uint8, logits_full=full))
            us["pixel_cross_entropy"] = loop(lambda: m.pixel_cross_entropy(full, tgt))
            us["ce_gradient"] = loop(lambda: m.ce_gradient(full, tgt, low.shape[2:], T))
            us["head_gradient"] = loop(lambda: m.head_gradient(gl))
            us["head_loss_and_gradient"] = loop(lambda: m.head_loss_and_gradient(tgt, theta, T, logits_full=full))
            us["lovasz_softmax"] = loop(lambda: m.lovasz_softmax(full, tgt))
            us["lovasz_gradient"] = loop(lambda: m.lovasz_gradient(full, tgt, low.shape[2:]))
            us["lovasz_gradient, mixed"] = loop(lambda: m.lovasz_gradient(full, tgt, low.shape[2:], T / (4.0 * H * W), 1.0))
            us["lovasz_gradient - lovasz_softmax"] = us["lovasz_gradient"] - us["lovasz_softmax"]
            us["head_loss_and_gradient, mixed"] = loop(lambda: m.head_loss_and_gradient(tgt, theta, T / (4.0 * H * W), logits_full=full,
                                                                                        lovasz_weight=1.0))
            bounds = byte_bounds(n, precision)
            print("%s, %d x %dx%d (loops of %d calls, launch gaps included):" % (precision, n, H, W, REPS), flush=True)
            for name, t in us.items():
                b = bounds.get(name)
                print("  %-24s %9.1f us per call%s" % (name, t, "" if b is None else "; %d bytes, %.1f us at the streaming rate"
                                                       % (b, b / HBM_BYTES_PER_S * 1e6)), flush=True)
            new = us["head_logits"] + us["ce_gradient"] + us["head_gradient"]
            print("  the three new calls together %.1f us = %.1f %% of the forward they follow" % (new, 100 * new / us["forward"]), flush=True)
        del m
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
        us = np.array([(int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3 for r in rows if kernel in r["Kernel_Name"]])
        if len(us):
            print("%s: %d launches, median %.2f us (p10 %.2f, p90 %.2f; every batch size and precision of the run pooled)"
                  % (kernel, len(us), np.median(us), np.percentile(us, 10), np.percentile(us, 90)))


def folder(n, precision, loss="ce"):
    from neuralbarkcalculator_amd import refit
    import time_evaluate
    root = tempfile.mkdtemp(prefix="nbc_refit_")
    try:
        ckpt = time_evaluate.make_folder(root, n)
        out = os.path.join(root, "refit_model.pt")
        for iterations in (1, 9):                       # at most 2 x iterations + 2 evaluations: 4 and 20
            t0 = time.perf_counter()
            st = refit.refit_folder(root, out, ckpt, **{"image_loss" if loss in refit.LOVASZ_LOSSES else "loss": loss}, iterations=iterations, precision=precision, device_index=0)
            dt = time.perf_counter() - t0
            ev = st["summary"]["evaluations"]
            print("refit %s --loss %s, %d images, --iterations %d: %d evaluations in %.2f s end to end (%.2f s set-up), %.3f s per evaluation "
                  "in the loops; a 20-evaluation refit at that rate %.1f s" % (precision, loss, n, iterations, ev, dt, st["setup_s"],
                                                                             (dt - st["setup_s"]) / ev, st["setup_s"] + 20 * (dt - st["setup_s"]) / ev),
                  flush=True)
            print("  " + refit.format_summary(st["summary"]).splitlines()[0], flush=True)
    finally:
        shutil.rmtree(root, ignore_errors=True)


if __name__ == "__main__":
    args = sys.argv[1:]
    if args[:1] == ["--kernels"]:
        kernels(BATCHES if len(args) < 2 else (int(args[1]),))
    elif args[:1] == ["parse"] and len(args) == 2:
        parse(args[1])
    elif args[:1] == ["--folder"] and len(args) >= 2:
        folder(int(args[1]), args[args.index("--precision") + 1] if "--precision" in args else "f16x2",
               args[args.index("--loss") + 1] if "--loss" in args else "ce")
    else:
        raise SystemExit(__doc__)
