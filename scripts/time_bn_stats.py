#!/usr/bin/env python3
"""Forward timing of fcn_resnet50 at batch 1, 1024^2, with BatchNorm on the running statistics (folded into the conv
epilogues) and with per-image statistics (raw conv, then a statistics and an apply kernel per BatchNorm): --precision fp32
times "running" and "image" on the f32 MFMA, --precision f16x2 times "running" and "image_f16x2" on the f16x2 pipe.  HIP
events around the timed forwards, on one stream and (--inflight 2) with two forwards in flight on two contexts that share
the weights; --repeats R alternates the modes R times each, so that the spread between repeats of one mode shows beside the
difference between modes.  Then one profiled pass per mode: the time of the statistics and apply ops, and on the 64 MB and
128 MB layer3/4 outputs their achieved bytes per second against the 6.29 TB/s the HBM delivers to a streaming kernel.
usage: python scripts/time_bn_stats.py [steps=30] [warmup=5] [out.json] [--precision fp32|f16x2] [--inflight 1|2]
       [--repeats R]   (one JSON line per configuration and repeat; all of them together in out.json when it is given)"""
import json
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import numpy as np
import torch
from neuralbarkcalculator_amd import synth
from neuralbarkcalculator_amd.model import fcn_resnet50

STREAM_TBPS = 6.29


def measure(precision, mode, steps, warmup, inflight):
    sd = synth.make_state_dict("trained_like", seed=7)
    m = fcn_resnet50(precision=precision, bn_statistics=mode).load_state_dict(sd).to("cuda:0")
    models = [m] + [m.clone_shared() for _ in range(inflight - 1)]
    streams = [torch.cuda.Stream("cuda:0") for _ in models]
    x = torch.from_numpy(np.stack([synth.make_input(0, 1024, 1024)])).to("cuda:0")
    torch.cuda.synchronize()

    def run(count):
        for i in range(count):
            with torch.cuda.stream(streams[i % inflight]):
                models[i % inflight].lowres_logits(x)

    run(warmup * inflight)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for st in streams:
        st.wait_event(e0)
    run(steps * inflight)
    for st in streams:
        torch.cuda.current_stream().wait_stream(st)
    e1.record()
    torch.cuda.synchronize()
    ms = e0.elapsed_time(e1) / (steps * inflight)
    m.set_profiling(True)
    for _ in range(5):
        m.lowres_logits(x)
    recs = m.op_records()
    m.set_profiling(False)
    return ms, recs, m.nonfinite_seen()


def main():
    import argparse
    ap = argparse.ArgumentParser()
    ap.add_argument("steps", type=int, nargs="?", default=30)
    ap.add_argument("warmup", type=int, nargs="?", default=5)
    ap.add_argument("out", nargs="?", default=None)
    ap.add_argument("--precision", choices=["fp32", "f16x2"], default="fp32")
    ap.add_argument("--inflight", type=int, choices=[1, 2], default=1)
    ap.add_argument("--repeats", type=int, default=1)
    args = ap.parse_args()
    prec = args.precision
    image = "image" if prec == "fp32" else "image_f16x2"
    out = {}
    for rep in range(args.repeats):
        for mode in ("running", image):
            ms, recs, flagged = measure(prec, mode, args.steps, args.warmup, args.inflight)
            row = {"ms_per_forward": ms, "images_per_s": 1000.0 / ms, "inflight": args.inflight, "nonfinite_seen": flagged}
            bn = [r for r in recs if r["kernel"] in ("bn_stats", "bn_apply")]
            if bn:
                row["bn_ms"] = sum(r["ms"] for r in bn)
                for k in ("bn_stats", "bn_apply"):
                    sel = [r for r in bn if r["kernel"] == k]
                    row[k + "_ms"] = sum(r["ms"] for r in sel)
                    row[k + "_tb_per_s"] = sum(r["bytes"] for r in sel) / (row[k + "_ms"] * 1e9)
                row["conv_ms"] = sum(r["ms"] for r in recs if r["kernel"] == "conv_dma")
                big = []
                for r in bn:
                    mb = r["cout"] * 128 * 128 * 4 / 2 ** 20            # the tensor at 1024^2 (layer2-4 maps are 128 x 128)
                    if r["name"].startswith(("backbone.layer3", "backbone.layer4")) and mb in (64.0, 128.0):
                        big.append({"name": r["name"], "kernel": r["kernel"], "tensor_mb": mb, "ms": round(r["ms"], 4),
                                    "tb_per_s": round(r["bytes"] / (r["ms"] * 1e9), 2),
                                    "frac_of_stream": round(r["bytes"] / (r["ms"] * 1e9) / STREAM_TBPS, 3)})
                row["large_tensors"] = big
                for k in ("bn_stats", "bn_apply"):
                    sel = [b for b in big if b["kernel"] == k]
                    if sel:
                        row[k + "_median_frac_of_stream"] = float(np.median([b["frac_of_stream"] for b in sel]))
            out.setdefault("%s b1 %s" % (prec, mode), []).append(row)
            print(json.dumps({"config": "fcn_resnet50 %s b1 bn_stats=%s" % (prec, mode), "repeat": rep,
                              **{k: v for k, v in row.items() if k != "large_tensors"}}), flush=True)
    rate = lambda mode: float(np.median([r["images_per_s"] for r in out["%s b1 %s" % (prec, mode)]]))
    out["image_over_running"] = rate(image) / rate("running")
    print(json.dumps({"image_over_running": out["image_over_running"]}), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
