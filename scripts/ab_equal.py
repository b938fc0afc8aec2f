#!/usr/bin/env python3
"""Do two builds of libnbc_hip.so compute the same bits from the same plan?  Per network, precision and BatchNorm mode, on a few
seeded frames: full-resolution logits and labels, and what each build planned (op records without their timings, plan tiles).
Exit status 1 on any difference.
  gpurun -- 'python scripts/ab_equal.py neuralbarkcalculator_amd/libnbc_hip.so tools/_bin/libnbc_x.so'"""
import ctypes as C
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import numpy as np
import torch
from neuralbarkcalculator_amd import _lib, synth
from neuralbarkcalculator_amd.model import MODELS

dev = torch.device("cuda", 0)
THREE = (([0], 1024, 1024), ([3, 4], 200, 328), ([5], 520, 1024))
TWO = (([5], 520, 1024), ([3, 4], 200, 328))                     # batch 1 and batch 2
# (network, precision, BatchNorm statistics, (frame indices, height, width) ...)
CASES = [("fcn_resnet50", p, "running", THREE) for p in ("f16x2", "fp32", "bf16")]
CASES += [("deeplabv3_resnet50", p, "running", TWO) for p in ("f16x2", "fp32", "bf16")]
CASES += [("fcn_efficientnet_b0", "fp32", "running", TWO), ("deeplabv3_efficientnet_b0", "fp32", "running", TWO),
          ("fcn_resnet50", "fp32", "image", TWO)]
state_dicts = {}


def model_on(path, arch, precision, bn):
    lib = C.CDLL(os.path.abspath(path))
    for name, (res, argtypes) in _lib.SIGNATURES.items():
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = res, argtypes
    if arch not in state_dicts:
        state_dicts[arch] = synth.make_state_dict("trained_like", seed=7, arch=arch)
    keep = _lib._lib
    _lib._lib = lib
    try:
        return MODELS[arch](precision).load_state_dict(state_dicts[arch]).to(dev).set_bn_statistics(bn)
    finally:
        _lib._lib = keep if keep is not None else lib


def run(m, x):
    """logits, labels and the plan of one profiled forward: its op records without the measured fields, its tiles"""
    m.set_profiling(True)
    logits = m(x)
    plan = [{k: v for k, v in r.items() if k not in ("ms", "calls")} for r in m.op_records()]
    m.set_profiling(False)
    return logits, m.predict_labels(x, labels_dtype=torch.uint8)[0], (plan, m.plan_tiles())


bad = 0
for arch, precision, bn, shapes in CASES:
    a, b = model_on(sys.argv[1], arch, precision, bn), model_on(sys.argv[2], arch, precision, bn)
    for idx, h, w in shapes:
        x = torch.from_numpy(np.stack([synth.make_input(i, h, w) for i in idx])).to(dev)
        (la, ya, pa), (lb, yb, pb) = run(a, x), run(b, x)
        same = torch.equal(la, lb) and torch.equal(ya, yb)
        bad += not same or pa != pb
        print("%s %s bn=%s %s x %dx%d: %s (max |logit difference| %.3e), plans %s (%d ops, %d tiles)" %
              (arch, precision, bn, idx, h, w, "identical" if same else "DIFFERENT", float((la - lb).abs().max()),
               "equal" if pa == pb else "DIFFERENT", len(pa[0]), len(pa[1])), flush=True)
    a._destroy()
    b._destroy()
sys.exit(1 if bad else 0)
