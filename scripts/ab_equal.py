#!/usr/bin/env python3
"""Do two builds of libnbc_hip.so compute the same bits from the same plan?  Per network, precision and BatchNorm mode, on a few
seeded frames: full-resolution logits and labels, and what each build planned (op records without their timings, plan tiles);
for the ResNet-50 networks also keep-mode reads of a few activations (the max-pool, one unit each of 64, 128, 256 and 2048
channels, DeepLab's pooled vector and concat) and the calibration guard's peaks, byte for byte, on one small batch; for the
EfficientNet DeepLab networks a keep-mode read of the pooled vector (their peaks are not compared: nbc_activation_peaks reports
that vector for them only since their pooling branch is aspp_pool).  An op record that differs only as POOL_RELABEL allows
(a build from before every DeepLab head ran on aspp_pool) is reported and is no difference.
Then the per-image reduction passes on the same seeded inputs, every output buffer byte for byte: nbc_confusion (u8 and i64
labels), nbc_image_moments and nbc_target_counts -- these three also on views that start 1, 5 and 17 bytes off a 16-byte
boundary --, nbc_pixel_cross_entropy, nbc_lovasz_softmax, and dropout_draws (p = 0.1, low-resolution logits, small zones on
and off, a short last pass) in the three precisions.  Exit status 1 on any difference.
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
          ("fcn_efficientnet_b5", "fp32", "running", TWO),              # a 512-wide classifier.4 on the lane-strided kernel
          ("deeplabv3_efficientnet_b6", "fp32", "running", TWO),        # a pooling branch of 2304 channels
          ("fcn_resnet50", "fp32", "image", TWO), ("fcn_resnet50", "f16x2", "image_f16x2", TWO)]
# keep-mode reads, (name, channels): their maps are at most a quarter of the image each way
KEEP_SHAPE = ([3, 4], 200, 328)
KEPT = {"fcn_resnet50": [("backbone.maxpool", 64), ("backbone.layer1.0.conv1", 64), ("backbone.layer2.0.conv1", 128),
                         ("backbone.layer1.0.conv3", 256), ("backbone.layer4.2.conv3", 2048)]}
KEPT["deeplabv3_resnet50"] = KEPT["fcn_resnet50"] + [("classifier.0.convs.4", 256), ("classifier.0.concat", 1280)]
EFF_DEEPLAB = ("deeplabv3_efficientnet_b0", "deeplabv3_efficientnet_b6")
for _arch in EFF_DEEPLAB:
    KEPT[_arch] = [("classifier.0.convs.4", 256)]                    # the pooled vector alone (the peaks count it since aspp_pool)
KEEP_CASES = {("fcn_resnet50", p, "running") for p in ("f16x2", "fp32", "bf16")} | {
    ("deeplabv3_resnet50", "f16x2", "running"), ("deeplabv3_resnet50", "bf16", "running"),
    ("fcn_resnet50", "fp32", "image"), ("fcn_resnet50", "f16x2", "image_f16x2")} | {(a, "fp32", "running") for a in EFF_DEEPLAB}
# the one op record that may differ, and how: the EfficientNet DeepLab pooling branch ran as `pool` in two launches
POOL_RELABEL = ("classifier.0.convs.4", {("pool", 2), ("aspp_pool", 3)})
state_dicts = {}


def lib_of(path):
    lib = C.CDLL(os.path.abspath(path))
    for name, (res, argtypes) in _lib.SIGNATURES.items():
        fn = getattr(lib, name, None)
        if fn is None:                                   # a build of an older revision: calls added since are not made here
            continue
        fn.restype, fn.argtypes = res, argtypes
    return lib


def model_on(path, arch, precision, bn):
    lib = lib_of(path)
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


def kept(m, arch, x):
    """keep-mode reads of one forward, and the stored peaks of another"""
    n, _, h, w = x.shape
    m.set_keep_activations(True)
    m(x)
    out = {name: torch.from_numpy(m.read_activation(name, n * ch * ((h + 3) // 4) * ((w + 3) // 4)).copy()) for name, ch in KEPT[arch]}
    m.set_keep_activations(False)
    if arch not in EFF_DEEPLAB:
        peaks = m.activation_peaks(x)
        out["activation_peaks"] = torch.tensor([peaks[k] for k in sorted(peaks)], dtype=torch.float32)
    return out


def plans_equal(arch, pa, pb):
    """"equal", "DIFFERENT", or equal but for the relabelled pooling branch of an EfficientNet DeepLab network"""
    if pa == pb:
        return "equal"
    (ra, ta), (rb, tb) = pa, pb
    if arch.startswith("deeplabv3_efficientnet") and ta == tb and len(ra) == len(rb):
        rest = lambda r: {k: v for k, v in r.items() if k not in ("kernel", "launches")}
        odd = [(x, y) for x, y in zip(ra, rb) if x != y]
        if all(rest(x) == rest(y) and x["name"] == POOL_RELABEL[0] and
               {(x["kernel"], x["launches"]), (y["kernel"], y["launches"])} == POOL_RELABEL[1] for x, y in odd) and len(odd) == 1:
            return "equal but for %s: %s x %d / %s x %d" % (POOL_RELABEL[0], odd[0][0]["kernel"], odd[0][0]["launches"],
                                                         odd[0][1]["kernel"], odd[0][1]["launches"])
    return "DIFFERENT"


def same_bytes(p, q):
    return p.shape == q.shape and p.dtype == q.dtype and torch.equal(p.contiguous().view(torch.uint8), q.contiguous().view(torch.uint8))


def compare(what, outs_a, outs_b):
    diff = [k for k in outs_a if not same_bytes(outs_a[k], outs_b[k])]
    print("%s: %s" % (what, "identical (%d buffers)" % len(outs_a) if not diff else "DIFFERENT in " + ", ".join(diff)), flush=True)
    return len(diff)


KEEP_CALLS_OK = all(hasattr(lib_of(p), name) for p in sys.argv[1:3]
                    for name in ("nbc_set_keep_activations", "nbc_read_activation", "nbc_activation_peaks"))
bad = 0
for arch, precision, bn, shapes in CASES:
    if bn == "image_f16x2" and not all(hasattr(lib_of(p), "nbc_attach_bn_raw") for p in sys.argv[1:3]):
        print("%s %s bn=%s: skipped, a library lacks nbc_attach_bn_raw" % (arch, precision, bn), flush=True)
        continue
    a, b = model_on(sys.argv[1], arch, precision, bn), model_on(sys.argv[2], arch, precision, bn)
    for idx, h, w in shapes:
        x = torch.from_numpy(np.stack([synth.make_input(i, h, w) for i in idx])).to(dev)
        (la, ya, pa), (lb, yb, pb) = run(a, x), run(b, x)
        same = torch.equal(la, lb) and torch.equal(ya, yb)
        plans = plans_equal(arch, pa, pb)
        bad += not same or plans == "DIFFERENT"
        print("%s %s bn=%s %s x %dx%d: %s (max |logit difference| %.3e), plans %s (%d ops, %d tiles)" %
              (arch, precision, bn, idx, h, w, "identical" if same else "DIFFERENT", float((la - lb).abs().max()),
               plans, len(pa[0]), len(pa[1])), flush=True)
    if (arch, precision, bn) in KEEP_CASES and not KEEP_CALLS_OK:
        print("%s %s bn=%s kept activations and peaks: skipped, a library lacks a keep-mode call" % (arch, precision, bn), flush=True)
    elif (arch, precision, bn) in KEEP_CASES:
        idx, h, w = KEEP_SHAPE
        x = torch.from_numpy(np.stack([synth.make_input(i, h, w) for i in idx])).to(dev)
        what = "kept activations (peaks not compared: they count the pooled vector since aspp_pool)" if arch in EFF_DEEPLAB else "kept activations and peaks"
        bad += compare("%s %s bn=%s %s x %dx%d %s" % (arch, precision, bn, idx, h, w, what), kept(a, arch, x), kept(b, arch, x))
    a._destroy()
    b._destroy()

# ---- the per-image reduction passes ----------------------------------------------------------------------------------
PASS_SHAPES = ((2, 1024, 1024), (1, 520, 1024), (3, 203, 317))      # 203 x 317 is odd: planes off a 16-byte boundary
OFFSETS = (0, 1, 5, 17)                                             # bytes (elements of the labels) off a 16-byte boundary
gen = torch.Generator(device=dev).manual_seed(11)


def off_view(t, off):
    """A contiguous copy of `t` that starts `off` elements behind a 512-byte aligned allocation."""
    buf = torch.empty(t.numel() + off, dtype=t.dtype, device=dev)
    assert buf.data_ptr() % 16 == 0
    v = buf[off:].view(t.shape)
    v.copy_(t)
    return v


def ok(lib, rc, what):
    if rc != _lib.NBC_OK:
        raise RuntimeError("%s: %s" % (what, lib.nbc_last_error().decode()))


def byte_stream_passes(lib, n, h, w, off, rgb, grey, lab8, lab64, stream):
    """outputs of the three byte-stream calls on inputs `off` bytes off; the last confusion has aligned targets and labels 3 off"""
    out = {}
    x, t, l8, l64 = off_view(rgb, off), off_view(grey, off), off_view(lab8, off), off_view(lab64, off)
    for name, labels, dtype, target in (("confusion u8", l8, _lib.LABEL_U8, t), ("confusion i64", l64, _lib.LABEL_I64, t),
                                        ("confusion u8, labels alone off", off_view(lab8, 3), _lib.LABEL_U8, off_view(grey, 0))):
        conf = torch.full((n, 3, 3), -1, dtype=torch.int64, device=dev)
        ok(lib, lib.nbc_confusion(labels.data_ptr(), dtype, target.data_ptr(), n, h, w, conf.data_ptr(), stream), name)
        out[name] = conf
    moments = torch.full((n, 6), -1, dtype=torch.int64, device=dev)
    ok(lib, lib.nbc_image_moments(x.data_ptr(), n, h, w, moments.data_ptr(), stream), "nbc_image_moments")
    counts = torch.full((n, 4), -1, dtype=torch.int64, device=dev)
    ok(lib, lib.nbc_target_counts(t.data_ptr(), n, h, w, counts.data_ptr(), stream), "nbc_target_counts")
    out["image_moments"], out["target_counts"] = moments, counts
    return out


def loss_passes(lib, n, h, w, logits, grey, stream):
    out = {}
    need = lib.nbc_pixel_ce_workspace_bytes(n, h, w)
    ws = torch.empty(need, dtype=torch.uint8, device=dev)
    sums = torch.zeros((n, 3, 3), dtype=torch.float64, device=dev)
    counts = torch.full((n, 3, 3), -1, dtype=torch.int64, device=dev)
    ok(lib, lib.nbc_pixel_cross_entropy(logits.data_ptr(), grey.data_ptr(), n, h, w, ws.data_ptr(), need, sums.data_ptr(),
                                        counts.data_ptr(), stream), "nbc_pixel_cross_entropy")
    out["pixel_ce workspace bytes"], out["pixel_ce sums"], out["pixel_ce counts"] = torch.tensor([need]), sums, counts
    need = lib.nbc_lovasz_workspace_bytes(n, h, w)
    ws = torch.empty(need, dtype=torch.uint8, device=dev)
    terms = torch.zeros((n, 3), dtype=torch.float64, device=dev)
    fg = torch.full((n, 3), -1, dtype=torch.int64, device=dev)
    ok(lib, lib.nbc_lovasz_softmax(logits.data_ptr(), grey.data_ptr(), n, h, w, ws.data_ptr(), need, terms.data_ptr(), fg.data_ptr(),
                                   stream), "nbc_lovasz_softmax")
    out["lovasz workspace bytes"], out["lovasz terms"], out["lovasz fg_counts"] = torch.tensor([need]), terms, fg
    return out


libs = [lib_of(p) for p in sys.argv[1:3]]
stream = torch.cuda.current_stream(dev).cuda_stream
for n, h, w in PASS_SHAPES:
    rgb = torch.randint(0, 256, (n, h, w, 3), dtype=torch.uint8, device=dev, generator=gen)
    grey = torch.randint(0, 256, (n, h, w), dtype=torch.uint8, device=dev, generator=gen)
    lab8 = torch.randint(0, 4, (n, h, w), dtype=torch.uint8, device=dev, generator=gen)      # 3: a label counted nowhere
    lab64 = lab8.to(torch.int64)
    logits = torch.randn((n, 3, h, w), device=dev, generator=gen) * 3
    for off in OFFSETS:
        outs = [byte_stream_passes(lib, n, h, w, off, rgb, grey, lab8, lab64, stream) for lib in libs]
        torch.cuda.synchronize()
        bad += compare("byte streams %dx%dx%d, %d off" % (n, h, w, off), *outs)
    outs = [loss_passes(lib, n, h, w, logits, grey, stream) for lib in libs]
    torch.cuda.synchronize()
    bad += compare("losses %dx%dx%d" % (n, h, w), *outs)

for precision in ("f16x2", "fp32", "bf16"):
    a, b = (model_on(p, "fcn_resnet50", precision, "running") for p in sys.argv[1:3])
    for n, h, w in PASS_SHAPES:
        x = torch.from_numpy(np.stack([synth.make_input(i, h, w) for i in range(n)])).to(dev)
        outs = []
        for m in (a, b):
            m.predict_labels(x, labels_dtype=torch.uint8)
            o = {}
            for zones in (True, False):                  # 5 draws in passes of 2: the last pass is shorter
                counts, lowres = m.dropout_draws(5, [1000 + i for i in range(n)], p=0.1, seed=42, first_draw=3, small_zones=zones,
                                                 return_lowres=True, draws_per_pass=2)
                o["counts, small zones %s" % zones], o["lowres, small zones %s" % zones] = counts, lowres
            outs.append(o)
        torch.cuda.synchronize()
        bad += compare("dropout_draws %s %dx%dx%d" % (precision, n, h, w), *outs)
    a._destroy()
    b._destroy()
sys.exit(1 if bad else 0)
