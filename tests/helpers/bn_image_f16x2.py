"""Shared pieces of the tests of per-image BatchNorm statistics on the f16x2 pipe (bn_statistics "image_f16x2"): the suite's
constants as tests/test_gpu_bn_stats.py restates them, its float64 adjudication and tie-level label rule, the blob's layout
as the packer writes it, and the two checkpoints whose running statistics misjudge a channel (test infrastructure only)."""
from __future__ import annotations

import numpy as np
import torch

import bn_image_oracle
from neuralbarkcalculator_amd import synth, topology

# the FCN parity suite's fp32 tolerances, relative to the tensor's largest magnitude, and the per-image mode's tie allowance
LOGIT_RTOL_FP32 = 5e-6
LAYER_RTOL_FP32 = 4e-6
MAX_TIE_FLIPS_FRAC = 4e-6
MAX_TIE_FLIPS_FRAC_IMAGE = 2 * MAX_TIE_FLIPS_FRAC

worst = {}          # tag -> (gpu distance, oracle distance), relative: what DESIGN.md 3.6 records


def frames(idx, h, w):
    return torch.from_numpy(np.stack([synth.make_input(int(i), h, w) for i in idx]))


def within(got, want, want64, rtol, tag, group=None):
    """got (GPU) against the f32 oracle at rtol of the tensor's largest magnitude; where that fails, the float64 form
    adjudicates: the GPU must then be within 1.5x of the f32 oracle's own distance to float64 (both printed)."""
    scale = float(want.abs().max())
    err = float((got - want).abs().max())
    print("bn image_f16x2 %s: max err %.3e of scale %.4g = %.3e relative" % (tag, err, scale, err / scale), flush=True)
    if err <= rtol * scale:
        return
    assert want64 is not None, (tag, err, scale)
    w64 = want64()
    e_gpu = float((got.double() - w64).abs().max())
    e_ref = float((want.double() - w64).abs().max())
    print("bn image_f16x2 %s: adjudicated against float64: gpu %.3e, f32 oracle %.3e (scale %.4g) = %.3e, %.3e relative"
          % (tag, e_gpu, e_ref, scale, e_gpu / scale, e_ref / scale), flush=True)
    if group is not None:
        g, o = worst.get(group, (0.0, 0.0))
        worst[group] = (max(g, e_gpu / scale), max(o, e_ref / scale))
    assert e_gpu <= max(rtol * scale, 1.5 * e_ref), (tag, e_gpu, e_ref, scale)


def adjudicated_flips(labels_gpu, logits_ref, err, oracle64, x, tag):
    """The label rule of tests/test_gpu_bn_stats.py: flips against the f32 oracle are allowed at tie level (few, each within
    the logit error of a tie, confirmed by the float64 form), or else the float64 labels decide: the GPU must agree with them
    at least as well as the f32 oracle does.  Where the f32 oracle's own labels are not float64's beyond the allowance the map
    is ill-conditioned in f32: reported, the logits were held to float64 by the caller."""
    top2 = torch.topk(logits_ref, 2, dim=1).values
    margin = top2[:, 0] - top2[:, 1]
    want = torch.argmax(logits_ref, dim=1)
    mism = labels_gpu.cpu() != want
    n = int(mism.sum())
    if n == 0:
        return 0
    l64 = bn_image_oracle.predict_labels(oracle64, x.double())[2]
    t64 = torch.topk(l64, 2, dim=1).values
    allow = max(2, MAX_TIE_FLIPS_FRAC_IMAGE * mism.numel())
    if (n <= allow and float(margin[mism].max()) <= 2.0 * err
            and float((t64[:, 0] - t64[:, 1])[mism].max()) <= 4.0 * err):
        return n
    lab64 = torch.argmax(l64, dim=1)
    g, o = int((labels_gpu.cpu() != lab64).sum()), int((want != lab64).sum())
    print("bn image_f16x2 %s labels: %d flips against the f32 oracle; against float64 the GPU misses %d, the f32 oracle %d of %d"
          % (tag, n, g, o, mism.numel()), flush=True)
    if o > allow:
        print("bn image_f16x2 %s labels: ill-conditioned in f32 (the f32 oracle misses %d float64 labels): reported, not "
              "asserted" % (tag, o), flush=True)
        return n
    assert g <= o + allow, (tag, n, g, o)
    return n


def blob_sections(blob):
    """{unit name: (weights, scale, shift)} views of a packed FCN blob's BatchNorm'd units, and the trailer's exponents."""
    a = lambda v: (v + 255) // 256 * 256
    units = topology.conv_units()
    out, off = {}, 0
    for u in units:
        if u.bn is None:
            break
        ksteps = 7 if u.cin == 3 else u.k * u.k * u.cin * 4 // 128
        wbytes = u.cout * ksteps * 128
        s_off = a(off + wbytes)
        h_off = a(s_off + 4 * u.cout)
        out[u.name] = (blob[off: off + wbytes], blob[s_off: s_off + 4 * u.cout].view(np.float32),
                       blob[h_off: h_off + 4 * u.cout].view(np.float32))
        off = a(h_off + 4 * u.cout)
    exps = blob[-1024:].view(np.int32)[8: 8 + len(units)]
    return out, {u.name: int(exps[i]) for i, u in enumerate(units)}


def raw_sections(raw):
    """{unit name: (first, second)} of a raw-convolution array: 2^(r - k - a_in) and 2^-r per channel."""
    out, off = {}, 0
    for u in topology.conv_units():
        if u.bn is None:
            continue
        out[u.name] = (raw[off: off + u.cout], raw[off + u.cout: off + 2 * u.cout])
        off += 2 * u.cout
    assert off == raw.size
    return out


MISJUDGED_BN = "backbone.layer2.1.bn2"


def misjudged_state_dict(sd, log2_var):
    """The checkpoint with one trunk BatchNorm's running_var multiplied by 2^log2_var and its running_mean set to 0: running
    statistics that never saw the data.  Per-image statistics do not read them, so the network computes what it computed; the
    f16x2 raw convolution in front is stored 2^(log2_var / 2) away from where its pieces hold it."""
    out = dict(sd)
    out[MISJUDGED_BN + ".running_var"] = sd[MISJUDGED_BN + ".running_var"] * np.float32(2.0 ** log2_var)
    out[MISJUDGED_BN + ".running_mean"] = np.zeros_like(sd[MISJUDGED_BN + ".running_mean"])
    return out
