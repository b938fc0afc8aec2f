"""The bf16 kernels per element on the operands they read.  Every conv unit of FCN-ResNet-50 and the whole DeepLabV3 head in
bf16, keep mode: a unit's inputs are the tensors its producers stored (the producer map of tests/helpers/plan_reads.py), the
definition is evaluated in float64 on them, and every stored element must lie within the bound of
tests/helpers/operand_bound.py -- derived from the roundings of the arithmetic (the f32 accumulation, the f32 epilogue, one
bf16 rounding at the store), not measured.  Around the conv units: the max-pool and the concat bit for bit, classifier.4 and
the ASPP pooling branch by the same counting rule, and the 256x256 tiles that only bf16 has (3 and 12) bit for bit against the
planned ones.  tests/test_operand_bound.py shows on the CPU that the bound rejects a truncating store, a K-step left out, a
neighbour's alpha and a lost border tap; the 4e-2 max-norm checks of the other bf16 tests see none of the first and little of
the rest."""
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from neuralbarkcalculator_amd import synth, topology
from neuralbarkcalculator_amd.model import FCNResNet50, deeplabv3_resnet50

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import kept_operands as ko  # noqa: E402
import operand_bound as ob  # noqa: E402
from kept_operands import frames, same_bits, stored  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FCN, DL = "fcn_resnet50", "deeplabv3_resnet50"
# (N, H, W).  104 x 136: 442 and 1768 output pixels, partial 128- and 256-row tiles with an image boundary inside a tile;
# 40 x 72: 45 pixels, fewer than any tile; 72 x 200: 675 pixels, three 256-row tiles, the last one partial
FCN_SHAPES = [(2, 104, 136), (1, 40, 72), (3, 72, 200)]
# the planned tiles, and the two 256 x 256 tiles no other precision has (a layer whose Cout they do not divide keeps its own)
TILES = (-1, 3, 12)
# 640 x 640 is an 80 x 80 map: pixels 36..43 in each direction have all nine taps of dilation 36 inside the image;
# 96 x 96 is 12 x 12: every dilated tap but the centre reads padding
DL_SHAPES = [(1, 640, 640), (2, 96, 96)]


def plan_of(arch, n, h, w):
    """(op names, producer map, {op: shape of the tensor it stores}) of the bf16 keep-mode plan"""
    return ko.plan_of(arch, "bf16", n, h, w)[:3]


def pair_of(sd, u):
    return ob.bn_pair(sd[u.bn + ".weight"], sd[u.bn + ".bias"], sd[u.bn + ".running_mean"], sd[u.bn + ".running_var"])


def kind_of(u):
    if u.cin == 3:
        return "stem"
    if u.residual:
        return "identity 1x1"
    if u.name.startswith("classifier.0.convs."):
        return "ASPP 1x1" if u.k == 1 else "ASPP 3x3 dilation %d" % u.dil
    return "%dx%d" % (u.k, u.k)


def check_unit(u, sd, acts, reads, tag, worst):
    """One conv unit on its stored operands: finite, and every element within the bound.  worst: {kind: [c = 2, c = 1]}"""
    x = acts[reads[(u.name, "in")]]
    res = acts[reads[(u.name, "res")]] if u.residual else None
    got = acts[u.name]
    alpha, beta = pair_of(sd, u)
    y_ref, mag = ob.conv_unit_reference(x, sd[u.name + ".weight"], alpha, beta, res, u.relu, u.stride, u.pad, u.dil)
    assert got.shape == y_ref.shape, (u.name, got.shape, y_ref.shape)
    assert np.isfinite(got).all(), u.name
    err = np.abs(got.astype(np.float64) - y_ref)
    K = u.cin * u.k * u.k
    r2 = err / ob.bf16_unit_bound(y_ref, mag, alpha, beta, res, K)
    r1 = float((err / ob.bf16_unit_bound(y_ref, mag, alpha, beta, res, K, c=1)).max())
    at = tuple(int(i) for i in np.unravel_index(int(r2.argmax()), r2.shape))
    print("%s %-34s K %5d  worst %.3f of the bound (c = 2), %.3f (c = 1)  at %s" % (tag, u.name, K, float(r2.max()), r1, at), flush=True)
    w = worst.setdefault(kind_of(u), [0.0, 0.0])
    w[0], w[1] = max(w[0], float(r2.max())), max(w[1], r1)
    over = int((r2 > 1.0).sum())
    assert over == 0, "%s %s: %d of %d elements over the bound, the worst %.3f times at (n, c, y, x) = %s: got %r, float64 %r" % (
        tag, u.name, over, r2.size, float(r2.max()), at, float(got[at]), float(y_ref[at]))


def check_head(sd, x, low, tag, worst):
    """classifier.4: f32 weights on the stored bf16 features, f32 out, within (K + 2) u (sum |w x| + |bias|)"""
    y_ref, bound = ob.head_reference(x, sd["classifier.4.weight"], sd["classifier.4.bias"])
    assert low.shape == y_ref.shape and np.isfinite(low).all()
    r = float((np.abs(low.astype(np.float64) - y_ref) / bound).max())
    print("%s %-34s K %5d  worst %.3f of the (K + 2) u bound" % (tag, "classifier.4", x.shape[1], r), flush=True)
    worst.setdefault("classifier.4", [0.0, 0.0])
    worst["classifier.4"] = [max(worst["classifier.4"][0], r)] * 2
    assert r <= 1.0, (tag, r)


def report(tag, worst):
    for kind in sorted(worst):
        print("%s worst per kind: %-24s %.3f (c = 2)  %.3f (c = 1)" % (tag, kind, worst[kind][0], worst[kind][1]), flush=True)


@pytest.fixture(scope="module", autouse=True)
def reference_threads():
    torch.set_num_threads(min(16, len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else 8))


@pytest.fixture(scope="module")
def fcn(sd_np, built_lib):
    return FCNResNet50("bf16").load_state_dict(sd_np).to(DEV)


@pytest.fixture(scope="module")
def dl_sd():
    return synth.make_state_dict("trained_like", seed=7, arch=DL)


@pytest.fixture(scope="module")
def dl(dl_sd, built_lib):
    return deeplabv3_resnet50(precision="bf16").load_state_dict(dl_sd).to(DEV)


@pytest.mark.parametrize("n,h,w", FCN_SHAPES)
def test_fcn_every_unit_on_the_operands_it_read(fcn, sd_np, n, h, w):
    x = frames(range(20, 20 + n), h, w)
    names, reads, shapes = plan_of(FCN, n, h, w)
    wanted = [k for k in shapes if k != "ingest"]
    units = topology.conv_units(FCN)
    assert set(wanted) == {u.name for u in units if u.bn} | {"backbone.maxpool"} and len(wanted) == 55
    acts, low = stored(fcn, x, shapes, wanted)
    for tile in TILES[1:]:
        other, other_low = stored(fcn, x, shapes, wanted, tile)
        for name in wanted:
            assert same_bits(other[name], acts[name]), (tile, name)
        assert same_bits(other_low, low), tile
        del other
    tag = "fcn bf16 %dx%dx%d" % (n, h, w)
    worst = {}
    # the stem's operand: the frame cast to bf16, which is the ingest kernel's definition of the stored pixel
    acts["ingest"] = x.to(torch.bfloat16).to(torch.float32).numpy()
    for u in units:
        if u.bn is not None:
            check_unit(u, sd_np, acts, reads, tag, worst)
    pooled = F.max_pool2d(torch.from_numpy(acts["backbone.conv1"]), 3, 2, 1).numpy()
    assert same_bits(acts["backbone.maxpool"], pooled)
    check_head(sd_np, acts[reads[("classifier.4", "in")]], low, tag, worst)
    report(tag, worst)


@pytest.mark.parametrize("n,h,w", DL_SHAPES)
def test_deeplab_head_on_the_operands_it_read(dl, dl_sd, n, h, w):
    x = frames(range(30, 30 + n), h, w)
    names, reads, shapes = plan_of(DL, n, h, w)
    units = {u.name: u for u in topology.conv_units(DL)}
    trunk = "backbone.layer4.2.conv3"
    branches = ["classifier.0.convs.%d.0" % i for i in range(4)]
    wanted = [trunk] + branches + ["classifier.0.convs.4", "classifier.0.concat", "classifier.0.project.0", "classifier.1"]
    acts, low = stored(dl, x, shapes, wanted)
    hh, ww = shapes[trunk][2:]
    assert (hh, ww) == topology.out_hw(h, w) and ((h, w) != (640, 640) or (hh, ww) == (80, 80))
    tag = "deeplab bf16 %dx%dx%d" % (n, h, w)
    worst = {}
    for name in branches + ["classifier.0.project.0", "classifier.1"]:
        assert reads[(name, "in")] == (trunk if name in branches else {"classifier.0.project.0": "classifier.0.concat",
                                                                       "classifier.1": "classifier.0.project.0"}[name])
        check_unit(units[name], dl_sd, acts, reads, tag, worst)
    # the pooling branch: the mean of the stored trunk, the f32 1x1 conv, the pair, the ReLU, the bf16 store
    u = units["classifier.0.convs.4.1"]
    alpha, beta = pair_of(dl_sd, u)
    y_ref, bound = ob.pooled_reference(acts[trunk], dl_sd[u.name + ".weight"], alpha, beta)
    got = acts["classifier.0.convs.4"]
    assert got.shape == y_ref.shape and np.isfinite(got).all()
    r = float((np.abs(got.astype(np.float64) - y_ref) / bound).max())
    print("%s %-34s K %5d  worst %.3f of the bound (%d + %d roundings before the pair)" % (tag, "classifier.0.convs.4", u.cin, r, hh * ww, u.cin),
          flush=True)
    worst["ASPP pooled"] = [r, r]
    assert r <= 1.0, (tag, r)
    # the concat: its five stored inputs, the pooled vector broadcast over the image's pixels
    want = np.concatenate([acts[b] for b in branches] + [np.broadcast_to(got, (n, 256, hh, ww))], axis=1)
    assert same_bits(acts["classifier.0.concat"], np.ascontiguousarray(want))
    check_head(dl_sd, acts["classifier.1"], low, tag, worst)
    report(tag, worst)
