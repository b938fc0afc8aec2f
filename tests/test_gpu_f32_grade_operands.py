"""The f32-grade kernels ("f16x2", "fp32") per element on the operands they read.  Every conv unit of FCN-ResNet-50 and the whole
DeepLabV3 head, keep mode, planned tiles: a unit's inputs are the tensors its producers stored (the producer map of
tests/helpers/plan_reads.py, as read_activation returns them: pieces joined, activation power taken off), the definition is
evaluated in float64 on them with the weights as the packer holds them, and every stored element must lie within the bound of
tests/helpers/f32_grade_bound.py -- derived from the roundings of the arithmetic, measured from nothing.  Around the conv units:
the max-pool and the concat bit for bit, classifier.4 and the ASPP pooling branch by the counting rule of operand_bound.py with
the precision's store.  One case runs f16x2 on a checkpoint whose activations are all 2^-20 of their usual size, which makes
every reader's 2^-a and every producer's 2^a load-bearing.  The older checks (largest error over the tensor's largest value
against the oracle's chain, 4e-6) cannot see a fault confined to a tail tile, a border column or one K-step; what this bound
cannot see either -- piece-level faults at long K, a truncated low piece -- tests/test_gpu_gather_probe.py compares bit for bit."""
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from neuralbarkcalculator_amd import synth, topology
from neuralbarkcalculator_amd.model import MODELS, conv_tile_info

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import f32_grade_bound as fb  # noqa: E402
import kept_operands as ko  # noqa: E402
import operand_bound as ob  # noqa: E402

pytestmark = pytest.mark.gpu
FCN, DL = "fcn_resnet50", "deeplabv3_resnet50"
PRECISIONS = ("f16x2", "fp32")
# the three bf16 shapes (tests/test_gpu_bf16_operands.py), then 128-pixel-wide maps for the row-step kernel's tiles 18 / 19 / 20:
# 8 x 1024 is a one-row map from layer2 on, 40 x 1024 a five-row one
FCN_SHAPES = [(2, 104, 136), (1, 40, 72), (3, 72, 200), (1, 8, 1024), (2, 40, 1024)]
DL_SHAPES = [(1, 640, 640), (2, 96, 96)]
RESCALED_SHAPE = (2, 104, 136)


def kind_of(u, tile):
    if u.cin == 3:
        return "stem"
    if u.residual:
        return "identity 1x1"
    if u.name.startswith("classifier.0.convs."):
        return "ASPP 1x1" if u.k == 1 else "ASPP 3x3 dilation %d" % u.dil
    if u.name == "classifier.0.project.0":
        return "projection"
    if tile in ko.ROWSTEP_TILES:
        return "row-step 3x3"
    return "%dx%d" % (u.k, u.k)


def pair_of(sd, u):
    return ob.bn_pair(sd[u.bn + ".weight"], sd[u.bn + ".bias"], sd[u.bn + ".running_mean"], sd[u.bn + ".running_var"])


def check_unit(u, sd, precision, acts, reads, a_out, tile, tag, worst):
    """One conv unit on its stored operands: finite, and every element within the bound.  worst: {kind: [c = 2, c = 1]}"""
    x = acts[reads[(u.name, "in")]]
    res = acts[reads[(u.name, "res")]] if u.residual else None
    got = acts[u.name]
    alpha, beta = pair_of(sd, u)
    y_ref, mag, tiny = fb.conv_unit_reference(x, sd[u.name + ".weight"], precision, alpha, beta, res, u.relu, u.stride, u.pad, u.dil)
    assert got.shape == y_ref.shape, (u.name, got.shape, y_ref.shape)
    assert np.isfinite(got).all(), u.name
    err = np.abs(got.astype(np.float64) - y_ref)
    K = u.cin * u.k * u.k
    r2 = err / fb.unit_bound(precision, y_ref, mag, tiny, alpha, beta, res, K, a_out)
    r1 = float((err / fb.unit_bound(precision, y_ref, mag, tiny, alpha, beta, res, K, a_out, c=1)).max())
    at = tuple(int(i) for i in np.unravel_index(int(r2.argmax()), r2.shape))
    print("%s %-34s K %5d tile %2d  worst %.4f of the bound (c = 2), %.4f (c = 1)  at %s" % (tag, u.name, K, tile, float(r2.max()), r1, at), flush=True)
    w = worst.setdefault(kind_of(u, tile), [0.0, 0.0])
    w[0], w[1] = max(w[0], float(r2.max())), max(w[1], r1)
    over = int((r2 > 1.0).sum())
    assert over == 0, "%s %s tile %d: %d of %d elements over the bound, the worst %.3f times at (n, c, y, x) = %s: got %r, float64 %r" % (
        tag, u.name, tile, over, r2.size, float(r2.max()), at, float(got[at]), float(y_ref[at]))


def check_head(sd, x, low, tag, worst):
    """classifier.4: f32 weights on the stored features, f32 out, within (K + 2) u (sum |w x| + |bias|)"""
    y_ref, bound = ob.head_reference(x, sd["classifier.4.weight"], sd["classifier.4.bias"])
    assert low.shape == y_ref.shape and np.isfinite(low).all()
    r = float((np.abs(low.astype(np.float64) - y_ref) / bound).max())
    print("%s %-34s K %5d          worst %.4f of the (K + 2) u bound" % (tag, "classifier.4", x.shape[1], r), flush=True)
    worst["head"] = [max(worst.get("head", [0.0])[0], r)] * 2
    assert r <= 1.0, (tag, r)


def report(tag, worst):
    for kind in sorted(worst):
        print("%s worst per kind: %-24s %.4f (c = 2)  %.4f (c = 1)" % (tag, kind, worst[kind][0], worst[kind][1]), flush=True)


def ingested(x, precision):
    """The stem's operand: the frame as the ingest kernel stores it -- its two f16 pieces (f16x2), or itself"""
    a = x.numpy()
    return fb.join16(*fb.split16(a)) if precision == "f16x2" else a


@pytest.fixture(scope="module", autouse=True)
def reference_threads():
    torch.set_num_threads(min(16, len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else 8))


@pytest.fixture(scope="module")
def dl_sd():
    return synth.make_state_dict("trained_like", seed=7, arch=DL)


@pytest.fixture(scope="module")
def models(sd_np, dl_sd, built_lib):
    made = {}

    def get(arch, precision):
        if (arch, precision) not in made:
            made[(arch, precision)] = MODELS[arch](precision).load_state_dict(sd_np if arch == FCN else dl_sd).to(ko.DEV)
        return made[(arch, precision)]
    yield get
    made.clear()


def run_fcn(m, sd, precision, n, h, w, tag):
    x = ko.frames(range(20, 20 + n), h, w)
    names, reads, shapes, tiles = ko.plan_of(FCN, precision, n, h, w)
    wanted = [k for k in shapes if k != "ingest"]
    units = topology.conv_units(FCN)
    assert set(wanted) == {u.name for u in units if u.bn} | {"backbone.maxpool"} and len(wanted) == 55
    acts, low = ko.stored(m, x, shapes, wanted)
    assert m.pack_flags == 0 and not m.nonfinite_seen()
    worst = {}
    acts["ingest"] = ingested(x, precision)
    for u in units:
        if u.bn is not None:
            check_unit(u, sd, precision, acts, reads, m.activation_exponent(u.name), tiles[u.name], tag, worst)
    pooled = F.max_pool2d(torch.from_numpy(acts["backbone.conv1"]), 3, 2, 1).numpy()
    assert ko.same_bits(acts["backbone.maxpool"], pooled)
    check_head(sd, acts[reads[("classifier.4", "in")]], low, tag, worst)
    report(tag, worst)
    if precision == "f16x2" and w == 1024:
        # the row-step kernel: tiles 19 (64 / 128 output channels) and 20 (256 or more) are planned; 18, the one-row tile of the
        # layers that plan 20, has the same K order: forced, it stores the same bits, so every element above holds for it too
        assert {19, 20} <= set(tiles.values()), sorted(set(tiles.values()))
        # a forced tile that does not fit a layer is ignored there (the planned one runs): the fit rule, on the host, so that
        # the comparison below cannot become vacuous -- tile 18 exists in f16x2, is of tile 20's kind (conv_tile_ok wants the
        # layer's row-step kind) and its columns divide the Cout of every layer that plans 20
        t18, t20 = conv_tile_info("f16x2", 18), conv_tile_info("f16x2", 20)
        on20 = [u for u in units if tiles.get(u.name) == 20]
        assert t18 is not None and t18[2] == t20[2] and t18[2] != conv_tile_info("f16x2", 19)[2] and len(on20) >= 10
        assert all(u.cout % t18[1] == 0 for u in on20), [(u.name, u.cout) for u in on20]
        other, other_low = ko.stored(m, x, shapes, wanted, 18)
        for name in wanted:
            assert ko.same_bits(other[name], acts[name]), (18, name)
        assert ko.same_bits(other_low, low)


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("n,h,w", FCN_SHAPES)
def test_fcn_every_unit_on_the_operands_it_read(models, sd_np, n, h, w, precision):
    run_fcn(models(FCN, precision), sd_np, precision, n, h, w, "fcn %s %dx%dx%d" % (precision, n, h, w))


def test_fcn_f16x2_with_every_activation_power_load_bearing(sd_np, built_lib):
    """Every tensor between a BatchNorm and the next convolution at 2^-20 of its usual size: the packer stores each with a power
    of two, the producing launch applies 2^a and every reading launch 2^-a -- in a per-element check"""
    from conftest import rescale_activations
    sd = rescale_activations(sd_np, 2.0 ** -20, "all")
    m = MODELS[FCN]("f16x2").load_state_dict(sd).to(ko.DEV)
    powers = {u.name: m.activation_exponent(u.name) for u in topology.conv_units(FCN) if u.bn is not None}
    assert any(powers.values()), powers
    print("activation powers: %d of %d units non-zero, from %d to %d" % (sum(1 for v in powers.values() if v), len(powers), min(powers.values()),
                                                                          max(powers.values())), flush=True)
    n, h, w = RESCALED_SHAPE
    run_fcn(m, sd, "f16x2", n, h, w, "fcn f16x2 activations x 2^-20 %dx%dx%d" % (n, h, w))


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("n,h,w", DL_SHAPES)
def test_deeplab_head_on_the_operands_it_read(models, dl_sd, n, h, w, precision):
    m = models(DL, precision)
    x = ko.frames(range(30, 30 + n), h, w)
    names, reads, shapes, tiles = ko.plan_of(DL, precision, n, h, w)
    units = {u.name: u for u in topology.conv_units(DL)}
    trunk = "backbone.layer4.2.conv3"
    branches = ["classifier.0.convs.%d.0" % i for i in range(4)]
    wanted = [trunk] + branches + ["classifier.0.convs.4", "classifier.0.concat", "classifier.0.project.0", "classifier.1"]
    acts, low = ko.stored(m, x, shapes, wanted)
    assert m.pack_flags == 0 and not m.nonfinite_seen()
    hh, ww = shapes[trunk][2:]
    assert (hh, ww) == topology.out_hw(h, w) and ((h, w) != (640, 640) or (hh, ww) == (80, 80))
    tag = "deeplab %s %dx%dx%d" % (precision, n, h, w)
    worst = {}
    for name in branches + ["classifier.0.project.0", "classifier.1"]:
        assert reads[(name, "in")] == (trunk if name in branches else {"classifier.0.project.0": "classifier.0.concat",
                                                                       "classifier.1": "classifier.0.project.0"}[name])
        check_unit(units[name], dl_sd, precision, acts, reads, m.activation_exponent(name), tiles[name], tag, worst)
    # the pooling branch: the mean of the stored trunk, the f32 1x1 conv, the pair, the ReLU, the precision's store
    u = units["classifier.0.convs.4.1"]
    alpha, beta = pair_of(dl_sd, u)
    y_ref, bound = fb.pooled_reference(acts[trunk], dl_sd[u.name + ".weight"], alpha, beta, precision, m.activation_exponent(branches[0]))
    got = acts["classifier.0.convs.4"]
    assert got.shape == y_ref.shape and np.isfinite(got).all()
    r = float((np.abs(got.astype(np.float64) - y_ref) / bound).max())
    print("%s %-34s K %5d          worst %.4f of the bound (%d + %d roundings before the pair)" % (tag, "classifier.0.convs.4", u.cin, r, hh * ww, u.cin),
          flush=True)
    worst["pooled"] = [r, r]
    assert r <= 1.0, (tag, r)
    # the concat: its five stored inputs, the pooled vector broadcast over the image's pixels
    want = np.concatenate([acts[b] for b in branches] + [np.broadcast_to(got, (n, 256, hh, ww))], axis=1)
    assert ko.same_bits(acts["classifier.0.concat"], np.ascontiguousarray(want))
    check_head(dl_sd, acts["classifier.1"], low, tag, worst)
    report(tag, worst)
