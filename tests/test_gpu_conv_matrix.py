"""Every generic tile of the convolution menu on every form of layer of the three networks (tests/helpers/conv_matrix.py
has the cases and the forms; tests/test_conv_matrix_ledger.py the cover they give).

include/nbc.h: results do not depend on the tile, because every tile walks K in the same order with one accumulator per
output.  So one oracle comparison per case anchors the planned tiles, under the suite's tolerances, and every other tile must
then store the same BITS, layer by layer: a tile installed strictly (nbc_set_plan_tiles refuses what does not fit, and
nbc_get_plan_tiles reads back what ran), every tensor of the keep-mode forward compared as uint32 words.  A failure names
the tile, the first layer that differs, its form and the first differing (n, c, y, x).  The lenient knob every other tile
test uses (nbc_set_conv_tile) is tied to the strict one: same logits bits, and the fused (downsample.0, conv3) launches the
plan and the menu say.  The last test checks that what ran here is what the ledger test computes."""
import os
import sys
import time
import types

import numpy as np
import pytest
import torch

from neuralbarkcalculator_amd import synth, topology
from neuralbarkcalculator_amd.model import MODELS

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import conv_matrix as cm  # noqa: E402
import deeplab_oracle  # noqa: E402
import efficientnet_oracle  # noqa: E402
from test_gpu_efficientnet import _check  # noqa: E402
from test_gpu_parity import LAYER_RTOL_BF16, LAYER_RTOL_FP32, LOGIT_RTOL_BF16, LOGIT_RTOL_FP32  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
RTOL = {"fp32": (LAYER_RTOL_FP32, LOGIT_RTOL_FP32), "f16x2": (LAYER_RTOL_FP32, LOGIT_RTOL_FP32),
        "bf16": (LAYER_RTOL_BF16, LOGIT_RTOL_BF16)}
LOGITS = "classifier.4"

_NETS, _MODELS, _REFS = {}, {}, {}
_LEDGER = {}                             # (precision, tile, form) -> layers, of the cases that passed
_RAN = []


def _net(arch):
    """(state_dict, the oracles of the network), built once."""
    if arch not in _NETS:
        torch.set_num_threads(min(16, len(os.sched_getaffinity(0))))
        sd = synth.make_state_dict("trained_like", seed=7, arch=arch)
        tsd = {k: torch.from_numpy(v) for k, v in sd.items()}
        if topology.is_efficientnet(arch):
            n, head = topology.efficientnet_variant(arch), "deeplab" if arch.startswith("deeplabv3") else "fcn"
            oracles = (efficientnet_oracle.EfficientNetOracle(tsd, n, head),
                       efficientnet_oracle.EfficientNetOracle(tsd, n, head, torch.float64))
        elif arch == "deeplabv3_resnet50":
            oracles = (deeplab_oracle.load(sd),)
        else:
            from oracle.fcn_resnet50_oracle import OracleFCNResNet50
            oracles = (OracleFCNResNet50(),)
            oracles[0].load_state_dict(tsd)
        _NETS[arch] = (sd, oracles)
    return _NETS[arch]


def _model(arch, precision):
    if (arch, precision) not in _MODELS:
        _MODELS[(arch, precision)] = MODELS[arch](precision).load_state_dict(_net(arch)[0]).to(DEV)
    return _MODELS[(arch, precision)]


def _reference(arch, shape):
    """(x, {op name: oracle tensor}, float64 lookup or None) of one (network, shape): computed once, shared by the precisions
    and never written to."""
    if (arch, shape) not in _REFS:
        from oracle.fcn_resnet50_oracle import layer_outputs
        n, h, w = shape
        x = torch.from_numpy(np.stack([synth.make_input(31 + i, h, w) for i in range(n)]))
        oracles = _net(arch)[1]
        ref64 = None
        if topology.is_efficientnet(arch):
            ref, keep64 = {}, {}
            ref[LOGITS] = oracles[0].forward(x, ref)[0]

            def ref64(name):
                if not keep64:
                    keep64[LOGITS] = oracles[1].forward(x, keep64)[0]
                return keep64[name]
        elif arch == "deeplabv3_resnet50":
            # the trunk's conv units by the FCN oracle's walk (its head slots filled with identities), then the head's tensors
            trunk = types.SimpleNamespace(backbone=oracles[0].backbone, classifier=[torch.nn.Identity()] * 5)
            ref = layer_outputs(trunk, x)
            del ref["classifier.0"], ref[LOGITS]
            head = deeplab_oracle.head_outputs(oracles[0], x)
            del head["layer4"]
            ref.update(head)
        else:
            ref = layer_outputs(oracles[0], x)
        _REFS[(arch, shape)] = (x, ref, ref64)
    return _REFS[(arch, shape)]


def _kept(m, lowres, ops):
    """Host copies of every tensor the keep-mode forward left, and the low-resolution logits."""
    out = {name: m.read_activation(name, numel).copy() for name, numel in ops}
    out[LOGITS] = lowres.cpu().numpy()
    return out


def _check_baseline(arch, precision, kept, ref, ref64):
    rl, rlog = RTOL[precision]
    worst = ("", 0.0)
    for name, want in ref.items():
        got = kept[name]
        assert got.shape == tuple(want.shape), (name, got.shape, tuple(want.shape))
        rtol = rlog if name == LOGITS else rl
        if ref64 is not None:
            rel = _check(name, got, want, lambda: ref64(name), rtol)
        else:
            scale = float(want.abs().max())
            err = float(np.abs(got - want.numpy()).max())
            rel = err / scale
            assert err <= rtol * scale, f"{name}: max err {err} vs scale {scale} ({arch}, {precision}, planned tiles)"
        worst = max(worst, (name, rel), key=lambda t: t[1])
    return worst


@pytest.mark.parametrize("case", cm.flat_cases(), ids=cm.case_id)
def test_every_tile_stores_the_planned_tiles_bits(built_lib, case):
    arch, precision, (n, h, w) = case
    t0 = time.perf_counter()
    x, ref, ref64 = _reference(arch, (n, h, w))
    t_ref = time.perf_counter() - t0
    m = _model(arch, precision)
    xd = x.to(DEV)
    form = cm.forms(arch)
    ops = cm.readable_ops(arch, precision, n, h, w)
    kinds = {o["name"]: o["kernel"] for o in cm.plan(arch, precision, n, h, w, True)[0]}
    planned = [o["tile"] for o in cm.conv_launches(arch, precision, n, h, w)]
    problems, ran = [], {}
    default = None
    try:
        # 1. planned tiles in keep mode against the oracle; every tensor kept on the host
        m.set_conv_tile(-1)
        m.set_keep_activations(True)
        m.reserve(n, h, w)
        default = m.plan_tiles()
        assert default == planned, "the plan text and nbc_get_plan_tiles disagree"
        base = _kept(m, m.lowres_logits(xd), ops)
        assert m.plan_tiles() == default
        assert set(ref) <= set(base), sorted(set(ref) - set(base))
        worst = _check_baseline(arch, precision, base, ref, ref64)

        # 2. every generic tile of the precision, installed strictly
        for tile in cm.tiles_of(precision):
            tiles, took = cm.install_list(arch, precision, n, h, w, tile)
            assert took, (tile, "lands on no layer")
            m.set_plan_tiles(tiles)                      # RuntimeError: the helper's rule and conv_tile_ok disagree
            got = _kept(m, m.lowres_logits(xd), ops)
            assert m.plan_tiles() == tiles, (tile, "the forward did not keep the installed tiles")
            differing = [(name, cm.first_difference(got[name], base[name])) for name in base]
            differing = [(name, d) for name, d in differing if d is not None]
            if differing:
                name, (where, count) = differing[0]
                on = "on tile %d" % tile if name in took else "on its planned tile" if name in form else "no convolution"
                problems.append("tile %d: %s (%s, %s) differs first at (n, c, y, x) = %s, %d words; %d of %d tensors differ"
                                % (tile, name, form.get(name, kinds.get(name, "logits")), on, where, count, len(differing), len(base)))
            ran[tile] = took
        m.set_plan_tiles(default)

        # 3. the lenient knob on the keep-off plan: same logits, and the fused pairs the plan and the menu say
        m.set_keep_activations(False)
        low = m.lowres_logits(xd)
        assert m.fused_pairs() == cm.expected_fused_pairs(arch, precision, n, h, w, -1)
        low = low.cpu().numpy()
        for tile in cm.tiles_of(precision):
            m.set_conv_tile(tile)
            got = m.lowres_logits(xd)
            pairs = m.fused_pairs()
            d = cm.first_difference(got.cpu().numpy(), low)
            if d is not None:
                problems.append("nbc_set_conv_tile(%d), keep off: the logits differ first at (n, c, y, x) = %s, %d words" % ((tile,) + d))
            want_pairs = cm.expected_fused_pairs(arch, precision, n, h, w, tile)
            if pairs != want_pairs:
                problems.append("nbc_set_conv_tile(%d), keep off: %d fused pairs, the plan and the menu say %d" % (tile, pairs, want_pairs))
        if precision == "f16x2":
            dual = [t for t in cm.tiles_of(precision) if cm.model.conv_tile_info(precision, t)[3]]
            pair_ops = [o for o in cm.conv_launches(arch, precision, n, h, w, keep=False) if "ds" in o]
            assert dual and pair_ops and all(o["unit"].residual for o in pair_ops)
            for t in dual:
                if all(cm.library_fits(precision, t, o["co"], 0) for o in pair_ops):
                    assert cm.expected_fused_pairs(arch, precision, n, h, w, t) == len(pair_ops)
    finally:
        # 4. tile state back to the planner's
        m.set_conv_tile(-1)
        if default is not None:
            m.set_keep_activations(True)
            m.reserve(n, h, w)
            m.set_plan_tiles(default)
        m.set_keep_activations(False)
    print("%s: %d tensors, worst %s against the oracle; %d tiles; oracle %.1f s, case %.1f s"
          % (cm.case_id(case), len(base), "%s %.2e" % worst, len(ran), t_ref, time.perf_counter() - t0))
    assert not problems, "%s:\n" % cm.case_id(case) + "\n".join(problems)
    for tile, took in ran.items():
        for name in took:
            key = (precision, tile, form[name])
            _LEDGER[key] = _LEDGER.get(key, 0) + 1
    _RAN.append(case)


@pytest.mark.parametrize("arch", [a for a, _, _ in cm.CASES if topology.is_efficientnet(a)])
def test_autotune_on_efficientnet_keeps_the_bits(built_lib, arch):
    """nbc_autotune on an EfficientNet context times every fitting tile on every layer, the per-image launches of the gated
    project convolutions included, and only picks tiles: each fits its layer, and the logits keep their bits."""
    precision = "fp32"
    n, h, w = next(shapes for a, _, shapes in cm.CASES if a == arch)[1]
    m = _model(arch, precision)
    xd = _reference(arch, (n, h, w))[0].to(DEV)
    launches = cm.conv_launches(arch, precision, n, h, w, keep=False)
    m.set_conv_tile(-1)
    m.set_keep_activations(False)
    m.reserve(n, h, w)
    default = m.plan_tiles()
    assert default == [o["tile"] for o in launches]
    try:
        base = m.lowres_logits(xd).cpu().numpy()
        assert np.isfinite(base).all()
        tiles = m.autotune(xd, reps=1)
        assert len(tiles) == len(launches)
        for t, o in zip(tiles, launches):
            assert cm.library_fits(precision, t, o["co"], cm.planned_kind(precision, o)), (o["name"], t)
        assert cm.first_difference(m.lowres_logits(xd).cpu().numpy(), base) is None, tiles
        assert m.plan_tiles() == tiles
        m.autotune(xd, reps=1)
        m.set_plan_tiles(default)
        assert m.plan_tiles() == default
        assert cm.first_difference(m.lowres_logits(xd).cpu().numpy(), base) is None
        assert m.plan_tiles() == default
    finally:
        m.set_plan_tiles(default)


def test_the_ledger_that_ran_is_the_ledger_computed():
    """Non-vacuity: every case of the matrix ran and passed here, so every generic (precision, tile) of the menu landed on
    the layers the host arithmetic says.  A deselected or failed case makes this fail: it does not skip."""
    missing = [cm.case_id(c) for c in cm.flat_cases() if c not in _RAN]
    assert not missing, "cases that did not run and pass in this session: %s" % missing
    assert _LEDGER == cm.ledger(cm.flat_cases())
    counted = {p: len({k[1] for k in _LEDGER if k[0] == p}) for p in cm.PRECISIONS}
    assert counted == {p: len(cm.tiles_of(p)) for p in cm.PRECISIONS}
    print("generic (precision, tile) pairs that ran:", counted)
