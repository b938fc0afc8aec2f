"""EfficientNet networks on the MI355X (fp32) against the CPU oracle of tests/helpers/efficientnet_oracle.py: every block
output in keep mode, end to end at several sizes, a batch of different images equal to each alone, every variant once,
and predict / evaluate picking a b0 DeepLabV3 checkpoint from its keys.  The suite's fp32 tolerances apply unchanged; a
tensor beyond them is adjudicated against float64: the GPU must lie within 1.5x of the f32 oracle's
own distance from float64."""
import csv
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
from PIL import Image

from neuralbarkcalculator_amd import metrics, synth
from neuralbarkcalculator_amd import evaluate as ev
from neuralbarkcalculator_amd import predict as drv
from neuralbarkcalculator_amd.model import DeepLabV3EfficientNet, FCNEfficientNet
from neuralbarkcalculator_amd.postprocess import remove_small_zones

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import efficientnet_oracle  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LOGIT_RTOL_FP32 = 5e-6
LAYER_RTOL_FP32 = 4e-6

_cache = {}


def _net(n, head):
    """(state_dict, GPU model, f32 oracle, float64 oracle) of one network, built once per session."""
    key = (n, head)
    if key not in _cache:
        torch.set_num_threads(min(16, len(os.sched_getaffinity(0))))
        arch = "%s_efficientnet_b%d" % ("deeplabv3" if head == "deeplab" else "fcn", n)
        sd = synth.make_state_dict("trained_like", seed=7, arch=arch)
        cls = DeepLabV3EfficientNet if head == "deeplab" else FCNEfficientNet
        m = cls(n, "fp32").load_state_dict(sd).to(DEV)
        tsd = {k: torch.from_numpy(v) for k, v in sd.items()}
        _cache[key] = (sd, m, efficientnet_oracle.EfficientNetOracle(tsd, n, head),
                       efficientnet_oracle.EfficientNetOracle(tsd, n, head, torch.float64))
    return _cache[key]


def _inputs(idx, h, w, n=1):
    return torch.from_numpy(np.stack([synth.make_input(idx + i, h, w) for i in range(n)]))


def _check(name, got, ref32, ref64_fn, rtol):
    """got within rtol of the f32 oracle (relative to its largest value), or else within 1.5x of the f32 oracle's own
    distance from float64."""
    got = torch.as_tensor(got, dtype=torch.float64)
    scale = float(ref32.abs().max())
    err = float((got - ref32.double()).abs().max())
    if err <= rtol * scale:
        return err / scale
    ref64 = ref64_fn()
    e_gpu = float((got - ref64).abs().max())
    e_cpu = float((ref32.double() - ref64).abs().max())
    print(f"{name}: over the f32 constant ({err / scale:.2e}); against float64: GPU {e_gpu / scale:.2e}, "
          f"f32 oracle {e_cpu / scale:.2e}")
    assert e_gpu <= 1.5 * e_cpu, (name, e_gpu, e_cpu)
    return err / scale


@pytest.mark.parametrize("n,head", [(0, "fcn"), (0, "deeplab"), (5, "fcn"), (5, "deeplab")])
def test_every_block_output_in_keep_mode(n, head):
    sd, m, o32, o64 = _net(n, head)
    x = _inputs(11, 160, 224)
    keep32, keep64 = {}, {}
    o32.forward(x, keep32)
    m.set_keep_activations(True)
    try:
        m.lowres_logits(x.to(DEV))
        torch.cuda.synchronize()
        def ref64(name):
            if not keep64:
                o64.forward(x, keep64)
            return keep64[name]

        worst = 0.0
        for name, ref in keep32.items():
            got = m.read_activation(name, ref.numel())
            assert got.shape == tuple(ref.shape), name
            worst = max(worst, _check(name, got, ref, lambda: ref64(name), LAYER_RTOL_FP32))
        gate = m.read_activation("backbone.model._blocks.1._se_expand", 10 ** 5)
        assert gate.shape[2:] == (1, 1) and 0.0 < gate.min() and gate.max() < 1.0
        print(f"b{n} {head}: {len(keep32)} tensors, worst {worst:.2e} of the tensor's range")
    finally:
        m.set_keep_activations(False)


def _e2e(n, head, h, w, idx=3, batch=1):
    sd, m, o32, o64 = _net(n, head)
    x = _inputs(idx, h, w, batch)
    low32, full32 = o32.forward(x)
    xd = x.to(DEV)
    labels, counts, low = m.predict_labels(xd, return_lowres=True)
    full = m(xd)
    torch.cuda.synchronize()
    assert tuple(low.shape) == tuple(low32.shape)
    e1 = _check("lowres", low.cpu(), low32, lambda: o64.forward(x)[0], LOGIT_RTOL_FP32)
    e2 = _check("full", full.cpu(), full32, lambda: o64.forward(x)[1], LOGIT_RTOL_FP32)
    ref_labels = full32.argmax(1)
    diff = labels.cpu() != ref_labels
    if diff.any():                                       # a flip only where the oracle's top two logits nearly tie
        top2 = full32.topk(2, dim=1).values
        gap = (top2[:, 0] - top2[:, 1])[diff]
        assert float(gap.max()) <= 10 * LOGIT_RTOL_FP32 * float(full32.abs().max()), float(gap.max())
    assert torch.equal(counts.cpu(), torch.stack([(labels.cpu() == c).sum((1, 2)) for c in range(3)], 1))
    print(f"b{n} {head} {batch}x{h}x{w}: lowres {e1:.2e}, full {e2:.2e}, {int(diff.sum())} labels flipped")


@pytest.mark.parametrize("n,head", [(0, "fcn"), (0, "deeplab"), (5, "fcn"), (5, "deeplab")])
@pytest.mark.parametrize("h,w", [(1024, 1024), (600, 1024), (203, 317)])
def test_end_to_end_against_oracle(n, head, h, w):
    _e2e(n, head, h, w)


@pytest.mark.parametrize("n,head", [(0, "fcn"), (0, "deeplab"), (5, "fcn"), (5, "deeplab")])
def test_batch_of_two_different_images_equals_each_alone(n, head):
    _, m, _, _ = _net(n, head)
    x = _inputs(21, 96, 96, 2).to(DEV)
    both = m.lowres_logits(x)
    one = torch.cat([m.lowres_logits(x[i:i + 1].contiguous()) for i in range(2)])
    torch.cuda.synchronize()
    assert not torch.equal(both[0], both[1])
    assert torch.equal(both, one)
    _e2e(n, head, 96, 96, idx=21, batch=2)


@pytest.mark.parametrize("n", [1, 2, 3, 4, 6, 7])
@pytest.mark.parametrize("head", ["fcn", "deeplab"])
def test_every_variant_end_to_end(n, head):
    _e2e(n, head, 128, 192)
    _cache.pop((n, head), None)


def test_op_records_name_the_modules():
    _, m, _, _ = _net(0, "fcn")
    x = _inputs(5, 128, 128).to(DEV)
    m.set_profiling(True)
    m.lowres_logits(x)
    m.set_profiling(False)
    recs = {r["name"]: r for r in m.op_records()}
    assert recs["backbone.model._blocks.1._depthwise_conv"]["kernel"] == "dwconv"
    assert recs["backbone.model._blocks.1._se_expand"]["kernel"] == "se_excite"
    assert recs["backbone.model._blocks.1._project_conv.gated_weights"]["kernel"] == "gate_weights"
    assert recs["backbone.model._blocks.1._project_conv"]["kernel"] == "conv_dma"
    assert recs["backbone.model._conv_head.swish"]["kernel"] == "swish"
    assert recs["classifier.4"]["kernel"] == "head1x1"


LAYOUT = [("epinette_gelee", "a01.png", 40, 256, 256), ("sapin", "s1.bmp", 41, 200, 256),
          ("epinette_non_gelee", "n1.png", 42, 136, 256)]


def test_predict_and_evaluate_pick_a_b0_deeplab_checkpoint(tmp_path):
    sd, _, o32, _ = _net(0, "deeplab")
    root = str(tmp_path / "fold")
    frames_ = {}
    for wood, name, idx, h, w in LAYOUT:
        for sub in ("samples", "duals"):
            os.makedirs(os.path.join(root, sub, wood), exist_ok=True)
        img = synth.make_frame(idx, h, w)
        Image.fromarray(img, mode="RGB").save(os.path.join(root, "samples", wood, name))
        png = name.replace("bmp", "png")
        lab = o32.forward(torch.from_numpy(synth.normalize_frame(img))[None])[1].argmax(1)[0].numpy().astype(np.uint8)
        grey = np.array([0, 127, 255], np.uint8)[(lab + (np.arange(lab.size).reshape(lab.shape) % 7 == 0)) % 3]
        Image.fromarray(grey, mode="L").save(os.path.join(root, "duals", wood, png))
        frames_[(wood, png)] = (img, lab, grey)
    ckpt = os.path.join(root, "best_model.pt")
    torch.save({k: torch.from_numpy(v) for k, v in sd.items()}, ckpt)

    p = subprocess.run([sys.executable, "-m", "neuralbarkcalculator_amd.predict", root, "--model_path", ckpt, "--streams", "2"],
                       cwd=REPO, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-3000:]
    rows = list(csv.reader(open(os.path.join(root, "results", "final_stats.csv")), delimiter="\t"))
    assert rows[0] == drv.CSV_HEADER and len(rows) == 1 + len(LAYOUT)
    flips = 0
    for row in rows[1:]:
        name, wood = row[0], row[1]
        lab = remove_small_zones(frames_[(wood, name)][1].copy())
        got = np.asarray(Image.open(os.path.join(root, "results", "outputs", wood, name)))
        f = int((got != drv.label_png(lab)).sum())
        flips += f
        if f == 0:
            assert row == drv.stats_row(name, wood, lab.shape[0], lab.shape[1], int((lab == 1).sum()), int((lab == 2).sum()))
    assert flips <= 4, flips

    st = ev.evaluate_folder(root, ckpt, precision="f16x2", device_index=0, precision_auto=True)
    assert st["images_total"] == len(LAYOUT)
    erows = list(csv.reader(open(os.path.join(root, ev.STATS_CSV)), delimiter="\t"))
    assert erows[0] == metrics.EVAL_CSV_HEADER and len(erows) == 1 + len(LAYOUT)
    exact = 0
    for r in erows[1:]:
        img, lab, grey = frames_[(r[1], r[0])]
        t = metrics.target_classes(grey)
        want = metrics.eval_row(r[0], r[1], metrics.confusion_numpy(lab, t), metrics.confusion_numpy(remove_small_zones(lab), t))
        exact += r == want
    assert exact >= len(LAYOUT) - 1, exact
    summary = json.load(open(os.path.join(root, ev.SUMMARY_JSON)))
    assert summary["images_evaluated"] == len(LAYOUT) and summary["precision"] == "fp32"
    with pytest.raises(ValueError, match="fp32"):
        ev.evaluate_folder(root, ckpt, precision="bf16", device_index=0)
