"""deeplabv3_resnet50 on the GPU against the CPU oracle of tests/helpers/deeplab_oracle.py: every head tensor in keep mode
(the four ASPP convolutions, the pooled vector, the concat, the projection, classifier.1), end to end at 1024^2, a
trimmed-scan height, an odd shape and the small maps where the dilated taps are mostly or entirely padding, batches of
different images, the op records, and the folder drivers under --arch auto."""
import csv
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
from PIL import Image

from neuralbarkcalculator_amd import _lib, metrics, synth, topology
from neuralbarkcalculator_amd import evaluate as ev
from neuralbarkcalculator_amd import predict as drv
from neuralbarkcalculator_amd.model import DeepLabV3ResNet50, FCNResNet50, deeplabv3_resnet50, pack_state_dict
from neuralbarkcalculator_amd.postprocess import remove_small_zones

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import deeplab_oracle  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
DL = "deeplabv3_resnet50"
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# the FCN parity suite's tolerances (tests/test_gpu_parity.py), restated here: relative to the tensor's largest magnitude
LOGIT_RTOL_FP32 = 5e-6      # both f32-grade modes, fp32 and f16x2
LAYER_RTOL_FP32 = 4e-6
LOGIT_RTOL_BF16 = 4e-2
LAYER_RTOL_BF16 = 4e-2
MAX_TIE_FLIPS_FRAC = 4e-6
RTOL = {"fp32": (LAYER_RTOL_FP32, LOGIT_RTOL_FP32), "f16x2": (LAYER_RTOL_FP32, LOGIT_RTOL_FP32),
        "bf16": (LAYER_RTOL_BF16, LOGIT_RTOL_BF16)}
MODES = ("fp32", "f16x2", "bf16")


@pytest.fixture(scope="module")
def dl_sd():
    return synth.make_state_dict("trained_like", seed=7, arch=DL)


@pytest.fixture(scope="module")
def oracle(dl_sd):
    torch.set_num_threads(max(1, min(32, os.cpu_count() or 1)))
    return deeplab_oracle.load(dl_sd)


@pytest.fixture(scope="module")
def models(dl_sd, built_lib):
    return {m: deeplabv3_resnet50(precision=m).load_state_dict(dl_sd).to(DEV) for m in MODES}


def frames(idx, h, w):
    return torch.from_numpy(np.stack([synth.make_input(int(i), h, w) for i in idx]))


def adjudicated_flips(labels_gpu, logits_ref, err, oracle, x):
    """Label flips against the oracle are allowed only where the oracle's top-two margin is within twice the measured logit
    error (an exact-tie-level difference), and then the float64 evaluation must say the margin is that small too."""
    top2 = torch.topk(logits_ref, 2, dim=1).values
    margin = top2[:, 0] - top2[:, 1]
    want = torch.argmax(logits_ref, dim=1)
    mism = labels_gpu.cpu() != want
    n = int(mism.sum())
    if n:
        assert float(margin[mism].max()) <= 2.0 * err, (n, float(margin[mism].max()), err)
        assert n <= max(2, MAX_TIE_FLIPS_FRAC * mism.numel()), n
        o64 = oracle.double()
        try:
            with torch.no_grad():
                l64 = torch.nn.functional.interpolate(o64.lowres_logits(x.double()), size=x.shape[-2:], mode="bicubic",
                                                      align_corners=False)
        finally:
            oracle.float()
        t64 = torch.topk(l64, 2, dim=1).values
        assert float((t64[:, 0] - t64[:, 1])[mism].max()) <= 2.0 * err
    return n


_HEAD_REF = {}


def _head_reference(oracle, size):
    """The frame and the oracle's head tensors at `size`: computed once, shared by the three modes."""
    if size not in _HEAD_REF:
        x = frames([5], *size)
        _HEAD_REF[size] = (x, deeplab_oracle.head_outputs(oracle, x))
    return _HEAD_REF[size]


@pytest.mark.parametrize("size", [(256, 256), (640, 640)], ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("mode", MODES)
def test_head_layer_by_layer_against_oracle(oracle, models, mode, size):
    """Keep mode: every head tensor, including the pooled vector and the concat, and the logits.  At 256 x 256 (a 32 x 32
    map) a tap of dilation 24 lands inside the image for only 8 of a row's 32 pixels on either side and a tap of dilation 36
    for none: those two branches are their centre tap plus, at dilation 24, a fringe.  At 640 x 640 (an 80 x 80 map) pixels
    36..43 in each direction have all nine taps of every dilation inside the image, and every other pixel a proper subset."""
    m = models[mode]
    rl, rlog = RTOL[mode]
    x, ref = _head_reference(oracle, size)
    m.set_keep_activations(True)
    try:
        lowres = m.lowres_logits(x.to(DEV))
        torch.cuda.synchronize()
        report = {}
        for name, want in ref.items():
            if name == "layer4":
                name_gpu = "backbone.layer4.2.conv3"
            else:
                name_gpu = name
            got = lowres.cpu().numpy() if name == "classifier.4" else m.read_activation(name_gpu, want.numel())
            want = want.numpy()
            assert got.shape == want.shape, (name, got.shape, want.shape)
            scale = float(np.abs(want).max())
            err = float(np.abs(got - want).max())
            report[name] = err / scale
            assert err <= (rlog if name == "classifier.4" else rl) * scale, f"{name}: max err {err} vs scale {scale} ({mode})"
        print(mode, "%dx%d" % size, "head rel err", {k: "%.2e" % v for k, v in report.items()})
        # the calibration guard and the stored powers cover the new tensors by name
        peaks = m.activation_peaks(x.to(DEV))
        assert len(peaks) == len(topology.conv_units(DL)) - 1 and "classifier.0.convs.4.1" in peaks
        assert peaks["classifier.0.convs.4.1"] == pytest.approx(float(ref["classifier.0.convs.4"].abs().max()), rel=rl)
        for n in ("classifier.0.concat", "classifier.0.convs.4", "classifier.0.convs.3.0", "classifier.1"):
            assert m.activation_exponent(n) == 0
    finally:
        m.set_keep_activations(False)


_REF = {}


def _reference(oracle, n, h, w, idx):
    key = (n, h, w, tuple(idx))
    if key not in _REF:
        x = frames(idx, h, w)
        _REF[key] = (x,) + tuple(deeplab_oracle.predict_labels(oracle, x))
    return _REF[key]


@pytest.mark.parametrize("n,h,w", [(1, 1024, 1024), (1, 600, 1024), (1, 203, 317), (1, 64, 64), (2, 96, 96)])
def test_end_to_end_against_oracle(oracle, models, n, h, w):
    """Logits and labels in the three modes; at 64 x 64 (an 8 x 8 map) and 96 x 96 (12 x 12) every tap of the dilated
    convolutions but the centre one, or all of them at dilation 12 and beyond the map, reads padding."""
    x, labels_ref, counts_ref, logits_ref, lowres_ref = _reference(oracle, n, h, w, list(range(7, 7 + n)))
    scale = float(logits_ref.abs().max())
    for mode in MODES:
        m = models[mode]
        _, rlog = RTOL[mode]
        labels, counts, lowres = m.predict_labels(x.to(DEV), return_lowres=True)
        logits = m(x.to(DEV))
        torch.cuda.synchronize()
        err = float((logits.cpu() - logits_ref).abs().max())
        err_low = float((lowres.cpu() - lowres_ref).abs().max())
        print(mode, (n, h, w), "logit err %.3e lowres err %.3e scale %.3f" % (err, err_low, scale))
        assert err_low <= rlog * scale and err <= rlog * scale, (mode, err_low, err, scale)
        if mode != "bf16":
            flips = adjudicated_flips(labels, logits_ref, err, oracle, x)
            if flips == 0:
                assert torch.equal(counts.cpu(), counts_ref)
        else:
            assert float((labels.cpu() == labels_ref).float().mean()) >= 0.97


def test_batch_of_different_images_equals_each_alone(models):
    """The pooled vector is per image: a batch of two DIFFERENT frames gives each frame's own result, bit for bit."""
    a, b = frames([11], 160, 224), frames([12], 160, 224)
    both = torch.cat([a, b])
    for mode, m in models.items():
        lb = m.lowres_logits(both.to(DEV))
        la, lb1 = m.lowres_logits(a.to(DEV)), m.lowres_logits(b.to(DEV))
        torch.cuda.synchronize()
        assert torch.equal(lb[0:1], la) and torch.equal(lb[1:2], lb1), mode
        assert not torch.equal(la, lb1)


def test_op_records_autotune_and_plan_tiles(models):
    m = models["f16x2"]
    x = frames([3], 256, 256).to(DEV)
    m.set_profiling(True)
    try:
        for _ in range(3):
            m.lowres_logits(x)
        recs = m.op_records()
    finally:
        m.set_profiling(False)
    kinds = [r["kernel"] for r in recs]
    names = [r["name"] for r in recs]
    assert kinds.count("aspp_pool") == 1 and kinds.count("concat") == 1 and kinds.count("head1x1") == 1
    assert names[names.index("classifier.0.convs.4") + 1] == "classifier.0.concat"
    head = names[names.index("classifier.0.convs.0.0"):]
    assert head[:4] == ["classifier.0.convs.%d.0" % i for i in range(4)]
    assert head[4:9] == ["classifier.0.convs.4", "classifier.0.concat", "classifier.0.project.0", "classifier.1", "classifier.4"]
    assert all(r["ms"] > 0 for r in recs)
    want = m.lowres_logits(x).cpu()
    tiles = m.autotune(x, reps=1)
    assert len(tiles) == sum(1 for r in recs if r["kernel"] == "conv_dma") == 59
    assert torch.equal(m.lowres_logits(x).cpu(), want)           # results do not depend on the tile
    m.set_plan_tiles(tiles)


def test_wrong_architecture_blob_is_refused(dl_sd, models, built_lib):
    blob = torch.from_numpy(pack_state_dict(dl_sd, "fp32", DL)).to(DEV)
    f = FCNResNet50("fp32").to(DEV)
    with pytest.raises(RuntimeError, match="trailer mismatch"):
        f._attach(blob)
    d = DeepLabV3ResNet50("fp32").to(DEV)
    d._attach(blob)
    # the RCCL broadcast of the C ABI is FCN's; the model object broadcasts through torch.distributed
    dummy = C.c_void_p(1)
    assert built_lib.nbc_bcast_weights(d._ctx, dummy, 0, 0, None) == _lib.NBC_ERR_STATE
    assert "FCN-ResNet-50 only" in _lib.last_error()


LAYOUT = [("epinette_gelee", "a01.png", 40, 256, 256), ("sapin", "s1.bmp", 41, 200, 256),
          ("epinette_non_gelee", "n1.png", 42, 136, 256), ("sapin", "s0.png", 43, 256, 256)]


def test_predict_and_evaluate_folders_pick_deeplab_from_the_checkpoint(tmp_path, dl_sd, oracle, built_lib):
    """A DeepLabV3 .pt, no --arch: predict's CSV and label PNGs and evaluate's confusion rows equal those built from the
    oracle's labels."""
    root = str(tmp_path / "fold")
    frames_ = {}
    for wood, name, idx, h, w in LAYOUT:
        for sub in ("samples", "duals"):
            os.makedirs(os.path.join(root, sub, wood), exist_ok=True)
        img = synth.make_frame(idx, h, w)
        Image.fromarray(img, mode="RGB").save(os.path.join(root, "samples", wood, name))
        png = name.replace("bmp", "png")
        lab = deeplab_oracle.predict_labels(oracle, torch.from_numpy(synth.normalize_frame(img))[None])[0][0].numpy().astype(np.uint8)
        grey = np.array([0, 127, 255], np.uint8)[(lab + (np.arange(lab.size).reshape(lab.shape) % 7 == 0)) % 3]
        Image.fromarray(grey, mode="L").save(os.path.join(root, "duals", wood, png))
        frames_[(wood, png)] = (img, lab, grey)
    ckpt = os.path.join(root, "best_model.pt")
    torch.save({k: torch.from_numpy(v) for k, v in dl_sd.items()}, ckpt)

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

    st = ev.evaluate_folder(root, ckpt, precision="f16x2", device_index=0)
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
    assert json.load(open(os.path.join(root, ev.SUMMARY_JSON)))["images_evaluated"] == len(LAYOUT)
