"""Per-image BatchNorm statistics on the f16x2 pipe (bn_statistics "image_f16x2") on the GPU against the CPU oracle of
tests/helpers/bn_image_oracle.py: every conv unit in keep mode, end to end, the statistics and apply kernels on the operands
they read, batch invariance and run-to-run bits, mode switches, tiles, dropout draws, the op records, the range word and the
folder drivers with --bn_stats image_f16x2."""
import csv
import json
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F
from PIL import Image

from neuralbarkcalculator_amd import metrics, synth, topology
from neuralbarkcalculator_amd import evaluate as ev
from neuralbarkcalculator_amd import predict as drv
from neuralbarkcalculator_amd.model import FCNResNet50, fcn_resnet50
from neuralbarkcalculator_amd.postprocess import remove_small_zones

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import bn_image_oracle  # noqa: E402
from bn_image_f16x2 import (LAYER_RTOL_FP32, LOGIT_RTOL_FP32, MISJUDGED_BN, adjudicated_flips, frames,  # noqa: E402
                            misjudged_state_dict, within, worst)

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODE = "image_f16x2"
RANGE_BIT = 2                                                   # NBC_NONFINITE_BN_RANGE


@pytest.fixture(scope="module")
def oracle(sd_np):
    torch.set_num_threads(min(16, len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else 8))
    return bn_image_oracle.load(sd_np)


@pytest.fixture(scope="module")
def oracle64(oracle):
    return bn_image_oracle.double_of(oracle)


def _model(sd):
    return fcn_resnet50(precision="f16x2", bn_statistics=MODE).load_state_dict(sd).to(DEV)


@pytest.fixture(scope="module")
def model(sd_np, built_lib):
    return _model(sd_np)


def _word(m) -> int:
    """The context's sticky word as it stands (nbc_nonfinite_peek_async)."""
    host = torch.zeros(1, dtype=torch.int32).pin_memory()
    m.nonfinite_peek_async(host)
    torch.cuda.synchronize()
    return int(host[0])


def _kept(m, x, names, numel):
    m.set_keep_activations(True)
    try:
        m.lowres_logits(x.to(DEV))
        torch.cuda.synchronize()
        return {k: torch.from_numpy(m.read_activation(k, numel[k]).copy()) for k in names}
    finally:
        m.set_keep_activations(False)


@pytest.mark.parametrize("h,w", [(203, 317), (64, 1024)])
def test_every_unit_in_keep_mode(model, oracle, oracle64, h, w):
    x = frames([5], h, w)
    want = bn_image_oracle.layer_outputs(oracle, x)
    names = [k for k in want if k != "classifier.4"]
    got = _kept(model, x, names, {k: want[k].numel() for k in names})
    cache = {}

    def w64(k):
        def f():
            if not cache:
                cache.update(bn_image_oracle.layer_outputs(oracle64, x.double()))
            return cache[k]
        return f
    for k, g in got.items():
        assert g.shape == want[k].shape, k
        within(g, want[k], w64(k), LAYER_RTOL_FP32, "%dx%d %s" % (h, w, k), "layers %dx%d" % (h, w))
    print("bn image_f16x2 layers %dx%d: worst adjudicated (gpu, f32 oracle) %s" % (h, w, worst.get("layers %dx%d" % (h, w))))
    assert _word(model) == 0


@pytest.mark.parametrize("n,h,w", [(1, 203, 317), (1, 64, 1024), (2, 96, 160), (1, 16, 16)])
def test_end_to_end(model, oracle, oracle64, n, h, w):
    x = frames(range(11, 11 + n), h, w)
    labels_ref, counts_ref, logits_ref, lowres_ref = bn_image_oracle.predict_labels(oracle, x)
    labels, counts, lowres = model.predict_labels(x.to(DEV), return_lowres=True)
    lowres = lowres.cpu()
    within(lowres, lowres_ref, lambda: bn_image_oracle.lowres_logits(oracle64, x.double()), LOGIT_RTOL_FP32,
           "%dx%dx%d logits" % (n, h, w), "logits")
    err = max(float((lowres - lowres_ref).abs().max()), 1e-7)
    flips = adjudicated_flips(labels, logits_ref, 4.0 * err, oracle64, x, "%dx%dx%d" % (n, h, w))
    if flips == 0:
        assert torch.equal(counts.cpu(), counts_ref)
    assert _word(model) == 0                                    # an ordinary checkpoint: neither bit


def _unit(name):
    return [u for u in topology.conv_units() if u.name == name][0]


def _unit_in_torch(sd, u, x_in, identity, dtype):
    """conv, per-image BatchNorm (biased variance, eps 1e-5), + identity, ReLU of unit u on x_in, in torch at dtype."""
    t = lambda k: torch.from_numpy(sd[k]).to(dtype)
    y = F.conv2d(x_in.to(dtype), t(u.name + ".weight"), stride=u.stride, padding=u.pad, dilation=u.dil)
    y = torch.cat([F.batch_norm(y[i:i + 1], None, None, t(u.bn + ".weight"), t(u.bn + ".bias"), training=True, eps=1e-5)
                   for i in range(y.shape[0])])
    if identity is not None:
        y = y + identity.to(dtype)
    return F.relu(y) if u.relu else y


OPERAND_CASES = [
    # unit, the kept tensor it reads, the kept identity it adds, image
    ("backbone.conv1", None, None, (203, 317)),                  # the stem reads the image itself
    ("backbone.layer1.0.downsample.0", "backbone.maxpool", None, (203, 317)),
    ("backbone.layer1.0.conv3", "backbone.layer1.0.conv2", "backbone.layer1.0.downsample.0", (203, 317)),
    ("backbone.layer3.2.conv2", "backbone.layer3.2.conv1", None, (64, 1024)),
    ("classifier.0", "backbone.layer4.2.conv3", None, (203, 317)),
]


@pytest.fixture(scope="module")
def kept_operands(model):
    out = {}
    for h, w in sorted({c[3] for c in OPERAND_CASES}):
        names = sorted({n for c in OPERAND_CASES if c[3] == (h, w) for n in c[:3] if n})
        # room for the largest kept tensor: layer4's 2048 channels of an (h / 8) x (w / 8) map
        out[(h, w)] = _kept(model, frames([5], h, w), names, {n: 40 * (h + 8) * (w + 8) for n in names})
    return out


@pytest.mark.parametrize("name,src,idt,shape", OPERAND_CASES, ids=[c[0] for c in OPERAND_CASES])
def test_statistics_and_apply_on_the_operands_they_read(model, sd_np, kept_operands, name, src, idt, shape):
    """From the GPU's own kept input (and identity) of the unit: conv, per-image BatchNorm, add, ReLU in float64 and in f32
    torch; the GPU's distance to float64, relative to the tensor's range, is held to max(4e-6, 1.5 x the f32 form's)."""
    u, kept = _unit(name), kept_operands[shape]
    x_in = kept[src] if src else frames([5], *shape)
    identity = kept[idt] if idt else None
    w64 = _unit_in_torch(sd_np, u, x_in, identity, torch.float64)
    w32 = _unit_in_torch(sd_np, u, x_in, identity, torch.float32)
    got = kept[name]
    assert got.shape == w64.shape
    scale = float(w64.abs().max())
    e_gpu = float((got.double() - w64).abs().max()) / scale
    e_f32 = float((w32.double() - w64).abs().max()) / scale
    print("bn image_f16x2 operands %s (%s) %dx%d: gpu %.3e, f32 torch %.3e of the range %.4g" % (name, u.bn, *shape, e_gpu,
                                                                                               e_f32, scale), flush=True)
    assert e_gpu <= max(4e-6, 1.5 * e_f32), (name, e_gpu, e_f32)


def test_batch_of_two_equals_each_alone_and_runs_repeat(model):
    x = torch.cat([frames([21], 96, 160), frames([22], 96, 160) * 0.5 + 0.3])
    both = model.lowres_logits(x.to(DEV)).cpu()
    again = model.lowres_logits(x.to(DEV)).cpu()
    assert torch.equal(both, again)
    for i in range(2):
        assert torch.equal(both[i:i + 1], model.lowres_logits(x[i:i + 1].to(DEV)).cpu())


def test_mode_switches_leave_running_mode_bits_alone(sd_np, built_lib):
    x = frames([9], 96, 160).to(DEV)
    want = FCNResNet50("f16x2").load_state_dict(sd_np).to(DEV).lowres_logits(x).cpu()
    m = _model(sd_np)
    img = m.lowres_logits(x).cpu()
    assert m.bn_statistics == MODE
    assert torch.equal(m.set_bn_statistics("running").lowres_logits(x).cpu(), want)
    assert m.fused_pairs() > 0                                   # running mode is back on its fused pairs
    assert float((img - want).abs().max()) > 1e-2 * float(want.abs().max())     # the mode is live
    assert torch.equal(m.set_bn_statistics(MODE).lowres_logits(x).cpu(), img)
    assert m.fused_pairs() == 0


def test_tiles_relate_as_in_running_mode(sd_np, built_lib):
    x = frames([7, 8], 128, 192).to(DEV)
    same = {}
    for mode in ("running", MODE):
        m = fcn_resnet50(precision="f16x2", bn_statistics=mode).load_state_dict(sd_np).to(DEV)
        want = m.lowres_logits(x).cpu()
        tiles = m.autotune(x, reps=1)
        assert len(tiles) == 54
        tuned = m.lowres_logits(x).cpu()
        m.set_plan_tiles(tiles)
        assert torch.equal(m.lowres_logits(x).cpu(), tuned)
        same[mode] = (torch.equal(tuned, want), float((tuned - want).abs().max()) / float(want.abs().max()))
        print("bn image_f16x2 tiles, %s: tuned tiles %s the default-tile logits (max difference %.3e of the range)"
              % (mode, "repeat" if same[mode][0] else "do not repeat", same[mode][1]), flush=True)
    if same["running"][0]:
        assert same[MODE][0]
    else:                                                        # not bitwise there: f32 grade here, as there
        assert same[MODE][1] <= LOGIT_RTOL_FP32 and same["running"][1] <= LOGIT_RTOL_FP32


def test_dropout_draws_at_p0_are_the_forward(model):
    x = frames([31, 32], 96, 160).to(DEV)
    _, counts, lowres = model.predict_labels(x, return_lowres=True)
    d_counts, d_lowres = model.dropout_draws(1, [101, 102], p=0.0, small_zones=False, return_lowres=True)
    assert torch.equal(d_lowres[0].cpu(), lowres.cpu())
    assert torch.equal(d_counts[0].cpu(), counts.cpu())


def test_op_records_list_the_statistics_and_apply_ops(model):
    x = frames([3], 256, 256).to(DEV)
    model.set_profiling(True)
    try:
        for _ in range(2):
            model.lowres_logits(x)
        recs = model.op_records()
    finally:
        model.set_profiling(False)
    names = [r["name"] for r in recs]
    kinds = [r["kernel"] for r in recs]
    assert kinds.count("conv_dma") == 54 and kinds.count("bn_stats") == 54 and kinds.count("bn_apply") == 54
    i = names.index("backbone.layer3.4.conv2")
    assert names[i + 1: i + 3] == ["backbone.layer3.4.bn2.stats", "backbone.layer3.4.bn2.apply"]
    i = names.index("backbone.conv1")
    assert names[i + 1: i + 4] == ["backbone.bn1.stats", "backbone.bn1.apply", "backbone.maxpool"]
    i = names.index("backbone.layer1.0.downsample.0")
    assert names[i + 1: i + 4] == ["backbone.layer1.0.downsample.1.stats", "backbone.layer1.0.downsample.1.apply",
                                   "backbone.layer1.0.conv3"]
    assert names[-4:-1] == ["classifier.1.stats", "classifier.1.apply", "classifier.4"]
    assert all(r["ms"] > 0 for r in recs)
    assert [r["launches"] for r in recs if r["kernel"] == "bn_stats"] == [2] * 54
    assert model.fused_pairs() == 0


@pytest.mark.parametrize("log2_var", [40, -40], ids=["A_var_x2^40", "B_var_x2^-40"])
def test_range_word_on_misjudged_running_statistics(sd_np, built_lib, log2_var):
    """Running statistics that never saw the data: the stored raw values of the channels behind them sit 2^20 below (A) or
    above (B) where the pieces hold them.  A leaves finite numbers, so only the statistics kernel can tell: bit 2.  B leaves
    f16's range and may raise either bit.  The kernels compute finite or NaN numbers: no fault is involved."""
    m = _model(misjudged_state_dict(sd_np, log2_var))
    assert m.pack_flags == 0
    m.lowres_logits(frames([4], 96, 160).to(DEV))
    word = _word(m)
    print("bn image_f16x2 %s x 2^%d: word %d" % (MISJUDGED_BN, log2_var, word), flush=True)
    if log2_var > 0:
        assert word & RANGE_BIT
    assert word != 0 and m.nonfinite_seen()
    assert _word(m) == 0                                        # nonfinite_seen resets it


def test_both_side_arrays_are_needed(sd_np, built_lib):
    from neuralbarkcalculator_amd import _lib
    from neuralbarkcalculator_amd.model import pack_bn_affine, pack_bn_raw, pack_state_dict
    m = FCNResNet50("f16x2").set_bn_statistics(MODE).to(DEV)
    blob = torch.from_numpy(pack_state_dict(sd_np, "f16x2")).to(DEV)
    affine = torch.from_numpy(pack_bn_affine(sd_np)).to(DEV)
    m._attach(blob)                                             # the blob alone
    assert m._lib.nbc_reserve(m._ctx, 1, 96, 160) == _lib.NBC_ERR_STATE and "nbc_attach_bn_affine" in _lib.last_error()
    m._attach(blob, affine)                                     # no raw-convolution array yet
    assert m._lib.nbc_reserve(m._ctx, 1, 96, 160) == _lib.NBC_ERR_STATE and "nbc_attach_bn_raw" in _lib.last_error()
    x = frames([9], 96, 160).to(DEV)
    with pytest.raises(RuntimeError, match="nbc_attach_bn_raw"):
        m.lowres_logits(x)
    m._attach(blob, affine, torch.from_numpy(pack_bn_raw(sd_np)[0]).to(DEV))
    assert torch.equal(m.lowres_logits(x).cpu(), _model(sd_np).lowres_logits(x).cpu())
    # a context that loaded its weights through the C convenience call has both (clone_shared passes them on)
    assert torch.equal(m.clone_shared().lowres_logits(x).cpu(), m.lowres_logits(x).cpu())


def test_calibration_forward_runs_in_the_mode(model):
    peaks = model.activation_peaks(frames([3], 96, 160).to(DEV))
    ok, bad = FCNResNet50.f16x2_range_ok(peaks)
    assert ok and len(peaks) == 54, bad
    assert _word(model) == 0


LAYOUT = [("epinette_gelee", "a01.png", 60, 136, 256), ("sapin", "s1.bmp", 61, 200, 256), ("sapin", "s0.png", 63, 136, 256)]


def _make_folder(root, sd, oracle=None):
    frames_ = {}
    for wood, name, idx, h, w in LAYOUT:
        for sub in ("samples", "duals"):
            os.makedirs(os.path.join(root, sub, wood), exist_ok=True)
        img = synth.make_frame(idx, h, w)
        Image.fromarray(img, mode="RGB").save(os.path.join(root, "samples", wood, name))
        if oracle is None:
            continue
        png = name.replace("bmp", "png")
        lab = bn_image_oracle.predict_labels(oracle, torch.from_numpy(synth.normalize_frame(img))[None])[0][0].numpy()
        lab = lab.astype(np.uint8)
        grey = np.array([0, 127, 255], np.uint8)[(lab + (np.arange(lab.size).reshape(lab.shape) % 7 == 0)) % 3]
        Image.fromarray(grey, mode="L").save(os.path.join(root, "duals", wood, png))
        frames_[(wood, png)] = (img, lab, grey)
    ckpt = os.path.join(root, "best_model.pt")
    torch.save({k: torch.from_numpy(v) for k, v in sd.items()}, ckpt)
    return ckpt, frames_


def test_predict_and_evaluate_folders(tmp_path, sd_np, model, oracle, oracle64, built_lib):
    """The drivers' counts equal the oracle's up to adjudicated ties: this process's model gives each frame's labels, which
    are held to the oracle's by the label rule of the end-to-end test; the files the drivers write are then exactly those
    labels' (an image's bits depend neither on its batch nor on the process)."""
    root = str(tmp_path / "fold")
    ckpt, frames_ = _make_folder(root, sd_np, oracle)
    gpu_lab, flips = {}, 0
    for key, (img, lab, _) in frames_.items():
        x = torch.from_numpy(synth.normalize_frame(img))[None]
        _, _, logits_ref, lowres_ref = bn_image_oracle.predict_labels(oracle, x)
        labels, _, lowres = model.predict_labels(torch.from_numpy(img)[None].to(DEV), return_lowres=True)
        err = max(float((lowres.cpu() - lowres_ref).abs().max()), 1e-7)
        flips += adjudicated_flips(labels, logits_ref, 4.0 * err, oracle64, x, "folder %s/%s" % key)
        gpu_lab[key] = labels[0].cpu().numpy().astype(np.uint8)
    print("bn image_f16x2 folder: %d tie-level flips against the f32 oracle over %d images" % (flips, len(frames_)), flush=True)

    p = subprocess.run([sys.executable, "-m", "neuralbarkcalculator_amd.predict", root, "--model_path", ckpt, "--streams", "2",
                        "--bn_stats", MODE, "--precision", "f16x2", "--dropout_draws", "2"], cwd=REPO, capture_output=True,
                       text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-3000:]
    doc = json.load(open(os.path.join(root, "results", "dropout_summary.json")))
    assert (doc["bn_stats"], doc["precision"], doc["draws"], doc["images"]) == (MODE, "f16x2", 2, len(LAYOUT))
    rows = list(csv.reader(open(os.path.join(root, "results", "final_stats.csv")), delimiter="\t"))
    assert rows[0] == drv.CSV_HEADER and len(rows) == 1 + len(LAYOUT)
    for row in rows[1:]:
        name, wood = row[0], row[1]
        lab = remove_small_zones(gpu_lab[(wood, name)].copy())
        got = np.asarray(Image.open(os.path.join(root, "results", "outputs", wood, name)))
        assert np.array_equal(got, drv.label_png(lab)), name
        assert row == drv.stats_row(name, wood, lab.shape[0], lab.shape[1], int((lab == 1).sum()), int((lab == 2).sum()))

    p = subprocess.run([sys.executable, "-m", "neuralbarkcalculator_amd.evaluate", root, "--model_path", ckpt, "--streams", "2",
                        "--bn_stats", MODE], cwd=REPO, capture_output=True, text=True, timeout=600)     # --precision auto
    assert p.returncode == 0, p.stderr[-3000:]
    assert "running the folder again" not in p.stdout
    summary = json.load(open(os.path.join(root, ev.SUMMARY_JSON)))
    assert (summary["bn_statistics"], summary["precision"]) == (MODE, "f16x2") and summary["images_evaluated"] == len(LAYOUT)
    assert os.path.isfile(os.path.join(root, "results", "evaluation_stats.csv"))
    raw_t, clean_t, want_rows = np.zeros((3, 3), np.int64), np.zeros((3, 3), np.int64), []
    for wood, name, _, _, _ in LAYOUT:
        png = name.replace("bmp", "png")
        lab, grey = gpu_lab[(wood, png)], frames_[(wood, png)][2]
        t = metrics.target_classes(grey)
        raw, clean = metrics.confusion_numpy(lab, t), metrics.confusion_numpy(remove_small_zones(lab.copy()), t)
        raw_t += raw
        clean_t += clean
        want_rows.append(metrics.eval_row(png, wood, raw, clean))
    want = metrics.summarize(want_rows, raw_t, clean_t)["pooled"]
    for k, v in want.items():
        assert abs(summary["pooled"][k] - v) <= 1e-9, (k, summary["pooled"][k], v)


def test_auto_abandons_a_misjudged_checkpoint_and_repeats_in_fp32(tmp_path, sd_np, built_lib):
    sd = misjudged_state_dict(sd_np, 40)
    root, twin = str(tmp_path / "auto"), str(tmp_path / "image")
    ckpt, _ = _make_folder(root, sd)
    shutil.copytree(root, twin)
    p = subprocess.run([sys.executable, "-m", "neuralbarkcalculator_amd.predict", root, "--model_path", ckpt, "--streams", "2",
                        "--bn_stats", MODE, "--precision", "auto"], cwd=REPO, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-3000:]
    assert "running the folder again on the f32 MFMA" in p.stdout
    st = drv.predict_folder(twin, os.path.join(twin, "best_model.pt"), precision="fp32", device_index=0, streams=2,
                            bn_stats="image")
    assert st["images_total"] == len(LAYOUT)
    got = open(os.path.join(root, "results", "final_stats.csv"), "rb").read()
    assert got == open(os.path.join(twin, "results", "final_stats.csv"), "rb").read() and got.count(b"\n") == 1 + len(LAYOUT)
    # the label PNGs on disk are the second run's, none of the abandoned one
    for wood, name, _, _, _ in LAYOUT:
        png = os.path.join("results", "outputs", wood, name.replace("bmp", "png"))
        assert np.array_equal(np.asarray(Image.open(os.path.join(root, png))), np.asarray(Image.open(os.path.join(twin, png))))
    assert sorted(os.listdir(os.path.join(root, "results", "outputs", "sapin"))) == ["s0.png", "s1.png"]
