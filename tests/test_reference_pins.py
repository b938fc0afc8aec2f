"""Every host restatement of the reference against what the reference's own code returned (tests/golden/ref_*.npz, recorded
by oracle/record_reference.py): the Lovasz-Softmax and cross-entropy helpers, the metrics and statistics formulas, the grey
decode, and the oracle's head and forward.  No device.

A recorded float value v_ref is the reference's float32 result; ``d_ref`` is its distance from our float64 restatement when
it was recorded (absolute for the Lovasz values, relative for the cross-entropies; at most 1e-6, the recipe's condition).
A restatement passes within ``d_ref + 1e-7``: the float32 rounding the reference itself carries plus one float32 ulp of
room for another torch build's summation order.  A misread definition moves these values by percent.

Still restated and not pinned here: the ResNet-50 trunk (torchvision is absent; the recorded forward runs on OUR trunk, so
``test_oracle_forward_and_head`` pins the head, the interpolation and eval mode only), DeepLabHead, EfficientNet, and the
absent-class rule of ``PixelWiseF1`` (utils.py:222-226), whose caller needs scikit-image.

Bit equality of float32 results (the oracle's forward; the re-run recipe) is asked where ``torch.__version__`` and the CPU
(``reference_pins.cpu_name``) are the recorded ones: the same torch on another processor adds float32 numbers in another
order (measured: 1.2e-6 of the logit range between two machines).  The recipe itself refuses to record a forward that is
not bit-equal to ``OracleFCNResNet50.forward`` in its own process, whatever the machine.
"""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from neuralbarkcalculator_amd import metrics, synth
from neuralbarkcalculator_amd import stats as st

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import lovasz_oracle as lo  # noqa: E402
import pixel_ce_oracle as po  # noqa: E402
import reference_pins as rp  # noqa: E402

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROOM = 1e-7
LOGIT_RTOL_FP32 = 5e-6                # tests/test_gpu_parity.py


def _close(value, recorded, d_ref, relative):
    if np.isnan(recorded):
        return bool(np.isnan(value))
    return abs(value - recorded) <= (d_ref + ROOM) * (abs(recorded) if relative else 1.0)


@pytest.mark.parametrize("hw", rp.LOSS_SHAPES)
def test_lovasz_restatements(hw):
    g = rp.loss_fixture(*hw)
    worst = {"f32": 0.0, "f64": 0.0}
    for i in range(6):
        logits, grey = g["logits"][i], g["grey"][i]
        for name, fn in (("f32", lo.terms_torch_f32), ("f64", lo.terms_float64)):
            terms, counts = fn(logits, grey)
            assert np.array_equal(counts > 0, g["present"][i]), (i, name)
            assert np.array_equal(counts, np.bincount(g["classes"][i].ravel(), minlength=3))
            loss = metrics.lovasz_loss(terms, counts)
            assert lo.loss(terms, counts) == loss or (np.isnan(loss) and np.isnan(lo.loss(terms, counts)))
            if np.isnan(g["lovasz"][i]):
                assert np.isnan(loss) and np.all(np.isnan(terms[counts > 0])), (i, name, terms)
                continue
            assert np.all(terms[counts == 0] == 0.0)
            for c in range(3):
                assert _close(terms[c], g["lovasz_terms"][i, c], g["d_lovasz_terms"][i, c], False), (i, name, c, terms, g["lovasz_terms"][i])
            assert _close(loss, g["lovasz"][i], g["d_lovasz"][i], False), (i, name, loss, g["lovasz"][i])
            worst[name] = max(worst[name], abs(loss - g["lovasz"][i]), float(np.abs(terms - g["lovasz_terms"][i]).max()))
    print("%dx%d Lovasz: worst |restatement - reference| f32 %.3g, f64 %.3g; d_ref %.3g"
          % (hw + (worst["f32"], worst["f64"], max(g["d_lovasz"].max(), g["d_lovasz_terms"].max()))))


@pytest.mark.parametrize("hw", rp.LOSS_SHAPES)
def test_cross_entropy_restatements(hw):
    g = rp.loss_fixture(*hw)
    pixels = hw[0] * hw[1]
    worst = 0.0
    for i in range(6):
        logits, grey, cls = g["logits"][i], g["grey"][i], g["classes"][i].astype(np.int64)
        assert np.array_equal(po.target_classes(grey), cls)
        S, K = po.sums_float64(logits, grey)
        assert int(K.sum()) == pixels
        terms, counts = lo.terms_float64(logits, grey)
        got = {"ce": [(po.reference_procedure_f32(logits, cls, (1, 1, 1)), g["ce"][i], g["d_ce"][i]),
                      (po.weighted_float64(logits, cls, (1, 1, 1)), g["ce"][i], g["d_ce"][i]),
                      (metrics.cross_entropy(S, pixels), g["ce"][i], g["d_ce"][i])]}
        for k, w in enumerate(g["weights"]):
            w = [float(v) for v in w]
            wce = metrics.weighted_cross_entropy(S, pixels, w)
            got["wce%d" % k] = [(po.reference_procedure_f32(logits, cls, w), g["wce"][i, k], g["d_wce"][i, k]),
                                (po.weighted_float64(logits, cls, w), g["wce"][i, k], g["d_wce"][i, k]),
                                (wce, g["wce"][i, k], g["d_wce"][i, k])]
            got["mixed%d" % k] = [(metrics.mixed_loss(wce, metrics.lovasz_loss(terms, counts)), g["mixed"][i, k], g["d_mixed"][i, k])]
        for what, rows in got.items():
            for j, (value, recorded, d_ref) in enumerate(rows):
                assert _close(value, recorded, d_ref, True), (i, what, j, value, recorded, d_ref)
                if not np.isnan(recorded):
                    worst = max(worst, abs(value - recorded) / abs(recorded))
    assert np.isnan(g["ce"][5]) and np.all(np.isnan(g["wce"][5])) and np.all(np.isnan(g["mixed"][5]))
    assert np.allclose(g["weights"][0], metrics.REFERENCE_CLASS_WEIGHTS, rtol=1e-7, atol=0)     # get_pos_weight(), in float32
    print("%dx%d cross-entropies: worst relative |restatement - reference| %.3g; d_ref %.3g"
          % (hw + (worst, max(g["d_ce"].max(), g["d_wce"].max(), g["d_mixed"].max()))))


def test_grey_decode_on_all_256_levels():
    g = rp.load("ref_decode")
    grey, classes = g["grey"], g["classes"]
    assert sorted(grey.ravel().tolist()) == list(range(256))
    assert np.array_equal(metrics.target_classes(grey), classes)
    assert np.array_equal(lo.target_classes(grey), classes)
    assert np.array_equal(po.target_classes(grey), classes)
    assert np.bincount(classes.ravel()).tolist() == [64, 128, 64]


def _stats_rows(frames, greys):
    rows = []
    for i, (f, grey) in enumerate(zip(frames, greys)):
        v = f.reshape(-1, 3).astype(np.uint64)
        cls = metrics.target_classes(grey)
        rows.append([i, f.shape[0], f.shape[1], st.STATUS_OK] + [int(s) for c in range(3) for s in (v[:, c].sum(), (v[:, c] * v[:, c]).sum())]
                    + [int((cls == y).sum()) for y in range(3)] + [int(((grey != 0) & (grey != 127) & (grey != 255)).sum())])
    return np.asarray(rows, dtype=np.int64)


def test_dataset_statistics():
    s = rp.stats_fixture()
    assert sorted(f.shape[:2] for f in s["frames"])[0] == (1, 2) and len({f.shape[:2] for f in s["frames"]}) == 4
    for grey, classes in zip(s["greys"], s["classes"]):
        assert np.array_equal(metrics.target_classes(grey), classes)
    items = [{"name": str(i), "wood": "sapin"} for i in range(len(s["frames"]))]
    _, summary = st.report(items, _stats_rows(s["frames"], s["greys"]))
    for c in range(3):
        rel_m = abs(summary["mean"][c] - s["mean"][c]) / s["mean"][c]
        rel_s = abs(summary["std"][c] - s["std"][c]) / s["std"][c]
        print("channel %d: relative |stats.report - reference| mean %.3g, std %.3g" % (c, rel_m, rel_s))
        assert rel_m <= 1e-6 and rel_s <= 1e-6
        assert rp.within_one_f32_ulp(summary["pos_weight"][c], s["pos_weight"][c]), (c, summary["pos_weight"], s["pos_weight"])
    assert summary["class_counts"] == np.sum([np.bincount(c.ravel(), minlength=3) for c in s["classes"]], axis=0).tolist()


def test_iou_and_f1_from_confusions():
    """``lovasz_losses.iou`` returns percent, ``f1_score`` fractions: both compared on the fraction scale.  Where a class is
    on neither side, ``f1_score`` says 0 and ``metrics.f1`` applies the rule of utils.py:222-226 on top (the mean of the
    other two), which no recorded call covers."""
    g = rp.load("ref_metrics")
    seen_empty = seen_predicted_only = False
    for pred, grey, classes, iou, f1 in zip(g["pred"], g["grey"], g["classes"], g["iou"], g["f1_score"]):
        assert np.array_equal(metrics.target_classes(grey), classes)
        conf = metrics.confusion_numpy(pred, classes)
        np.testing.assert_allclose(metrics.iou(conf) / 100, iou / 100, rtol=0, atol=1e-12)
        ours = metrics.f1(conf) / 100
        on_a_side = (conf.sum(axis=0) + conf.sum(axis=1)) > 0
        np.testing.assert_allclose(ours[on_a_side], f1[on_a_side], rtol=0, atol=1e-12)
        for c in np.nonzero(~on_a_side)[0]:
            seen_empty = True
            assert iou[c] == 100.0 and f1[c] == 0.0                       # EMPTY = 1.
            assert abs(ours[c] - np.delete(f1, c).mean()) <= 1e-12
        seen_predicted_only |= bool(((conf.sum(axis=1) == 0) & (conf.sum(axis=0) > 0)).any())
    assert seen_empty and seen_predicted_only


@pytest.mark.parametrize("hw", rp.HEAD_SHAPES)
def test_oracle_forward_and_head(oracle_model, hw):
    """The reference's ``SimpleSegmentationModel.forward`` around its own ``FCNHead(2048, 3)`` in eval mode, on this
    repository's trunk: the trunk itself is NOT pinned (the fixture's ``note`` says so), the head's layer order, the
    interpolation and the key names are."""
    g = rp.load("ref_head_%dx%d" % hw)
    assert "NOT pinned" in str(g["note"])
    assert list(oracle_model.classifier.state_dict().keys()) == list(g["head_keys"])
    frame = g["frame"]
    assert np.array_equal(frame, synth.make_frame(int(g["frame_index"]), *hw))
    x = torch.from_numpy(synth.normalize_frame(frame))[None]
    threads = torch.get_num_threads()
    torch.set_num_threads(1)                         # the recorded run's summation order
    try:
        with torch.no_grad():
            logits = oracle_model(x)[0].numpy()
    finally:
        torch.set_num_threads(threads)
    want = g["logits"]
    err = float(np.abs(logits - want).max()) / float(np.abs(want).max())
    print("%dx%d forward: |oracle - reference| %.3g of the logit range; d_ref %.3g" % (hw + (err, float(g["d_ref"]))))
    if rp.same_build(g):                             # the recorded torch on the recorded kind of CPU: the same bits
        assert np.array_equal(logits, want), err
    else:                                            # oneDNN adds in another order there
        assert err <= LOGIT_RTOL_FP32
    assert np.array_equal(np.argmax(want, axis=0), g["labels"])


def test_the_recipe_reproduces_the_committed_fixtures(tmp_path):
    from oracle import record_reference as rr
    if not os.path.isdir(rr.DEFAULT_REFERENCE):
        pytest.skip("no reference on this machine")
    p = subprocess.run([sys.executable, "-m", "oracle.record_reference", "--out", str(tmp_path)], cwd=REPO, capture_output=True,
                       text=True, timeout=600)
    assert p.returncode == 0, (p.stdout + p.stderr)[-3000:]
    written = sorted(f[:-4] for f in os.listdir(tmp_path))
    assert written == rp.fixture_names()
    for name in written:
        new, old = np.load(str(tmp_path / (name + ".npz")), allow_pickle=False), rp.load(name)
        assert sorted(new.files) == sorted(old.files), name
        same_build = (str(new["torch_version"]), str(new["cpu"])) == (str(old["torch_version"]), str(old["cpu"]))
        for key in old.files:
            if key in ("torch_version", "cpu"):          # where the values were made: strings of any length
                continue
            a, b = new[key], old[key]
            assert a.dtype == b.dtype and a.shape == b.shape, (name, key)
            is_input = key.startswith(("frame", "grey", "weights")) or a.dtype == np.float16      # stored logits are float16
            if a.dtype.kind != "f" or is_input or same_build:
                assert np.array_equal(a, b, equal_nan=(a.dtype.kind == "f")), (name, key)
            elif not key.startswith("d_"):               # another torch or CPU: the recipe's own condition bounds each d_ref
                np.testing.assert_allclose(a, b, rtol=1e-5, atol=1e-6, equal_nan=True, err_msg="%s %s" % (name, key))
