"""nbc_softmax_census on the GPU against its host restatement (calibration.census_cpu), word for word and byte for byte; its
batch and stream independence; non-finite logits; the model method; `evaluate --calibration` and `predict --confidence` end
to end.

No tolerance: the inputs are chosen so that none is needed.  census_cpu reports the margin of its input, the smallest
distance of any p_c * 65536 to a bin edge it could cross; the helper's seeds give more than 1e-7 on every shape (asserted
here on the host, from the reference alone), and two float64 evaluations of exp differ by a few units of 2^-53 relative, about
1e-11 on that scale, so the device quantises every pixel as the host does."""
import csv
import json
import os
import sys

import numpy as np
import pytest
import torch
from PIL import Image

from neuralbarkcalculator_amd import _lib, synth
from neuralbarkcalculator_amd import calibration as cal
from neuralbarkcalculator_amd import evaluate as ev
from neuralbarkcalculator_amd import predict as pr

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import calibration_cases as cc  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
ROW_GUARD, PLANE_GUARD = 4, 16                      # words / bytes on either side of the outputs
ROW_FILL, PLANE_FILL = -77, 0xA5


def _run(lib, logits, grey=None, plane=True, stream=None, ws=None):
    """One nbc_softmax_census call on device tensors, guard words around both outputs: (rows uint64 [n, WORDS], plane or None)
    as numpy."""
    n, _, h, w = logits.shape
    need = lib.nbc_softmax_census_workspace_bytes(n, h, w)
    ws = torch.empty(need, dtype=torch.uint8, device=DEV) if ws is None else ws
    rows = torch.full((n * cal.WORDS + 2 * ROW_GUARD,), ROW_FILL, dtype=torch.int64, device=DEV)
    out = torch.full((n * h * w + 2 * PLANE_GUARD,), PLANE_FILL, dtype=torch.uint8, device=DEV) if plane else None
    s = stream if stream is not None else torch.cuda.current_stream(DEV)
    _lib.check(lib.nbc_softmax_census(logits.data_ptr(), None if grey is None else grey.data_ptr(), n, h, w, ws.data_ptr(), need,
                                      rows.data_ptr() + 8 * ROW_GUARD, None if out is None else out.data_ptr() + PLANE_GUARD,
                                      s.cuda_stream), "nbc_softmax_census")
    s.synchronize()
    r = rows.cpu().numpy()
    assert (r[:ROW_GUARD] == ROW_FILL).all() and (r[-ROW_GUARD:] == ROW_FILL).all()
    r = r[ROW_GUARD:-ROW_GUARD].view(np.uint64).reshape(n, cal.WORDS)
    if out is None:
        return r, None
    p = out.cpu().numpy()
    assert (p[:PLANE_GUARD] == PLANE_FILL).all() and (p[-PLANE_GUARD:] == PLANE_FILL).all()
    return r, p[PLANE_GUARD:-PLANE_GUARD].reshape(n, h, w)


def _dev(a):
    return torch.from_numpy(np.array(a)).to(DEV)


@pytest.mark.parametrize("shape", list(cc.SHAPES))
def test_rows_and_plane_equal_the_host_census(built_lib, shape):
    logits, grey, with_t, without = cc.case(*shape)
    assert with_t[2] > cc.MARGIN and without[2] > cc.MARGIN, (with_t[2], without[2])
    L, G = _dev(logits), _dev(grey)
    for target, want in ((G, with_t), (None, without)):
        rows, plane = _run(built_lib, L, target, plane=True)
        bad = np.argwhere(rows != want[0])
        assert bad.size == 0, (shape, target is None, bad[:8], rows[tuple(bad[0])], want[0][tuple(bad[0])])
        assert np.array_equal(plane, want[1])
        rows2, none = _run(built_lib, L, target, plane=False)          # the plane is optional and changes nothing
        assert none is None and rows2.tobytes() == rows.tobytes()
    n, h, w = shape
    H = with_t[0][:, :cal.OFF_R].reshape(n, 3, 3, 256)
    assert int(H.sum()) == 3 * n * h * w and int(H[:, :, :, 255].sum()) > 0 and int(H[:, :, :, 0].sum()) > 0
    assert int(with_t[0][:, cal.OFF_NONFINITE].sum()) == 0
    assert int(without[0][:, cal.OFF_R: cal.OFF_R + 256].sum()) == 0      # without a target every pixel is a hit


def test_non_finite_pixels_count_in_their_own_word_only(built_lib):
    n, h, w = 3, 33, 65
    logits, grey = (np.array(a) for a in cc.case(n, h, w)[:2])
    spots = [(0, 0, 0, 0, np.nan), (0, 2, 32, 64, np.inf), (1, 1, 5, 7, -np.inf), (1, 0, 5, 8, np.nan), (1, 1, 5, 8, np.inf),
             (2, 2, 16, 3, -np.inf), (2, 0, 16, 3, -np.inf), (2, 1, 16, 3, -np.inf)]
    for i, c, y, x, v in spots:
        logits[i, c, y, x] = v
    want_rows, want_plane, margin = cal.census_cpu(logits, grey)
    assert margin > cc.MARGIN and want_rows[:, cal.OFF_NONFINITE].tolist() == [2, 2, 1]
    clean = cc.case(n, h, w)[2][0]
    rows, plane = _run(built_lib, _dev(logits), _dev(grey))
    assert np.array_equal(rows, want_rows) and np.array_equal(plane, want_plane)
    for i, _, y, x, _ in spots:
        assert plane[i, y, x] == 0
    # a non-finite pixel is missing from every other field: the histograms hold three entries fewer per such pixel
    for i in range(n):
        lost = int(clean[i, :cal.OFF_R].sum()) - int(rows[i, :cal.OFF_R].sum())
        assert lost == 3 * int(rows[i, cal.OFF_NONFINITE])


def test_batch_and_stream_independence(built_lib):
    """An image's row and plane are bit-identical alone, at each position of a batch of 3 (odd H * W: the images of a batch
    start at different alignments) and from two streams running at once."""
    n, h, w = 3, 33, 65
    logits, grey = cc.case(n, h, w)[:2]
    L, G = _dev(logits), _dev(grey)
    alone = [_run(built_lib, L[i:i + 1].contiguous(), G[i:i + 1].contiguous()) for i in range(n)]
    orders = [[0, 1, 2], [1, 2, 0], [2, 0, 1]]
    for order in orders:
        rows, plane = _run(built_lib, L[order].contiguous(), G[order].contiguous())
        for pos, i in enumerate(order):
            assert rows[pos].tobytes() == alone[i][0][0].tobytes(), (order, pos)
            assert plane[pos].tobytes() == alone[i][1][0].tobytes(), (order, pos)
    need = built_lib.nbc_softmax_census_workspace_bytes(n, h, w)
    outs = []
    for order in orders[:2]:
        outs.append((torch.empty((n, cal.WORDS), dtype=torch.int64, device=DEV), torch.empty((n, h, w), dtype=torch.uint8, device=DEV),
                     torch.empty(need, dtype=torch.uint8, device=DEV), L[order].contiguous(), G[order].contiguous(),
                     torch.cuda.Stream(DEV), order))
    torch.cuda.synchronize()
    for rows, plane, ws, Ls, Gs, s, _ in outs:
        _lib.check(built_lib.nbc_softmax_census(Ls.data_ptr(), Gs.data_ptr(), n, h, w, ws.data_ptr(), need, rows.data_ptr(),
                                                plane.data_ptr(), s.cuda_stream), "nbc_softmax_census")
    torch.cuda.synchronize()
    for rows, plane, _, _, _, _, order in outs:
        for pos, i in enumerate(order):
            assert rows[pos].cpu().numpy().tobytes() == alone[i][0][0].tobytes()
            assert plane[pos].cpu().numpy().tobytes() == alone[i][1][0].tobytes()


def _model(sd_np, precision="fp32"):
    from neuralbarkcalculator_amd.model import FCNResNet50
    return FCNResNet50(precision).load_state_dict(sd_np).to(DEV)


def test_model_method_validates_and_reuses_its_workspace(sd_np, built_lib):
    from neuralbarkcalculator_amd.model import deeplabv3_resnet50
    m = _model(sd_np)
    n, h, w = 2, 203, 317
    logits, grey, with_t, without = cc.case(n, h, w)
    L, G = _dev(logits), _dev(grey)
    rows, plane = m.softmax_census(L, G, confidence=True)
    torch.cuda.synchronize()
    assert rows.dtype == torch.uint64 and tuple(rows.shape) == (n, cal.WORDS) and plane.dtype == torch.uint8
    assert np.array_equal(rows.cpu().numpy(), with_t[0]) and np.array_equal(plane.cpu().numpy(), with_t[1])
    ws = m._census_ws
    rows1, none = m.softmax_census(L[:1].contiguous())                    # smaller, no target, no plane: the cached workspace
    torch.cuda.synchronize()
    assert m._census_ws is ws and none is None and np.array_equal(rows1.cpu().numpy(), without[0][:1])
    for bad in ((L.double(), G), (L, G.long()), (L[:, :2], G), (L, G[:, :-1]), (L.cpu(), G.cpu()), (L[..., :-1], G[..., :-1]),
                (L[..., :-1], None), (L.double(), None), (L[:0], None)):
        with pytest.raises(ValueError):
            m.softmax_census(*bad)
    dl = deeplabv3_resnet50(precision="fp32")                             # every architecture's class has the method
    assert type(dl).softmax_census is type(m).softmax_census


# ---- the two drivers end to end -----------------------------------------------------------------------------------------
LAYOUT = [("epinette_gelee", "a.png", 91, 128, 128), ("epinette_gelee", "b.png", 92, 96, 128), ("sapin", "c.png", 93, 128, 128),
          ("sapin", "d.png", 94, 96, 128), ("sapin", "e.png", 95, 128, 128)]
FOLDER_MARGIN = 1e-9      # on the forward's own logits the inputs are not chosen: the equality below needs the margin, so it is asserted


def _make_folder(root, ckpt_sd):
    rng = np.random.default_rng(79)
    truth = {}
    for wood, name, idx, h, w in LAYOUT:
        for sub in ("samples", "duals"):
            os.makedirs(os.path.join(root, sub, wood), exist_ok=True)
        img = synth.make_frame(idx, h, w)
        Image.fromarray(img, mode="RGB").save(os.path.join(root, "samples", wood, name))
        grey = np.array([20, 128, 230], np.uint8)[rng.integers(0, 3, size=(h, w))]
        Image.fromarray(grey, mode="L").save(os.path.join(root, "duals", wood, name))
        truth[(wood, name)] = (img, grey)
    ckpt = os.path.join(root, "best_model.pt")
    torch.save({k: torch.from_numpy(v) for k, v in ckpt_sd.items()}, ckpt)
    return ckpt, truth


@pytest.fixture(scope="module")
def folder(tmp_path_factory, sd_np):
    root = str(tmp_path_factory.mktemp("calibration_folder"))
    return (root,) + _make_folder(root, sd_np)


def _read(path):
    with open(path, "rb") as f:
        return f.read()


def _tsv(path):
    return list(csv.reader(open(path), delimiter="\t"))


def _forward(m, img, tta=0):
    """(logits f32 [1,3,H,W] numpy, raw labels [H,W] numpy) of one frame, as the drivers' forward computes them."""
    x = torch.from_numpy(np.array(img)[None]).to(DEV)
    lg = torch.empty((1, 3) + img.shape[:2], dtype=torch.float32, device=DEV)
    if tta:
        labels = m.predict_labels_tta(x, tta, labels_dtype=torch.uint8, logits_full=lg)[0]
    else:
        labels = m.predict_labels(x, labels_dtype=torch.uint8, logits_full=lg)[0]
    torch.cuda.synchronize()
    return lg.cpu().numpy(), labels[0].cpu().numpy()


@pytest.mark.parametrize("tta", ["none", "hflip"])
def test_evaluate_calibration_end_to_end(folder, sd_np, tta):
    root, ckpt, truth = folder
    res = os.path.join(root, "results")
    kw = dict(precision="fp32", device_index=0, **({} if tta == "none" else dict(tta=tta)))
    for name in (ev.CALIBRATION_CSV, ev.CURVES_CSV):                     # the other case of this test may have left them
        if os.path.exists(os.path.join(res, name)):
            os.remove(os.path.join(res, name))
    ev.evaluate_folder(root, ckpt, **kw)
    stats_plain, summary_plain = _read(os.path.join(root, ev.STATS_CSV)), json.load(open(os.path.join(root, ev.SUMMARY_JSON)))
    assert not os.path.exists(os.path.join(res, ev.CALIBRATION_CSV)) and not os.path.exists(os.path.join(res, ev.CURVES_CSV))
    assert "calibration" not in summary_plain
    stats = ev.evaluate_folder(root, ckpt, calibration=True, **kw)
    assert _read(os.path.join(root, ev.STATS_CSV)) == stats_plain
    summary = json.load(open(os.path.join(root, ev.SUMMARY_JSON)))
    assert {k: v for k, v in summary.items() if k != "calibration"} == summary_plain and "calibration" in summary

    m = _model(sd_np)
    mask = 0 if tta == "none" else ev.folder_run.check_tta_arguments(tta)
    want, host_rows, conf_total = [list(cal.CALIBRATION_COLUMNS)], [], np.zeros((3, 3), np.int64)
    for g in stats["rows"]:
        item = ev.list_labelled(root)[g[0]]
        img, grey = truth[(item["wood"], item["name"])]
        logits, labels = _forward(m, img, mask)
        rows, _, margin = cal.census_cpu(logits, grey[None])
        assert margin > FOLDER_MARGIN, (item["name"], margin)
        host_rows.append(rows[0])
        hard = np.bincount(labels.ravel(), minlength=3)
        assert hard.tolist() == np.array(g[4:13]).reshape(3, 3).sum(axis=0).tolist()
        conf_total += np.array(g[4:13]).reshape(3, 3)
        want += cal.calibration_rows(item["name"], item["wood"], cal.figures(rows[0], 16), hard)
    assert _tsv(os.path.join(res, ev.CALIBRATION_CSV)) == want and len(want) == 1 + len(LAYOUT)
    pooled = cal.pool(np.stack(host_rows))
    assert _tsv(os.path.join(res, ev.CURVES_CSV)) == [list(cal.CURVE_COLUMNS)] + cal.curve_rows(pooled)
    assert summary["calibration"] == json.loads(json.dumps(cal.calibration_summary(pooled, len(LAYOUT), 16, conf_total)))
    assert summary["calibration"]["pooled"]["pixels"] == sum(h * w for _, _, _, h, w in LAYOUT)
    assert "calibration over 16 bins" in ev.format_summary(summary)
    if tta == "none":                                 # another bin count moves ECE and MCE and nothing else; --ce shares the logits
        ev.evaluate_folder(root, ckpt, calibration=True, ece_bins=64, ce=True, **kw)
        got = _tsv(os.path.join(res, ev.CALIBRATION_CSV))
        assert [r[:2] + r[4:] for r in got] == [r[:2] + r[4:] for r in want]
        assert [r[2] for r in got[1:]] == ["{:.6f}".format(cal.figures(r, 64)["ece"]) for r in host_rows]
        assert _tsv(os.path.join(res, ev.CURVES_CSV)) == [list(cal.CURVE_COLUMNS)] + cal.curve_rows(pooled)
        assert [r[:15] for r in _tsv(os.path.join(root, ev.STATS_CSV))] == list(csv.reader(stats_plain.decode().splitlines(), delimiter="\t"))


def test_predict_confidence_end_to_end(tmp_path, sd_np):
    roots = {}
    for tag in ("plain", "conf"):
        roots[tag] = str(tmp_path / tag)
        ckpt, truth = _make_folder(roots[tag], sd_np)
    kw = dict(precision="fp32", device_index=0, calibrate=False)
    pr.predict_folder(roots["plain"], os.path.join(roots["plain"], "best_model.pt"), **kw)
    assert not os.path.exists(os.path.join(roots["plain"], "results", "confidence"))
    assert not os.path.exists(os.path.join(roots["plain"], "results", "confidence_stats.csv"))
    pr.predict_folder(roots["conf"], os.path.join(roots["conf"], "best_model.pt"), confidence=True, **kw)
    res = {tag: os.path.join(roots[tag], "results") for tag in roots}
    assert _read(os.path.join(res["conf"], "final_stats.csv")) == _read(os.path.join(res["plain"], "final_stats.csv"))
    m = _model(sd_np)
    want, host_rows, hard_total = [list(cal.CONFIDENCE_COLUMNS)], [], np.zeros(3, np.int64)
    for path, name, wood in pr.list_images(roots["conf"]):
        label = _read(os.path.join(res["conf"], "outputs", wood, name))
        assert label == _read(os.path.join(res["plain"], "outputs", wood, name))
        img = np.asarray(Image.open(os.path.join(roots["conf"], "processed", "samples", wood, name)).convert("RGB"))
        logits, _ = _forward(m, img)
        rows, plane, margin = cal.census_cpu(logits)
        assert margin > FOLDER_MARGIN, (name, margin)
        got = np.asarray(Image.open(os.path.join(res["conf"], "confidence", wood, name)))
        assert got.dtype == np.uint8 and np.array_equal(got, plane[0]) and got.min() >= 85       # the winner holds at least a third
        png = np.asarray(Image.open(os.path.join(res["conf"], "outputs", wood, name)))
        hard = np.array([(png == 0).sum(), (png == 127).sum(), (png == 255).sum()])
        hard_total += hard
        host_rows.append(rows[0])
        want += cal.confidence_rows(name, wood, rows[0], hard, 0.9)
    assert _tsv(os.path.join(res["conf"], "confidence_stats.csv")) == want and len(want) == 1 + len(LAYOUT)
    doc = json.load(open(os.path.join(res["conf"], "confidence_summary.json")))
    ref = cal.confidence_summary(cal.pool(np.stack(host_rows)), len(LAYOUT), 0.9, hard_total)
    assert {k: v for k, v in doc.items() if k not in ("precision", "bn_statistics")} == json.loads(json.dumps(ref))
    assert doc["precision"] == "fp32" and doc["confidence_threshold"] == 0.9
    with pytest.raises(ValueError):
        pr.predict_folder(roots["conf"], os.path.join(roots["conf"], "best_model.pt"), confidence=True, dropout_draws=2, **kw)
