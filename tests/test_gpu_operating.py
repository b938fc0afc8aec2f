"""nbc_offset_sweep on the GPU against its host restatement (operating.sweep_cpu), integer for integer; its batch and stream
independence; the logit offsets in the forward's own upsample + argmax launch (both kernel forms); `evaluate
--operating_points`, `evaluate --logit_offsets` and `predict --logit_offsets` end to end.

No tolerance anywhere: the definition is integer from the comparison on, and the host makes the same float32 additions."""
import csv
import json
import os
import sys

import numpy as np
import pytest
import torch
from PIL import Image

from neuralbarkcalculator_amd import _lib, metrics, synth
from neuralbarkcalculator_amd import evaluate as ev
from neuralbarkcalculator_amd import operating as op
from neuralbarkcalculator_amd import predict as pr

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import operating_cases as oc  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
GUARD, FILL = 9, -77                                # words on either side of the table


def _dev(a):
    return torch.from_numpy(np.array(a)).to(DEV)


def _floats(v):
    v = np.ascontiguousarray(v, dtype=np.float32)
    return v, v.ctypes.data_as(_lib.C.POINTER(_lib.C.c_float))


def _run(lib, logits, grey, b1, b2, stream=None):
    """One nbc_offset_sweep call on device tensors, guard words around the output: int64 [n,G1,G2,3,3] as numpy."""
    n, _, h, w = logits.shape
    (k1, p1), (k2, p2) = _floats(b1), _floats(b2)
    need = lib.nbc_offset_sweep_workspace_bytes(n, h, w, k1.size, k2.size)
    ws = torch.empty(need, dtype=torch.uint8, device=DEV)
    words = n * k1.size * k2.size * 9
    out = torch.full((words + 2 * GUARD,), FILL, dtype=torch.int64, device=DEV)
    s = stream if stream is not None else torch.cuda.current_stream(DEV)
    _lib.check(lib.nbc_offset_sweep(logits.data_ptr(), grey.data_ptr(), n, h, w, p1, k1.size, p2, k2.size, ws.data_ptr(), need,
                                    out.data_ptr() + 8 * GUARD, s.cuda_stream), "nbc_offset_sweep")
    s.synchronize()
    r = out.cpu().numpy()
    assert (r[:GUARD] == FILL).all() and (r[-GUARD:] == FILL).all()
    return r[GUARD:-GUARD].reshape(n, k1.size, k2.size, 3, 3)


@pytest.mark.parametrize("grid", list(oc.GRIDS))
@pytest.mark.parametrize("shape", oc.SHAPES)
def test_tables_equal_the_host_sweep(built_lib, shape, grid):
    logits, grey = oc.inputs(*shape)
    want = oc.table(*shape, grid)
    got = _run(built_lib, _dev(logits), _dev(grey), *oc.GRIDS[grid])
    bad = np.argwhere(got != want)
    assert bad.size == 0, (shape, grid, bad[:8], got[tuple(bad[0])], want[tuple(bad[0])])
    assert (got.sum(axis=(3, 4)) == shape[1] * shape[2]).all()


def test_tables_of_unaligned_planes(built_lib):
    """Logits and target that start 4 and 1 bytes past a 16-byte boundary: the scalar loads, the same table."""
    n, h, w = 2, 33, 65
    logits, grey = oc.inputs(n, h, w)
    L = torch.empty(logits.size + 1, dtype=torch.float32, device=DEV)[1:].view(n, 3, h, w).copy_(_dev(logits))
    G = torch.empty(grey.size + 1, dtype=torch.uint8, device=DEV)[1:].view(n, h, w).copy_(_dev(grey))
    assert L.data_ptr() % 16 == 4 and G.data_ptr() % 4 == 1
    assert np.array_equal(_run(built_lib, L, G, *oc.GRIDS["uneven"]), oc.table(n, h, w, "uneven"))


def test_batch_and_stream_independence(built_lib):
    """An image's table is bit-identical alone, at each position of a batch of 3 (odd H * W: the images of a batch start at
    different alignments) and from two streams running at once."""
    n, h, w = 3, 67, 131
    logits, grey = oc.inputs(n, h, w)
    b1, b2 = oc.GRIDS["default"]
    L, G = _dev(logits), _dev(grey)
    alone = [_run(built_lib, L[i:i + 1].contiguous(), G[i:i + 1].contiguous(), b1, b2)[0] for i in range(n)]
    orders = [[0, 1, 2], [1, 2, 0], [2, 0, 1]]
    for order in orders:
        got = _run(built_lib, L[order].contiguous(), G[order].contiguous(), b1, b2)
        for pos, i in enumerate(order):
            assert got[pos].tobytes() == alone[i].tobytes(), (order, pos)
    (k1, p1), (k2, p2) = _floats(b1), _floats(b2)
    need = built_lib.nbc_offset_sweep_workspace_bytes(n, h, w, 33, 33)
    outs = [(torch.empty((n, 33, 33, 3, 3), dtype=torch.int64, device=DEV), torch.empty(need, dtype=torch.uint8, device=DEV),
             L[order].contiguous(), G[order].contiguous(), torch.cuda.Stream(DEV), order) for order in orders[:2]]
    torch.cuda.synchronize()
    for conf, ws, Ls, Gs, s, _ in outs:
        _lib.check(built_lib.nbc_offset_sweep(Ls.data_ptr(), Gs.data_ptr(), n, h, w, p1, 33, p2, 33, ws.data_ptr(), need, conf.data_ptr(),
                                              s.cuda_stream), "nbc_offset_sweep")
    torch.cuda.synchronize()
    for conf, _, _, _, _, order in outs:
        for pos, i in enumerate(order):
            assert conf[pos].cpu().numpy().tobytes() == alone[i].tobytes()


def _bare_model():
    from neuralbarkcalculator_amd.model import FCNResNet50
    return FCNResNet50("fp32").to(DEV)                            # a context without weights: the tail needs none


def _model(sd_np, precision="fp32"):
    from neuralbarkcalculator_amd.model import FCNResNet50
    return FCNResNet50(precision).load_state_dict(sd_np).to(DEV)


def _lowres(n, lh, lw, seed):
    """Low-resolution logits whose upsampled planes tie exactly: class 1's plane is class 0's in the left half, class 2's is
    class 0's in the upper half (equal inputs give equal bicubic sums), random elsewhere; one NaN, which the taps spread."""
    rng = np.random.default_rng(seed)
    low = (rng.standard_normal((n, 3, lh, lw)) * 3).astype(np.float32)
    low[:, 1, :, : lw // 2] = low[:, 0, :, : lw // 2]
    low[:, 2, : lh // 2] = low[:, 0, : lh // 2]
    low[0, 1, lh - 1, lw - 1] = np.nan
    return low


def test_origin_of_the_sweep_is_the_confusion_of_the_forwards_labels(built_lib):
    m = _bare_model()
    n, lh, lw, H, W = 2, 9, 17, 67, 131
    low = _dev(_lowres(n, lh, lw, 3))
    grey = _dev(oc.inputs(3, 67, 131)[1][:n])
    labels, counts, full = m.upsample_argmax(low, (H, W), labels_dtype=torch.uint8, return_logits=True)
    b1, b2 = oc.GRIDS["uneven"]                                   # (0, 0) is its point (2, 1)
    tables = m.offset_sweep(full, grey, b1, b2)
    conf = m.confusion(labels, grey)
    torch.cuda.synchronize()
    assert tables.dtype == torch.uint64 and tuple(tables.shape) == (n, 5, 3, 3, 3)
    t = tables.view(torch.int64).cpu().numpy()
    assert np.array_equal(t[:, 2, 1], conf.cpu().numpy())
    assert np.array_equal(t, op.sweep_cpu(full.cpu().numpy(), grey.cpu().numpy(), b1, b2))
    ws = m._sweep_ws                                             # the workspace is cached and re-used by a smaller call
    m.offset_sweep(full[:1].contiguous(), grey[:1].contiguous(), [0.0], [0.0])
    assert m._sweep_ws is ws
    for bad in ((full.double(), grey), (full, grey.long()), (full[:, :2], grey), (full, grey[:, :-1]), (full.cpu(), grey.cpu())):
        with pytest.raises(ValueError):
            m.offset_sweep(*bad, [0.0], [0.0])
    for lists in (([], [0.0]), ([0.0], list(range(34))), ([1.0, 0.0], [0.0]), ([0.0], [float("nan")])):
        with pytest.raises((ValueError, RuntimeError)):
            m.offset_sweep(full, grey, *lists)


# (lowres size, output size): x8 takes the tiled kernel, the others (a tap window wider than its LDS image) the
# one-pixel-per-thread kernel; 300 columns are more than one block wide, 67 rows are no multiple of the tile's 8
FORMS = {"tiled": ((9, 38), (67, 300)), "pixel": ((40, 50), (67, 60)), "identity": ((33, 65), (33, 65))}


@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("offsets", [(0.0, 1.5), (-2.0, 0.0), (0.75, -1.25)])
def test_offsets_move_the_decision_and_nothing_else(built_lib, form, offsets):
    (lh, lw), (H, W) = FORMS[form]
    n = 2
    low_np = _lowres(n, lh, lw, 11)
    if form == "identity":                                        # the taps are (0, 1, 0, 0): the logits are the input's,
        low_np[:, 1] = low_np[:, 0] - np.float32(offsets[0])      # so x1 + b1 == x0 exactly wherever the subtraction was
        low_np[:, 2, ::2] = low_np[:, 0, ::2] - np.float32(offsets[1])   # exact, x2 + b2 == x0 likewise on every other row
        low_np[0, 2, 5, 7] = np.nan
    low = _dev(low_np)
    plain = _bare_model()
    lab0, cnt0, full0 = plain.upsample_argmax(low, (H, W), labels_dtype=torch.uint8, return_logits=True)
    m = _bare_model().set_logit_offsets(*offsets)
    assert m.logit_offsets() == offsets
    lab, cnt, full = m.upsample_argmax(low, (H, W), labels_dtype=torch.uint8, return_logits=True)
    lab64, cnt64 = m.upsample_argmax(low, (H, W), labels_dtype=torch.int64)
    labx, cntx = m.upsample_argmax(low, (H, W), exclude_nodes=True, labels_dtype=torch.uint8)
    torch.cuda.synchronize()
    logits = full.cpu().numpy()
    assert logits.tobytes() == full0.cpu().numpy().tobytes()      # the logits are never offset
    want = op.decide_cpu(logits, *offsets)
    got = lab.cpu().numpy()
    assert np.array_equal(got, want) and np.array_equal(lab64.cpu().numpy(), want)
    assert (want != lab0.cpu().numpy()).any()                     # the decision did move
    x0, x1, x2 = logits[:, 0], logits[:, 1], logits[:, 2]
    with np.errstate(invalid="ignore"):
        ties = ((x1 + np.float32(offsets[0]) == x0) | (x2 + np.float32(offsets[1]) == x0)).sum()
    assert np.isnan(logits).any()                                 # a NaN was decided
    if form == "identity" or 0.0 in offsets:                      # and exact ties (equal planes tie under a zero offset only)
        assert ties > 50
    by_image = np.stack([np.bincount(w_.ravel(), minlength=3) for w_ in want])
    assert cnt.cpu().numpy().tolist() == by_image.tolist() == cnt64.cpu().numpy().tolist()
    remapped = np.where(want == 2, 1, want)                       # the remap follows the decision
    assert np.array_equal(labx.cpu().numpy(), remapped)
    assert cntx.cpu().numpy().tolist() == [[r[0], r[1] + r[2], 0] for r in by_image.tolist()]
    # the sweep's table at that point is the confusion of those labels
    grey = _dev(np.array([0, 128, 255], np.uint8)[np.random.default_rng(2).integers(0, 3, size=(n, H, W))])
    grid1, grid2 = sorted({0.0, offsets[0]}), sorted({0.0, offsets[1]})
    tables = m.offset_sweep(full, grey, grid1, grid2).view(torch.int64).cpu().numpy()
    conf = m.confusion(lab, grey).cpu().numpy()
    assert np.array_equal(tables[:, grid1.index(offsets[0]), grid2.index(offsets[1])], conf)
    assert np.array_equal(tables[:, grid1.index(0.0), grid2.index(0.0)], plain.confusion(lab0, grey).cpu().numpy())
    # (0, 0) is off: labels and counts byte-identical to a fresh model's
    m.set_logit_offsets(0, 0)
    lab1, cnt1 = m.upsample_argmax(low, (H, W), labels_dtype=torch.uint8)
    torch.cuda.synchronize()
    assert lab1.cpu().numpy().tobytes() == lab0.cpu().numpy().tobytes() and cnt1.cpu().tolist() == cnt0.cpu().tolist()


def test_forward_clone_and_dropout_with_offsets(sd_np, built_lib):
    offsets = (-0.5, 2.0)
    m = _model(sd_np)
    x = torch.from_numpy(np.stack([synth.make_input(5, 64, 64)])).to(DEV)
    full0 = torch.empty((1, 3, 64, 64), dtype=torch.float32, device=DEV)
    lab0, cnt0 = m.predict_labels(x, labels_dtype=torch.uint8, logits_full=full0)
    m.set_logit_offsets(*offsets)
    full = torch.empty_like(full0)
    lab, cnt = m.predict_labels(x, labels_dtype=torch.uint8, logits_full=full)
    torch.cuda.synchronize()
    logits = full.cpu().numpy()
    assert logits.tobytes() == full0.cpu().numpy().tobytes() and m(x).cpu().numpy().tobytes() == logits.tobytes()
    want = op.decide_cpu(logits, *offsets)
    assert np.array_equal(lab.cpu().numpy(), want) and cnt.cpu().tolist() == [np.bincount(want.ravel(), minlength=3).tolist()]
    assert np.array_equal(lab0.cpu().numpy(), op.decide_cpu(logits, 0.0, 0.0))
    clone = m.clone_shared()                                      # the drivers' per-stream models are clones
    assert clone.logit_offsets() == offsets
    labc, _ = clone.predict_labels(x, labels_dtype=torch.uint8)
    torch.cuda.synchronize()
    assert np.array_equal(labc.cpu().numpy(), want)
    for call in (m.dropout_draws, m.dropout_votes):
        with pytest.raises(RuntimeError, match="logit offsets"):
            call(2, [7])
    m.set_logit_offsets(0, 0)
    assert tuple(m.dropout_draws(2, [7]).shape) == (2, 1, 3)      # off again: the draws run
    ctx_nan = built_lib.nbc_set_logit_offsets(m._ctx, float("nan"), 0.0)
    assert ctx_nan == _lib.NBC_ERR_INVALID and m.logit_offsets() == (0.0, 0.0)


# ---- the two drivers end to end -----------------------------------------------------------------------------------------
LAYOUT = [("epinette_gelee", "a.png", 91, 128, 128), ("sapin", "b.png", 92, 96, 128), ("sapin", "c.png", 93, 128, 128)]
POINT = (14, 21)                                    # a point of the default grid other than (0, 0): bark -1.0, node +2.5


def _make_folder(root, ckpt_sd):
    rng = np.random.default_rng(83)
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


def _read(path):
    with open(path, "rb") as f:
        return f.read()


def _tsv(path):
    return list(csv.reader(open(path), delimiter="\t"))


def _logits(m, img):
    x = torch.from_numpy(np.array(img)[None]).to(DEV)
    lg = torch.empty((1, 3) + img.shape[:2], dtype=torch.float32, device=DEV)
    m.predict_labels(x, labels_dtype=torch.uint8, logits_full=lg)
    torch.cuda.synchronize()
    return lg.cpu().numpy()


def _tree(root):
    """{relative path: bytes} of every file under root."""
    out = {}
    for d, _, files in os.walk(root):
        for f in files:
            out[os.path.relpath(os.path.join(d, f), root)] = _read(os.path.join(d, f))
    return out


def test_evaluate_operating_points_end_to_end(tmp_path, sd_np):
    root = str(tmp_path / "labelled")
    ckpt, truth = _make_folder(root, sd_np)
    res = os.path.join(root, "results")
    kw = dict(precision="fp32", device_index=0, calibrate=False)
    ev.evaluate_folder(root, ckpt, **kw)
    before = _tree(root)
    assert not any(os.path.basename(k) in (op.POINTS_CSV, op.EVALUATION_CSV) for k in before)
    summary_plain = json.loads(before[ev.SUMMARY_JSON])
    assert "operating_points" not in summary_plain and "logit_offsets" not in summary_plain
    stats = ev.evaluate_folder(root, ckpt, operating_points=True, **kw)
    after = _tree(root)
    new = {os.path.join("results", op.POINTS_CSV), os.path.join("results", op.EVALUATION_CSV)}
    assert set(after) == set(before) | new
    for k in before:                                              # every other file byte for byte, but the summary's new entry
        if k != ev.SUMMARY_JSON:
            assert after[k] == before[k], k
    summary = json.loads(after[ev.SUMMARY_JSON])
    assert {k: v for k, v in summary.items() if k != "operating_points"} == summary_plain

    grid = op.parse_grid(op.DEFAULT_GRID)
    m = _model(sd_np)
    items = ev.list_labelled(root)
    images, raw_total = [], np.zeros((3, 3), np.int64)
    for g in stats["rows"]:
        item = items[g[0]]
        img, grey = truth[(item["wood"], item["name"])]
        table = op.sweep_cpu(_logits(m, img)[0], grey, grid, grid)
        assert np.array_equal(table[16, 16], np.array(g[4:13]).reshape(3, 3))       # the row's own raw confusion
        images.append((item["name"], item["wood"], table))
        raw_total += np.array(g[4:13]).reshape(3, 3)
    pooled = sum(t for _, _, t in images)
    entry = summary["operating_points"]
    assert entry == json.loads(json.dumps(op.summary_entry(pooled, grid, grid)))
    assert entry["points"]["argmax"]["confusion"] == raw_total.tolist() and set(entry["points"]) == set(op.POINT_NAMES)
    rows = _tsv(os.path.join(res, op.POINTS_CSV))
    assert rows[0] == op.POINTS_COLUMNS and len(rows) == 1 + 33 * 33
    for i in range(33):
        for j in range(33):
            assert rows[1 + i * 33 + j] == op.point_row(pooled[i, j], grid[i], grid[j]), (i, j)
    origin = rows[1 + 16 * 33 + 16]                               # the (0, 0) row is the summary's pooled raw IoU
    assert [float(v) for v in origin[2:6]] == [round(summary["pooled"][k], 6) for k in ("iou_nothing", "iou_bark", "iou_node", "iou_mean")]
    assert open(os.path.join(res, op.EVALUATION_CSV)).read() == _expected_evaluation_csv(tmp_path, images, entry["points"])
    assert "operating point best_miou: --logit_offsets" in ev.format_summary(summary)

    # the application: a second run at a grid point other than (0, 0) labels what the first run's table says
    i, j = POINT
    offsets = (float(grid[i]), float(grid[j]))
    stats2 = ev.evaluate_folder(root, ckpt, logit_offsets=offsets, **kw)
    raw2 = sum(np.array(g[4:13]).reshape(3, 3) for g in stats2["rows"])
    assert np.array_equal(raw2, pooled[i, j])
    for g in stats2["rows"]:
        assert np.array_equal(np.array(g[4:13]).reshape(3, 3), images[[it[0] for it in images].index(items[g[0]]["name"])][2][i, j])
    summary2 = json.load(open(os.path.join(root, ev.SUMMARY_JSON)))
    assert summary2["logit_offsets"] == list(offsets) and "operating_points" not in summary2
    # the sweep ignores the offsets the run decides with, and records them
    ev.evaluate_folder(root, ckpt, logit_offsets=offsets, operating_points=True, bark_offsets="-1:0:1", node_offsets=[0.0, 2.5], **kw)
    summary3 = json.load(open(os.path.join(root, ev.SUMMARY_JSON)))
    assert summary3["operating_points"]["run_logit_offsets"] == list(offsets)
    assert summary3["operating_points"]["points"]["argmax"]["confusion"] == raw_total.tolist()
    assert _tsv(os.path.join(res, op.POINTS_CSV))[1] == op.point_row(pooled[14, 16], -1.0, 0.0)
    assert _tsv(os.path.join(res, op.POINTS_CSV))[2] == op.point_row(pooled[14, 21], -1.0, 2.5)
    with pytest.raises(ValueError, match="needs --operating_points"):
        ev.evaluate_folder(root, ckpt, node_offsets="-1:1:1", **kw)


def _expected_evaluation_csv(tmp_path, images, points):
    path = str(tmp_path / "expected_operating_evaluation.csv")
    op.write_evaluation_csv(path, images, points)
    return open(path).read()


def test_predict_logit_offsets_end_to_end(tmp_path, sd_np):
    offsets = (-1.0, 2.5)
    roots = {}
    for tag in ("plain", "moved"):
        roots[tag] = str(tmp_path / tag)
        _make_folder(roots[tag], sd_np)
    kw = dict(precision="fp32", small_zones=False, device_index=0, calibrate=False)
    pr.predict_folder(roots["plain"], os.path.join(roots["plain"], "best_model.pt"), **kw)
    pr.predict_folder(roots["moved"], os.path.join(roots["moved"], "best_model.pt"), logit_offsets=offsets, **kw)
    res = {tag: os.path.join(roots[tag], "results") for tag in roots}
    m = _model(sd_np)
    grey_of = np.array([0, 127, 255], np.uint8)
    seen = 0
    for path, name, wood in pr.list_images(roots["moved"]):
        img = np.asarray(Image.open(os.path.join(roots["moved"], "processed", "samples", wood, name)).convert("RGB"))
        logits = _logits(m, img)
        png = {tag: np.asarray(Image.open(os.path.join(res[tag], "outputs", wood, name))) for tag in roots}
        assert np.array_equal(png["plain"], grey_of[op.decide_cpu(logits, 0.0, 0.0)[0]])
        assert np.array_equal(png["moved"], grey_of[op.decide_cpu(logits, *offsets)[0]])
        seen += 1
    assert seen == len(LAYOUT)
    for bad in (dict(dropout_draws=2), dict(confidence=True)):
        with pytest.raises(ValueError):
            pr.predict_folder(roots["moved"], os.path.join(roots["moved"], "best_model.pt"), logit_offsets=offsets, **dict(kw, **bad))
