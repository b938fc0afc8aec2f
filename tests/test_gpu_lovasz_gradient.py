"""nbc_lovasz_gradient on the GPU (include/nbc.h): the terms against nbc_lovasz_softmax bit for bit, the pixel
gradient and the low-resolution gradient against the float64 restatements of neuralbarkcalculator_amd/refit.py fed the device's
own keys, ties, absent classes, a non-finite image, batch and stream independence, the model's chain and the driver end to end
on ``--loss lovasz`` and ``--loss mixed``."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
from PIL import Image

from neuralbarkcalculator_amd import _lib, metrics, refit, synth
from neuralbarkcalculator_amd import evaluate as ev
from neuralbarkcalculator_amd import model as mdl
from neuralbarkcalculator_amd.model import FCNResNet50
from neuralbarkcalculator_amd.topology import out_hw

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
from lovasz_gradient_cases import quantised_image, saturated_image  # noqa: E402

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = torch.device("cuda", 0)
# tests/test_gpu_refit.py's bound on a device / float64 pair that differ by the order of their roundings, restated: relative to
# the sum of the absolute values of an element's terms, plus an absolute part per term
SUM_RTOL, SUM_ATOL_PER_TERM = 1e-9, 1e-12
WEIGHTS = (0.40, 2.03, 93.2)
# (H, W, h, w): the smallest; small; P = 8192, exactly one sort tile; P = 8193, one key into the second tile; two tiles; eight
SHAPES = [(1, 1, 1, 1), (8, 8, 1, 1), (64, 128, 8, 16), (3, 2731, 1, 342), (97, 131, 13, 17), (203, 317, 26, 40)]
TILE = 8192


def _bits(t) -> bytes:
    return (t.detach().cpu().contiguous().numpy() if isinstance(t, torch.Tensor) else np.ascontiguousarray(t)).tobytes()


def _batch(H, W, seed, n=3):
    """n images of different content: random logits of growing spread, grey levels over the whole range."""
    rng = np.random.default_rng(seed)
    logits = np.stack([(rng.normal(size=(3, H, W)) * (1.0 + 2.0 * i)).astype(np.float32) for i in range(n)])
    grey = rng.integers(0, 256, size=(n, H, W), dtype=np.uint8)
    return logits, grey


_TAPS = {}


def _tables(n_in, n_out):
    if (n_in, n_out) not in _TAPS:
        host = mdl.bicubic_taps(n_in, n_out)
        _TAPS[(n_in, n_out)] = (host, tuple(torch.from_numpy(a).to(DEV) for a in host))
    return _TAPS[(n_in, n_out)]


def _gradient(lib, logits, grey, h, w, table=None, lam=1.0, stream=None):
    """One nbc_lovasz_gradient call on numpy inputs with both optional outputs and guard words around grad_lowres: a dict of numpy
    arrays (terms, fg, low, keys, pix)."""
    n, _, H, W = logits.shape
    L, G = torch.from_numpy(np.ascontiguousarray(logits)).to(DEV), torch.from_numpy(np.ascontiguousarray(grey)).to(DEV)
    (_, rows), (_, cols) = _tables(h, H), _tables(w, W)
    need = lib.nbc_lovasz_gradient_workspace_bytes(n, H, W, h, w)
    assert need > 0
    ws = torch.empty(need, dtype=torch.uint8, device=DEV)
    guard = 4
    out = torch.full((n * 3 * h * w + 2 * guard,), 1234.5, dtype=torch.float64, device=DEV)
    terms = torch.empty((n, 3), dtype=torch.float64, device=DEV)
    fg = torch.empty((n, 3), dtype=torch.int64, device=DEV)
    keys = torch.full((n, 3, H, W), -1, dtype=torch.int32, device=DEV)
    pix = torch.full((n, 3, H, W), 1234.5, dtype=torch.float64, device=DEV)
    tab = None if table is None else np.ascontiguousarray(np.asarray(table, dtype=np.float64).reshape(-1))
    s = stream if stream is not None else torch.cuda.current_stream(DEV)
    torch.cuda.synchronize()
    _lib.check(lib.nbc_lovasz_gradient(L.data_ptr(), G.data_ptr(), n, H, W, h, w, *[t.data_ptr() for t in rows + cols],
                                       None if tab is None else tab.ctypes.data_as(C.POINTER(C.c_double)), float(lam), ws.data_ptr(),
                                       need, terms.data_ptr(), fg.data_ptr(), out.data_ptr() + 8 * guard, keys.data_ptr(),
                                       pix.data_ptr(), s.cuda_stream), "nbc_lovasz_gradient")
    s.synchronize()
    t = out.cpu().numpy()
    assert (t[:guard] == 1234.5).all() and (t[-guard:] == 1234.5).all()
    return dict(terms=terms.cpu().numpy(), fg=fg.cpu().numpy(), low=t[guard:-guard].reshape(n, 3, h, w), keys=keys.cpu().numpy(),
                pix=pix.cpu().numpy())


def _lovasz_softmax(lib, logits, grey):
    n, _, H, W = logits.shape
    L, G = torch.from_numpy(np.ascontiguousarray(logits)).to(DEV), torch.from_numpy(np.ascontiguousarray(grey)).to(DEV)
    need = lib.nbc_lovasz_workspace_bytes(n, H, W)
    ws = torch.empty(need, dtype=torch.uint8, device=DEV)
    terms = torch.empty((n, 3), dtype=torch.float64, device=DEV)
    fg = torch.empty((n, 3), dtype=torch.int64, device=DEV)
    s = torch.cuda.current_stream(DEV)
    _lib.check(lib.nbc_lovasz_softmax(L.data_ptr(), G.data_ptr(), n, H, W, ws.data_ptr(), need, terms.data_ptr(), fg.data_ptr(),
                                      s.cuda_stream), "nbc_lovasz_softmax")
    s.synchronize()
    return terms.cpu().numpy(), fg.cpu().numpy()


def _ce_gradient(lib, logits, grey, h, w, table):
    n, _, H, W = logits.shape
    L, G = torch.from_numpy(np.ascontiguousarray(logits)).to(DEV), torch.from_numpy(np.ascontiguousarray(grey)).to(DEV)
    (_, rows), (_, cols) = _tables(h, H), _tables(w, W)
    need = lib.nbc_ce_gradient_workspace_bytes(n, H, W, h, w)
    ws = torch.empty(need, dtype=torch.uint8, device=DEV)
    out = torch.empty((n, 3, h, w), dtype=torch.float64, device=DEV)
    tab = np.ascontiguousarray(np.asarray(table, dtype=np.float64).reshape(-1))
    s = torch.cuda.current_stream(DEV)
    _lib.check(lib.nbc_ce_gradient(L.data_ptr(), G.data_ptr(), n, H, W, h, w, *[t.data_ptr() for t in rows + cols],
                                   tab.ctypes.data_as(C.POINTER(C.c_double)), ws.data_ptr(), need, out.data_ptr(), s.cuda_stream),
               "nbc_ce_gradient")
    s.synchronize()
    return out.cpu().numpy()


def _check_keys(keys, grey):
    """The exported keys: the fg bit is (class == c) for every pixel, the decoded e lies in [0, 1]."""
    t = metrics.target_classes(grey)
    for c in range(3):
        e, fg = refit._decode_keys(keys[c])
        assert np.array_equal(fg, t == c)
        assert e.dtype == np.float32 and (e >= 0).all() and (e <= 1).all()


def _check_against_restatement(got, logits, grey, h, w, table, lam, what):
    """Tests 6 and 7 for every image of a call: every element of the pixel gradient and of grad_lowres within its bound of the
    restatement fed the device's keys.  Returns the worst ratio to the bound."""
    H, W = grey.shape[1:]
    taps = (_tables(h, H)[0], _tables(w, W)[0])
    worst = 0.0
    for i in range(len(logits)):
        want, mag, terms = refit.lovasz_pixel_gradient_cpu(logits[i], grey[i], got["keys"][i], table, lam, return_abs=True)
        ratio = np.abs(got["pix"][i] - want) / (SUM_RTOL * mag + SUM_ATOL_PER_TERM * terms)
        assert ratio.shape == (3, H, W) and np.all(ratio <= 1.0), (what, "pixel", i, float(ratio.max()))
        low, lmag, lterms = refit.lovasz_gradient_cpu(logits[i], grey[i], h, w, got["keys"][i], table, lam, taps, return_abs=True)
        lratio = np.abs(got["low"][i] - low) / (SUM_RTOL * lmag + SUM_ATOL_PER_TERM * lterms)
        assert lratio.shape == (3, h, w) and np.all(lratio <= 1.0), (what, "lowres", i, float(lratio.max()))
        worst = max(worst, float(ratio.max()), float(lratio.max()))
    return worst


@pytest.mark.parametrize("shape", SHAPES)
def test_terms_pixel_gradient_and_lowres_gradient(built_lib, shape):
    H, W, h, w = shape
    logits, grey = _batch(H, W, seed=H * 131 + W)
    T = refit.table_of("weighted_ce", WEIGHTS)
    want_terms, want_fg = _lovasz_softmax(built_lib, logits, grey)
    worst = {}
    for name, table, lam in (("lovasz", None, 1.0), ("table", T, 0.0), ("mixed", T / (4.0 * H * W), 1.0)):
        got = _gradient(built_lib, logits, grey, h, w, table, lam)
        assert _bits(got["terms"]) == _bits(want_terms) and _bits(got["fg"]) == _bits(want_fg), (shape, name)
        for i in range(len(logits)):
            _check_keys(got["keys"][i], grey[i])
        worst[name] = _check_against_restatement(got, logits, grey, h, w, table, lam, (shape, name))
        if name == "table":                             # the Lovasz term off: nbc_ce_gradient's numbers
            assert _bits(got["low"]) == _bits(_ce_gradient(built_lib, logits, grey, h, w, T)), shape
        else:
            assert np.isfinite(got["pix"]).all() and (H * W == 1 or np.abs(got["pix"]).max() > 0)
    print("%s: worst |device - float64| of its bound: %s" % (shape, ", ".join("%s %.3g" % kv for kv in worst.items())))
    assert (H * W + TILE - 1) // TILE == {1: 1, 64: 1, 8192: 1, 8193: 2, 97 * 131: 2, 203 * 317: 8}[H * W]


def test_ties_on_the_device(built_lib):
    worst = 0.0
    for make in (quantised_image, saturated_image):
        lg, gr = make()
        H, W = gr.shape
        got = _gradient(built_lib, lg[None], gr[None], 3, 5)
        e, _ = refit._decode_keys(got["keys"][0])
        assert all(np.unique(e[c]).size < e[c].size for c in range(3))              # the image does tie
        if make is saturated_image:
            assert set(np.unique(e).tolist()) == {0.0, 1.0}
        worst = max(worst, _check_against_restatement(got, lg[None], gr[None], 3, 5, None, 1.0, make.__name__))
        # a pixel-permuted copy: the same numbers, permuted, bit for bit (three images in one call: the original and two copies)
        rng = np.random.default_rng(2)
        perms = [np.arange(H * W), rng.permutation(H * W), np.arange(H * W)[::-1]]
        lgs = np.stack([lg.reshape(3, -1)[:, p].reshape(3, H, W) for p in perms])
        grs = np.stack([gr.ravel()[p].reshape(H, W) for p in perms])
        got3 = _gradient(built_lib, lgs, grs, 3, 5, refit.table_of("weighted_ce", WEIGHTS) / (4.0 * H * W), 1.0)
        assert _bits(got3["terms"][0]) == _bits(got3["terms"][1]) == _bits(got3["terms"][2])
        for k, p in enumerate(perms):
            assert _bits(got3["pix"][k].reshape(3, -1)) == _bits(got3["pix"][0].reshape(3, -1)[:, p]), (make.__name__, k)
            assert _bits(got3["keys"][k].reshape(3, -1)) == _bits(got3["keys"][0].reshape(3, -1)[:, p])
    print("ties: worst |device - float64| %.3g of its bound" % worst)


def test_absent_and_single_classes(built_lib):
    H, W, h, w = 40, 52, 5, 7
    logits, grey = _batch(H, W, seed=17)
    rng = np.random.default_rng(18)
    grey[0] = rng.choice(np.array([5, 120], np.uint8), size=(H, W))                  # class 2 absent
    grey[1] = 130                                                                    # class 1 on every pixel
    got = _gradient(built_lib, logits, grey, h, w)
    assert got["fg"].tolist()[0][2] == 0 and got["fg"].tolist()[1] == [0, H * W, 0] and (got["fg"][2] > 0).all()
    assert got["terms"][0][2] == 0 and got["terms"][1][0] == 0 and got["terms"][1][2] == 0
    for key in ("terms", "low", "pix"):
        assert np.isfinite(got[key]).all(), key
    worst = _check_against_restatement(got, logits, grey, h, w, None, 1.0, "absent")
    # C_p and the absent classes' zero stated here, not taken from the restatement: d of an absent class is 0, the slopes of the
    # present ones are divided by their number.  Both sides are float64 with a handful of roundings on numbers below 1: 1e-9
    # relative, and 1e-15 absolute where d - sum d q cancels.
    for i, present in ((0, [0, 1]), (1, [1]), (2, [0, 1, 2])):
        x = logits[i].astype(np.float64)
        q = np.exp(x - x.max(axis=0))
        q /= q.sum(axis=0)
        e, fg = refit._decode_keys(got["keys"][i].reshape(3, -1))
        d = np.zeros((3, H * W))
        for c in present:
            d[c] = np.where(fg[c], -1.0, 1.0) * refit.lovasz_slopes_cpu(e[c], fg[c]) / len(present)
        d = d.reshape(q.shape)
        want = q * (d - (d * q).sum(axis=0))
        assert np.allclose(got["pix"][i], want, rtol=1e-9, atol=1e-15), i
    print("absent classes: worst |device - float64| %.3g of its bound" % worst)


def test_a_non_finite_image_is_nan_and_alone(built_lib):
    H, W, h, w = 97, 131, 13, 17
    logits, grey = _batch(H, W, seed=23)
    solo = [_gradient(built_lib, logits[i:i + 1], grey[i:i + 1], h, w) for i in (0, 2)]
    logits[1, 2, 50, 60] = np.nan
    got = _gradient(built_lib, logits, grey, h, w)
    assert np.isnan(got["terms"][1]).all() and np.isnan(got["low"][1]).all() and np.isnan(got["pix"][1]).all()
    for pos, alone in zip((0, 2), solo):
        for key in ("terms", "fg", "low", "keys", "pix"):
            assert _bits(got[key][pos]) == _bits(alone[key][0]), (pos, key)
        assert np.isfinite(got["low"][pos]).all()
    # with a table beside it, too
    both = _gradient(built_lib, logits, grey, h, w, refit.table_of("weighted_ce", WEIGHTS) / (4.0 * H * W), 1.0)
    assert np.isnan(both["low"][1]).all() and np.isfinite(both["low"][[0, 2]]).all()


def test_batch_and_stream_independence(built_lib):
    H, W, h, w = 203, 317, 26, 40
    logits, grey = _batch(H, W, seed=29)
    T = refit.table_of("weighted_ce", WEIGHTS) / (4.0 * H * W)
    keys = ("terms", "fg", "low", "keys", "pix")
    alone = [_gradient(built_lib, logits[i:i + 1], grey[i:i + 1], h, w, T, 1.0) for i in range(3)]
    for order in ([0, 1, 2], [2, 0, 1], [1, 2]):
        got = _gradient(built_lib, logits[order], grey[order], h, w, T, 1.0)
        for pos, i in enumerate(order):
            for key in keys:
                assert _bits(got[key][pos]) == _bits(alone[i][key][0]), (order, pos, key)
    side = torch.cuda.Stream(DEV)
    got = _gradient(built_lib, logits[[1, 2, 0]], grey[[1, 2, 0]], h, w, T, 1.0, stream=side)
    for pos, i in enumerate([1, 2, 0]):
        for key in keys:
            assert _bits(got[key][pos]) == _bits(alone[i][key][0]), (pos, key)


# ---- the model ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", ["fp32", "f16x2"])
def test_model_chain(sd_np, built_lib, precision):
    H, W = 64, 96
    m = FCNResNet50(precision).load_state_dict(sd_np).to(DEV)
    theta0 = refit.theta_of(sd_np)
    n = 2
    x = torch.from_numpy(np.stack([synth.make_input(i, H, W) for i in (40, 41)])).to(DEV)
    tgt = torch.from_numpy(np.random.default_rng(3).integers(0, 256, size=(n, H, W), dtype=np.uint8)).to(DEV)
    lg = torch.empty((n, 3, H, W), dtype=torch.float32, device=DEV)
    m.predict_labels(x, labels_dtype=torch.uint8, logits_full=lg)
    want_terms, want_fg = m.lovasz_softmax(lg, tgt)
    T = refit.table_of("weighted_ce", WEIGHTS)
    old = m.head_loss_and_gradient(tgt, theta0, T)
    assert len(old) == 3
    for table, lam in ((None, 1.0), (T / (4.0 * H * W), 1.0)):
        sums, counts, grad, terms, fg = m.head_loss_and_gradient(tgt, theta0, table, lovasz_weight=lam)
        torch.cuda.synchronize()
        assert _bits(terms) == _bits(want_terms) and _bits(fg) == _bits(want_fg)
        assert _bits(sums) == _bits(old[0]) and _bits(counts) == _bits(old[1])
        assert grad.shape == (n, 3, 513) and grad.dtype == torch.float64 and bool(torch.isfinite(grad).all())
        bias = grad[:, :, 512].cpu().numpy()
        assert np.abs(bias).sum() > 0 and np.all(np.abs(bias.sum(axis=1)) <= 1e-9 * np.abs(bias).sum(axis=1))
    # lovasz_gradient alone, with its optional outputs
    out = m.lovasz_gradient(lg, tgt, out_hw(H, W), return_keys=True, return_pixel_gradient=True)
    assert len(out) == 5 and out[3].dtype == torch.int32 and tuple(out[3].shape) == tuple(out[4].shape) == (n, 3, H, W)
    assert _bits(out[0]) == _bits(want_terms) and bool((out[3] >= 0).all())
    assert len(m.lovasz_gradient(lg, tgt, out_hw(H, W))) == 3


# ---- the driver ---------------------------------------------------------------------------------------------------------------------
ITEMS = [("epinette_gelee", "a.png", 91), ("epinette_gelee", "b.png", 92), ("sapin", "c.png", 93), ("sapin", "d.png", 94)]
SIZE = (64, 96)


@pytest.fixture(scope="module")
def folder(tmp_path_factory, sd_np, built_lib):
    """tests/test_gpu_refit.py's folder: four synthetic frames whose duals are the labels of a perturbed head."""
    root = str(tmp_path_factory.mktemp("lovasz_refit_folder"))
    theta0 = refit.theta_of(sd_np)
    star = (theta0 + np.float32(0.02) * synth.normal(11, 3, 1539).astype(np.float32)).astype(np.float32)
    teacher = FCNResNet50("fp32").load_state_dict(refit.replace_head(sd_np, star)).to(DEV)
    for wood, name, idx in ITEMS:
        for sub in ("samples", "duals"):
            os.makedirs(os.path.join(root, sub, wood), exist_ok=True)
        img = synth.make_frame(idx, *SIZE)
        Image.fromarray(img, mode="RGB").save(os.path.join(root, "samples", wood, name))
        labels, _ = teacher.predict_labels(torch.from_numpy(img[None]).to(DEV), labels_dtype=torch.uint8)
        Image.fromarray(np.array([20, 128, 230], np.uint8)[labels[0].cpu().numpy()], mode="L").save(os.path.join(root, "duals", wood, name))
    ckpt = os.path.join(root, "best_model.pt")
    torch.save({k: torch.from_numpy(v) for k, v in sd_np.items()}, ckpt)
    st = ev.evaluate_folder(root, ckpt, precision="fp32", device_index=0, target_size=128, loss=True)
    return dict(root=root, ckpt=ckpt, lovasz_before=st["summary"]["lovasz_softmax"]["mean_over_images"])


def _files(root):
    return open(os.path.join(root, refit.LOG_CSV), "rb").read(), open(os.path.join(root, refit.SUMMARY_JSON), "rb").read()


@pytest.mark.parametrize("loss", ["lovasz", "mixed"])
def test_driver_end_to_end(folder, sd_np, loss, tmp_path):
    out = str(tmp_path / ("refit_%s.pt" % loss))
    st = refit.refit_folder(folder["root"], out, folder["ckpt"], image_loss=loss, iterations=5, precision="fp32", device_index=0, target_size=128)
    log, raw = _files(folder["root"])
    summary = json.loads(raw)
    rows = [r.split("\t") for r in log.decode().splitlines()]
    assert rows[0] == refit.LOG_HEADER and 1 <= len(rows) - 1 <= 2 * 5 + 2
    assert st["summary"] == summary and summary["loss"] == loss and summary["images"] == len(ITEMS) and summary["skipped"] == 0
    objectives = [float(r[1]) for r in rows[1:]]
    assert summary["objective"]["before"] == objectives[0] and summary["objective"]["after"] == min(objectives) <= objectives[0]
    print("%s: objective %.6g -> %.6g in %d evaluations (%s)" % (loss, objectives[0], min(objectives), len(objectives),
                                                                  summary["optimizer_message"]))
    assert abs(summary["lovasz_softmax"]["before"] - folder["lovasz_before"]) <= 1e-12
    assert 0 < summary["lovasz_softmax"]["after"] < 1
    if loss == "mixed":
        assert summary["data_term"]["before"] == summary["mixed_loss"]["before"] > summary["lovasz_softmax"]["before"]
        assert summary["table"] == refit.table_of("weighted_ce").tolist()
    else:
        assert "mixed_loss" not in summary and summary["data_term"]["before"] == summary["lovasz_softmax"]["before"]
    back = torch.load(out, map_location="cpu", weights_only=True)
    assert list(back) == list(sd_np)
    for k, v in sd_np.items():
        assert back[k].dtype == torch.from_numpy(v).dtype and tuple(back[k].shape) == v.shape
        if k not in (refit.W_KEY, refit.B_KEY):
            assert torch.equal(back[k], torch.from_numpy(v)), k
    # two ranks over gloo on one GPU write the same bytes as one
    out2 = str(tmp_path / "two_ranks.pt")
    code = ("import sys, torch.distributed as dist\n"
            "sys.path.insert(0, %r)\n"
            "from neuralbarkcalculator_amd import refit\n"
            "dist.init_process_group('gloo')\n"
            "st = refit.refit_folder(%r, %r, %r, image_loss=%r, iterations=5, precision='fp32', device_index=0, target_size=128)\n"
            "assert st['world'] == 2 and (st['summary'] is not None) == (st['rank'] == 0)\n"
            "dist.destroy_process_group()\n" % (REPO, folder["root"], out2, folder["ckpt"], loss))
    script = tmp_path / "run2.py"
    script.write_text(code)
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0", OMP_NUM_THREADS="1")
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK"):
        env.pop(k, None)
    p = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
                        "--master-port", "29713" if loss == "lovasz" else "29714", str(script)],
                       cwd=REPO, env=env, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-3000:]
    log2, raw2 = _files(folder["root"])
    two = json.loads(raw2)
    assert log2 == log and two.pop("ranks") == 2 and two.pop("out") == out2
    one = dict(summary)
    one.pop("ranks"), one.pop("out")
    assert two == one
    a, b = torch.load(out, map_location="cpu", weights_only=True), torch.load(out2, map_location="cpu", weights_only=True)
    assert list(a) == list(b) and all(torch.equal(a[k], b[k]) for k in a)


def test_the_ce_family_writes_what_it_wrote(folder, tmp_path):
    """A --loss ce run: its log is `objective` on today's rows -- one pass's rows, gathered by hand from the model's own calls
    without a lovasz_weight, give the first row of the log bit for bit -- and its summary has no key of the new losses."""
    out = str(tmp_path / "refit_ce.pt")
    refit.refit_folder(folder["root"], out, folder["ckpt"], loss="ce", iterations=2, precision="fp32", device_index=0, target_size=128)
    log, raw = _files(folder["root"])
    summary = json.loads(raw)
    assert set(summary) == {"loss", "table", "class_weights_source", "l2", "iterations", "evaluations", "optimizer_message", "stopped",
                            "images", "skipped", "objective", "data_term", "before", "after", "model_path", "out", "normalization",
                            "precision", "ranks"}
    sd = torch.load(folder["ckpt"], map_location="cpu", weights_only=True)
    m = FCNResNet50("fp32").load_state_dict({k: v.numpy() for k, v in sd.items()}).to(DEV)
    theta0 = refit.theta_of(sd)
    T = refit.table_of("ce")
    rows = []
    for d in ev.list_labelled(folder["root"]):
        img, grey = ev._decode_rgb(d["src"]), ev.decode_dual(d["dual"])
        m.lowres_logits(torch.from_numpy(img[None]).to(DEV))
        sums, counts, grad = m.head_loss_and_gradient(torch.from_numpy(grey[None]).to(DEV), theta0, T)
        rows.append((sums[0].cpu().numpy(), counts[0].cpu().numpy(), grad[0].cpu().numpy()))
    value, data, grad = refit.objective(rows, T, 0.0, theta0, theta0)
    first = log.decode().splitlines()[1].split("\t")
    assert first == ["1", repr(float(value)), repr(float(data)), repr(float(np.sqrt(grad @ grad))), "1"]
