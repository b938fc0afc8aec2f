"""nbc_lovasz_softmax on the GPU against the two host restatements of tests/helpers/lovasz_oracle.py, its batch and stream
independence, non-finite logits, and `evaluate --loss` end to end."""
import csv
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
from PIL import Image

from neuralbarkcalculator_amd import _lib, metrics, synth
from neuralbarkcalculator_amd import evaluate as ev

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import lovasz_oracle as lo  # noqa: E402

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = torch.device("cuda", 0)
TOL = 1e-6


def _run(lib, logits: torch.Tensor, grey: torch.Tensor, stream=None):
    """One nbc_lovasz_softmax call on device tensors, with guard words around both outputs: (terms, counts) numpy."""
    n, _, h, w = logits.shape
    need = lib.nbc_lovasz_workspace_bytes(n, h, w)
    ws = torch.empty(need, dtype=torch.uint8, device=DEV)
    guard = 4
    terms = torch.full((3 * n + 2 * guard,), 1234.5, dtype=torch.float64, device=DEV)
    counts = torch.full((3 * n + 2 * guard,), -77, dtype=torch.int64, device=DEV)
    s = stream if stream is not None else torch.cuda.current_stream(DEV)
    _lib.check(lib.nbc_lovasz_softmax(logits.data_ptr(), grey.data_ptr(), n, h, w, ws.data_ptr(), need,
                                      terms.data_ptr() + 8 * guard, counts.data_ptr() + 8 * guard, s.cuda_stream),
               "nbc_lovasz_softmax")
    s.synchronize()
    t, c = terms.cpu().numpy(), counts.cpu().numpy()
    assert (t[:guard] == 1234.5).all() and (t[-guard:] == 1234.5).all()
    assert (c[:guard] == -77).all() and (c[-guard:] == -77).all()
    return t[guard:-guard].reshape(n, 3), c[guard:-guard].reshape(n, 3)


def _cases(h, w, seed):
    """Five images: random logits and grey levels; one class absent; one class on every pixel; constant logits (every
    error of a class ties); saturated logits +-80 (every error exactly 0 or 1)."""
    rng = np.random.default_rng(seed)
    logits = (rng.normal(size=(5, 3, h, w)) * 3).astype(np.float32)
    grey = rng.integers(0, 256, size=(5, h, w), dtype=np.uint8)
    grey[1] = np.where(rng.random((h, w)) < 0.5, rng.integers(0, 64, size=(h, w)), rng.integers(192, 256, size=(h, w)))
    grey[2] = 130
    logits[3] = np.array([0.5, -1.0, 2.0], np.float32)[:, None, None]
    sat = rng.integers(0, 3, size=(h, w))
    logits[4] = -80
    for c in range(3):
        logits[4, c][sat == c] = 80
    return logits, grey


@pytest.mark.parametrize("hw", [(1, 1), (1, 7), (33, 65), (203, 317), (520, 1024), (1024, 1024)])
def test_terms_match_both_oracles(built_lib, hw):
    h, w = hw
    logits, grey = _cases(h, w, seed=h * 131 + w)
    t, c = _run(built_lib, torch.from_numpy(logits).to(DEV), torch.from_numpy(grey).to(DEV))
    worst64 = worst32 = 0.0
    for i in range(len(logits)):
        t64, c64 = lo.terms_float64(logits[i], grey[i])
        t32, _ = lo.terms_torch_f32(logits[i], grey[i])
        np.testing.assert_array_equal(c[i], c64, err_msg=str(i))
        assert np.all(t[i][c64 == 0] == 0.0), (i, t[i], c64)
        d64 = float(np.max(np.abs(t[i] - t64)))
        worst64, worst32 = max(worst64, d64), max(worst32, float(np.max(np.abs(t[i] - t32))))
        assert d64 <= TOL, (i, t[i], t64)
    assert c[1][1] == 0 and c[2].tolist() == [0, h * w, 0]
    print("%dx%d: max |device - float64| %.3g, max |device - torch f32| %.3g" % (h, w, worst64, worst32))


def test_batch_and_stream_independence(built_lib):
    """An image's terms are bit-identical alone, in a batch of 4 (at each position) and on two streams at once."""
    logits, grey = _cases(203, 317, seed=5)
    logits, grey = logits[:4].copy(), grey[:4].copy()
    L, G = torch.from_numpy(logits).to(DEV), torch.from_numpy(grey).to(DEV)
    batch_t, batch_c = _run(built_lib, L, G)
    for i in range(4):
        alone_t, alone_c = _run(built_lib, L[i:i + 1].contiguous(), G[i:i + 1].contiguous())
        assert alone_t[0].tobytes() == batch_t[i].tobytes() and (alone_c[0] == batch_c[i]).all()
    s1, s2 = torch.cuda.Stream(DEV), torch.cuda.Stream(DEV)
    torch.cuda.synchronize()
    n, _, h, w = L.shape
    outs = []
    for s, sl in ((s1, slice(0, 2)), (s2, slice(2, 4))):
        need = built_lib.nbc_lovasz_workspace_bytes(2, h, w)
        ws = torch.empty(need, dtype=torch.uint8, device=DEV)
        terms = torch.empty((2, 3), dtype=torch.float64, device=DEV)
        counts = torch.empty((2, 3), dtype=torch.int64, device=DEV)
        Ls, Gs = L[sl].contiguous(), G[sl].contiguous()
        torch.cuda.synchronize()
        _lib.check(built_lib.nbc_lovasz_softmax(Ls.data_ptr(), Gs.data_ptr(), 2, h, w, ws.data_ptr(), need, terms.data_ptr(),
                                                counts.data_ptr(), s.cuda_stream), "nbc_lovasz_softmax")
        outs.append((terms, counts, ws, Ls, Gs))
    torch.cuda.synchronize()
    two = np.concatenate([o[0].cpu().numpy() for o in outs])
    assert two.tobytes() == batch_t.tobytes()


def test_non_finite_logits_poison_their_image_only(built_lib):
    logits, grey = _cases(33, 65, seed=9)
    logits = logits[:4].copy()
    logits[1, 0, 5, 7] = np.nan
    logits[2, 2, 30, 60] = np.inf
    logits[3, 1, 0, 0] = -np.inf                       # one class at -inf alone: a finite softmax, as in torch
    t, c = _run(built_lib, torch.from_numpy(logits).to(DEV), torch.from_numpy(grey[:4]).to(DEV))
    for i in (1, 2):
        assert np.all(np.isnan(t[i][c[i] > 0])) and np.all(t[i][c[i] == 0] == 0.0), (i, t[i], c[i])
        assert np.isnan(lo.terms_torch_f32(logits[i], grey[i])[0][c[i] > 0]).all()
        assert np.isnan(metrics.lovasz_loss(t[i], c[i]))
    for i in (0, 3):
        assert np.all(np.isfinite(t[i]))
        np.testing.assert_allclose(t[i], lo.terms_float64(logits[i], grey[i])[0], rtol=0, atol=TOL)


def test_model_method_validates_and_reuses_its_workspace(sd_np, built_lib):
    from neuralbarkcalculator_amd.model import FCNResNet50
    m = FCNResNet50("fp32").load_state_dict(sd_np).to(DEV)
    logits, grey = _cases(64, 96, seed=2)
    L, G = torch.from_numpy(logits).to(DEV), torch.from_numpy(grey).to(DEV)
    t, c = m.lovasz_softmax(L, G)
    assert t.dtype == torch.float64 and c.dtype == torch.int64 and tuple(t.shape) == (5, 3)
    ws = m._lovasz_ws
    t2, _ = m.lovasz_softmax(L[:2].contiguous(), G[:2].contiguous())      # smaller: the cached workspace serves it
    assert m._lovasz_ws is ws
    assert t2.cpu().numpy().tobytes() == t[:2].cpu().numpy().tobytes()
    want, _ = _run(built_lib, L, G)
    assert t.cpu().numpy().tobytes() == want.tobytes()
    for bad in ((L.double(), G), (L, G.long()), (L[:, :2], G), (L, G[:, :-1]), (L.cpu(), G.cpu()), (L[..., :-1], G[..., :-1])):
        with pytest.raises(ValueError):
            m.lovasz_softmax(*bad)
    # predict_labels writes the logits of its own forward
    x = torch.from_numpy(synth.make_frame(3, 64, 96)[None]).to(DEV)
    lg = torch.empty((1, 3, 64, 96), dtype=torch.float32, device=DEV)
    lab, _ = m.predict_labels(x, labels_dtype=torch.uint8, logits_full=lg)
    assert torch.equal(lg, m(x)) and torch.equal(lab, m.predict_labels(x, labels_dtype=torch.uint8)[0])
    with pytest.raises(ValueError):
        m.predict_labels(x, logits_full=torch.empty((1, 3, 64, 95), device=DEV))


# ---- evaluate --loss end to end ----------------------------------------------------------------------------------------
LAYOUT = [("epinette_gelee", "a.png", 81, 128, 128), ("epinette_gelee", "b.png", 82, 96, 128), ("sapin", "c.png", 83, 128, 128),
          ("sapin", "d.png", 84, 128, 128), ("sapin", "e_nodual.png", 85, 96, 128)]


@pytest.fixture(scope="module")
def folder(tmp_path_factory, sd_np):
    """Five samples; four duals with grey levels in all three bands (d.png without nodes), one sample without a dual."""
    root = str(tmp_path_factory.mktemp("lovasz_folder"))
    rng = np.random.default_rng(77)
    truth = {}
    for wood, name, idx, h, w in LAYOUT:
        for sub in ("samples", "duals"):
            os.makedirs(os.path.join(root, sub, wood), exist_ok=True)
        img = synth.make_frame(idx, h, w)
        Image.fromarray(img, mode="RGB").save(os.path.join(root, "samples", wood, name))
        if "nodual" in name:
            continue
        cls = rng.integers(0, 2 if name == "d.png" else 3, size=(h, w))
        grey = np.array([20, 128, 230], np.uint8)[cls]
        Image.fromarray(grey, mode="L").save(os.path.join(root, "duals", wood, name))
        truth[(wood, name)] = (img, grey)
    ckpt = os.path.join(root, "best_model.pt")
    torch.save({k: torch.from_numpy(v) for k, v in sd_np.items()}, ckpt)
    return root, ckpt, truth


def _csv(root):
    return list(csv.reader(open(os.path.join(root, ev.STATS_CSV)), delimiter="\t"))


def _model_terms(sd_np, precision, img, grey):
    from neuralbarkcalculator_amd.model import FCNResNet50
    m = FCNResNet50(precision).load_state_dict(sd_np).to(DEV)
    logits = m(torch.from_numpy(img[None]).to(DEV))
    t, c = m.lovasz_softmax(logits, torch.from_numpy(grey[None]).to(DEV))
    torch.cuda.synchronize()
    return logits.cpu().numpy()[0], t.cpu().numpy()[0], c.cpu().numpy()[0]


def test_evaluate_loss_end_to_end(folder, sd_np):
    root, ckpt, truth = folder
    losses = {}
    for precision in ("fp32", "f16x2"):
        st = ev.evaluate_folder(root, ckpt, precision=precision, device_index=0, loss=True)
        rows = _csv(root)
        assert rows[0] == ev.csv_header(loss=True) and len(rows[0]) == 19
        assert len(rows) == 1 + 4
        summary = json.load(open(os.path.join(root, ev.SUMMARY_JSON)))
        for r in rows[1:]:
            img, grey = truth[(r[1], r[0])]
            logits, t, c = _model_terms(sd_np, precision, img, grey)
            cells = metrics.loss_cells(t, c)
            assert r[15:] == cells, (r[0], r[15:], cells)             # the same bits as the method on model(x)'s logits
            t32, c32 = lo.terms_torch_f32(logits, grey)
            assert np.all(c == c32) and np.max(np.abs(t - t32)) <= TOL
            if r[0] == "d.png":
                assert r[17] == "" and c[2] == 0
            assert st["loss_terms"][[i for i, it in enumerate(ev.list_labelled(root)) if it["name"] == r[0]][0]].tobytes() \
                == t.tobytes()
            losses.setdefault(r[0], {})[precision] = float(r[18])
        ls = summary["lovasz_softmax"]
        assert ls["mean_over_images"] == pytest.approx(np.mean([float(r[18]) for r in rows[1:]]), abs=1e-15)
        for k, name in enumerate(metrics.CLASS_NAMES):
            vals = [float(r[15 + k]) for r in rows[1:] if r[15 + k] != ""]
            assert ls["per_class_mean"][name] == pytest.approx(np.mean(vals), abs=1e-15)
        assert "lovasz_softmax loss" in ev.format_summary(summary)
    diff = max(abs(v["fp32"] - v["f16x2"]) for v in losses.values())
    print("fp32 against f16x2: largest per-image loss difference %.3g" % diff)
    assert diff < 1e-5, losses

    # without --loss: the 15 columns, 22-wide rows and no loss key, as before
    st = ev.evaluate_folder(root, ckpt, precision="fp32", device_index=0)
    rows = _csv(root)
    assert rows[0] == metrics.EVAL_CSV_HEADER and all(len(r) == 15 for r in rows)
    assert all(len(r) == ev.ROW_WIDTH for r in st["rows"]) and "loss_terms" not in st
    assert "lovasz_softmax" not in json.load(open(os.path.join(root, ev.SUMMARY_JSON)))


def test_two_ranks_gather_the_terms_of_one(folder, tmp_path):
    root, ckpt, _ = folder
    ev.evaluate_folder(root, ckpt, precision="f16x2", device_index=0, loss=True)
    want = open(os.path.join(root, ev.STATS_CSV)).read()
    code = ("import sys, torch.distributed as dist\n"
            "sys.path.insert(0, %r)\n"
            "from neuralbarkcalculator_amd import evaluate\n"
            "dist.init_process_group('gloo')\n"
            "st = evaluate.evaluate_folder(%r, %r, precision='f16x2', device_index=0, loss=True)\n"
            "assert st['world'] == 2 and st['images_total'] == %d\n"
            "dist.destroy_process_group()\n" % (REPO, root, ckpt, len(LAYOUT)))
    script = tmp_path / "run2.py"
    script.write_text(code)
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0", OMP_NUM_THREADS="1")
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK"):
        env.pop(k, None)
    p = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2",
                        "--master-addr", "127.0.0.1", "--master-port", "29693", str(script)],
                       cwd=REPO, env=env, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-3000:]
    assert open(os.path.join(root, ev.STATS_CSV)).read() == want
    p = subprocess.run([sys.executable, "-m", "neuralbarkcalculator_amd.evaluate", root, "--model_path", ckpt, "--precision", "f16x2",
                        "--loss"], cwd=REPO, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-3000:]
    assert open(os.path.join(root, ev.STATS_CSV)).read() == want
    assert "lovasz_softmax loss: mean over images" in p.stdout
