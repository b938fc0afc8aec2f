"""The classifier.4 refit on the GPU (include/nbc.h): nbc_head_logits against the forward bit for bit,
nbc_ce_gradient and nbc_head_gradient against the float64 restatements of neuralbarkcalculator_amd/refit.py, batch and stream
independence, the state contract, the tap table against the forward's own upsample, and the driver end to end on one and two
ranks."""
import csv
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
from PIL import Image

from neuralbarkcalculator_amd import _lib, refit, synth
from neuralbarkcalculator_amd import evaluate as ev
from neuralbarkcalculator_amd import model as mdl
from neuralbarkcalculator_amd.model import DeepLabV3ResNet50, FCNResNet50
from neuralbarkcalculator_amd.topology import out_hw

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = torch.device("cuda", 0)
# device and restatement are float64 sums of the same terms in another order: the project's bound on such a pair
# (tests/test_gpu_pixel_ce.py), relative to the sum of the absolute values of a cell's terms, plus an absolute part per term
SUM_RTOL, SUM_ATOL_PER_TERM = 1e-9, 1e-12
WEIGHTS = (0.40, 2.03, 93.2)
SHAPES = [(8, 8, 1, 1), (24, 40, 3, 5), (64, 96, 8, 12), (17, 23, 3, 4), (203, 317, 26, 40), (256, 256, 32, 32)]   # (H, W, h, w)


def frames(idx, h, w):
    return torch.from_numpy(np.stack([synth.make_input(int(i), h, w) for i in idx]))


@pytest.fixture(scope="module")
def models(sd_np, built_lib):
    return {p: FCNResNet50(p).load_state_dict(sd_np).to(DEV) for p in ("fp32", "f16x2", "bf16")}


@pytest.fixture(scope="module")
def theta0(sd_np):
    return refit.theta_of(sd_np)


def _cases(h, w, seed):
    """Five images, as tests/test_gpu_pixel_ce.py builds them: random logits and grey levels; saturated logits +-80; a constant
    image; one class absent from the dual; one class on every pixel of it."""
    rng = np.random.default_rng(seed)
    logits = (rng.normal(size=(5, 3, h, w)) * 3).astype(np.float32)
    grey = rng.integers(0, 256, size=(5, h, w), dtype=np.uint8)
    sat = rng.integers(0, 3, size=(h, w))
    logits[1] = -80
    for c in range(3):
        logits[1, c][sat == c] = 80
    logits[2] = np.array([0.5, -1.0, 2.0], np.float32)[:, None, None]
    grey[2] = 127
    grey[3] = np.where(rng.random((h, w)) < 0.5, rng.integers(0, 64, size=(h, w)), rng.integers(192, 256, size=(h, w)))
    grey[4] = 130
    return logits, grey


def _bits(t: torch.Tensor) -> bytes:
    return t.detach().cpu().contiguous().numpy().tobytes()


# ---- identity ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", ["fp32", "f16x2", "bf16"])
@pytest.mark.parametrize("hw", [(64, 96), (203, 317)])
def test_checkpoint_theta_gives_the_forward_bit_for_bit(models, theta0, precision, hw):
    m = models[precision]
    H, W = hw
    T = refit.table_of("weighted_ce", WEIGHTS)
    rng = np.random.default_rng(H)
    for n in (1, 3):
        x = frames(range(40, 40 + n), H, W).to(DEV)
        tgt = torch.from_numpy(rng.integers(0, 256, size=(n, H, W), dtype=np.uint8)).to(DEV)
        lg = torch.empty((n, 3, H, W), dtype=torch.float32, device=DEV)
        _, _, low = m.predict_labels(x, labels_dtype=torch.uint8, return_lowres=True, logits_full=lg)
        trial = m.head_logits(theta0)
        assert trial.shape == low.shape == (n, 3) + out_hw(H, W) and _bits(trial) == _bits(low), (precision, n)
        sums, counts, grad = m.head_loss_and_gradient(tgt, theta0, T)
        want_s, want_c = m.pixel_cross_entropy(lg, tgt)
        torch.cuda.synchronize()
        assert _bits(sums) == _bits(want_s) and _bits(counts) == _bits(want_c), (precision, n)
        assert grad.shape == (n, 3, 513) and grad.dtype == torch.float64 and bool(torch.isfinite(grad).all())
        # a softmax gradient sums to zero over the classes, pixel by pixel; so do the bias columns, up to their rounding
        bias = grad[:, :, 512].cpu().numpy()
        assert np.all(np.abs(bias.sum(axis=1)) <= 1e-9 * np.abs(bias).sum(axis=1))
    assert not m.nonfinite_seen()
    # another theta gives other logits: the call reads its argument
    other = theta0.copy()
    other[1536:] += np.float32(0.25)
    moved = m.head_logits(other)
    assert not torch.equal(moved, trial) and torch.allclose(moved, trial + 0.25, rtol=0, atol=1e-4 * float(trial.abs().max()) + 1e-5)


# ---- nbc_ce_gradient against the restatement -------------------------------------------------------------------------------
def _tables_on_device(n_in, n_out):
    host = mdl.bicubic_taps(n_in, n_out)
    return host, tuple(torch.from_numpy(a).to(DEV) for a in host)


def _ce_gradient(lib, logits, grey, h, w, table, rows, cols, stream=None):
    """One nbc_ce_gradient call with guard words around the output: numpy float64 [N,3,h,w]."""
    n, _, H, W = logits.shape
    need = lib.nbc_ce_gradient_workspace_bytes(n, H, W, h, w)
    assert need > 0
    ws = torch.empty(need, dtype=torch.uint8, device=DEV)
    guard = 4
    out = torch.full((n * 3 * h * w + 2 * guard,), 1234.5, dtype=torch.float64, device=DEV)
    tab = np.ascontiguousarray(np.asarray(table, dtype=np.float64).reshape(-1))
    import ctypes as C
    s = stream if stream is not None else torch.cuda.current_stream(DEV)
    _lib.check(lib.nbc_ce_gradient(logits.data_ptr(), grey.data_ptr(), n, H, W, h, w, *[t.data_ptr() for t in rows + cols],
                                   tab.ctypes.data_as(C.POINTER(C.c_double)), ws.data_ptr(), need, out.data_ptr() + 8 * guard,
                                   s.cuda_stream), "nbc_ce_gradient")
    s.synchronize()
    t = out.cpu().numpy()
    assert (t[:guard] == 1234.5).all() and (t[-guard:] == 1234.5).all()
    return t[guard:-guard].reshape(n, 3, h, w)


@pytest.mark.parametrize("shape", SHAPES)
def test_ce_gradient_matches_the_float64_restatement(built_lib, shape):
    H, W, h, w = shape
    logits, grey = _cases(H, W, seed=H * 131 + W)
    rows_h, rows_d = _tables_on_device(h, H)
    cols_h, cols_d = _tables_on_device(w, W)
    L, G = torch.from_numpy(logits).to(DEV), torch.from_numpy(grey).to(DEV)
    for loss in refit.LOSSES:
        T = refit.table_of(loss, WEIGHTS)
        got = _ce_gradient(built_lib, L, G, h, w, T, rows_d, cols_d)
        worst = 0.0
        for i in range(len(logits)):
            want, mag, terms = refit.ce_gradient_cpu(logits[i], grey[i], h, w, T, (rows_h, cols_h), return_abs=True)
            bound = SUM_RTOL * mag + SUM_ATOL_PER_TERM * terms
            ratio = np.abs(got[i] - want) / bound
            worst = max(worst, float(ratio.max()))
            assert np.all(ratio <= 1.0), (shape, loss, i, float(ratio.max()))
        print("%s %s: worst |device - float64| %.3g of its bound" % (shape, loss, worst))
    assert np.abs(got[0]).max() > 0


def test_ce_gradient_propagates_nan_into_the_cells_it_touches(built_lib):
    H, W, h, w = 24, 40, 3, 5
    logits, grey = _cases(H, W, seed=1)
    logits[0, 1, 0, 0] = np.nan
    rows_h, rows_d = _tables_on_device(h, H)
    cols_h, cols_d = _tables_on_device(w, W)
    T = refit.table_of("ce")
    got = _ce_gradient(built_lib, torch.from_numpy(logits[:1]).to(DEV), torch.from_numpy(grey[:1]).to(DEV), h, w, T, rows_d, cols_d)[0]
    want = refit.ce_gradient_cpu(logits[0], grey[0], h, w, T, (rows_h, cols_h))
    assert np.array_equal(np.isnan(got), np.isnan(want)) and np.isnan(got).any() and not np.isnan(got).all()
    hit = np.zeros((h, w), dtype=bool)
    hit[np.unique(rows_h[0][0])[:, None], np.unique(cols_h[0][0])[None, :]] = True       # the cells pixel (0, 0) has taps on
    assert np.array_equal(np.isnan(got), np.broadcast_to(hit, (3, h, w)))


# ---- batch and stream independence ----------------------------------------------------------------------------------------------
def test_batch_and_stream_independence(models, built_lib, theta0):
    H, W, h, w = 203, 317, 26, 40
    logits, grey = _cases(H, W, seed=5)
    rows_h, rows_d = _tables_on_device(h, H)
    cols_h, cols_d = _tables_on_device(w, W)
    T = refit.table_of("weighted_ce", WEIGHTS)
    L, G = torch.from_numpy(logits[:3].copy()).to(DEV), torch.from_numpy(grey[:3].copy()).to(DEV)
    alone = [_ce_gradient(built_lib, L[i:i + 1].contiguous(), G[i:i + 1].contiguous(), h, w, T, rows_d, cols_d)[0] for i in range(3)]
    for order in ([0, 1, 2], [2, 0, 1], [1, 2], [2, 1]):
        got = _ce_gradient(built_lib, L[order].contiguous(), G[order].contiguous(), h, w, T, rows_d, cols_d)
        for pos, i in enumerate(order):
            assert got[pos].tobytes() == alone[i].tobytes(), (order, pos)
    side = torch.cuda.Stream(DEV)
    torch.cuda.synchronize()
    got = _ce_gradient(built_lib, L[[1, 2, 0]].contiguous(), G[[1, 2, 0]].contiguous(), h, w, T, rows_d, cols_d, stream=side)
    for pos, i in enumerate([1, 2, 0]):
        assert got[pos].tobytes() == alone[i].tobytes()
    # the whole chain on the features of a forward: alone, in batches of 2 and 3, and on a side stream
    m = models["fp32"]
    x = frames([50, 51, 52], H, W).to(DEV)
    tgt = G

    def chain(sel):
        m.lowres_logits(x[sel].contiguous())
        low = m.head_logits(theta0)
        _, _, full = m.upsample_argmax(low, (H, W), labels_dtype=torch.uint8, return_logits=True)
        gl = m.ce_gradient(full, tgt[sel].contiguous(), (h, w), T)
        return gl, m.head_gradient(gl)
    single = []
    for i in range(3):
        gl, gt = chain([i])
        single.append((_bits(gl[0]), _bits(gt[0])))
    for sel in ([0, 1, 2], [1, 0], [2, 1]):
        gl, gt = chain(sel)
        for pos, i in enumerate(sel):
            assert (_bits(gl[pos]), _bits(gt[pos])) == single[i], (sel, pos)
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        gl, gt = chain([2, 0, 1])
    side.synchronize()
    for pos, i in enumerate([2, 0, 1]):
        assert (_bits(gl[pos]), _bits(gt[pos])) == single[i]


# ---- nbc_head_gradient against the restatement -----------------------------------------------------------------------------
def _with_large_head_features(sd_np):
    """The same network with the tensor classifier.4 reads 2^10 times larger: its BatchNorm's gamma and beta times 2^10 (exact),
    so that f16x2 stores it with a power of two of its own."""
    sd = dict(sd_np)
    for leaf in ("weight", "bias"):
        sd["classifier.1." + leaf] = sd_np["classifier.1." + leaf] * np.float32(1024.0)
    return sd


@pytest.mark.parametrize("precision", ["fp32", "f16x2"])
@pytest.mark.parametrize("hw", [(64, 96), (203, 317)])
def test_head_gradient_matches_the_float64_restatement(sd_np, built_lib, precision, hw):
    H, W = hw
    h, w = out_hw(H, W)
    sd = _with_large_head_features(sd_np) if precision == "f16x2" else sd_np
    m = FCNResNet50(precision).load_state_dict(sd).to(DEV)
    n = 2
    x = frames([60, 61], H, W).to(DEV)
    rng = np.random.default_rng(H + 1)
    G = rng.normal(size=(n, 3, h, w)) * np.exp(rng.normal(size=(n, 3, h, w)) * 3)
    m.set_keep_activations(True)
    try:
        low = m.lowres_logits(x)
        got = m.head_gradient(torch.from_numpy(G).to(DEV))
        trial = m.head_logits(refit.theta_of(sd))
        torch.cuda.synchronize()
        X = m.read_activation("classifier.0", n * 512 * h * w)
        exponent = m.activation_exponent("classifier.0")
    finally:
        m.set_keep_activations(False)
    assert (exponent != 0) == (precision == "f16x2"), exponent          # f16x2: the 2^-a of both calls is exercised
    assert _bits(trial) == _bits(low)
    assert X.shape == (n, 512, h, w)
    got = got.cpu().numpy()
    worst = 0.0
    for i in range(n):
        want, mag = refit.head_gradient_cpu(G[i], X[i], return_abs=True)
        ratio = np.abs(got[i] - want) / (SUM_RTOL * mag + SUM_ATOL_PER_TERM * h * w)
        worst = max(worst, float(ratio.max()))
        assert np.all(ratio <= 1.0), (precision, hw, i, float(ratio.max()))
    print("%s %dx%d: worst |device - float64| %.3g of its bound (stored exponent %d)" % (precision, H, W, worst, exponent))


# ---- state contract ---------------------------------------------------------------------------------------------------------------
def test_state_contract(sd_np, built_lib):
    lib = built_lib
    theta = torch.from_numpy(refit.theta_of(sd_np)).to(DEV)
    H, W = 64, 96
    h, w = out_hw(H, W)
    low = torch.empty((1, 3, h, w), dtype=torch.float32, device=DEV)
    gl = torch.zeros((1, 3, h, w), dtype=torch.float64, device=DEV)
    gt = torch.empty((1, 3, 513), dtype=torch.float64, device=DEV)
    need = lib.nbc_head_gradient_workspace_bytes(1, H, W)
    ws = torch.empty(need, dtype=torch.uint8, device=DEV)
    stream = torch.cuda.current_stream(DEV).cuda_stream

    def both(m, n=1, hh=H, ww=W):
        return (lib.nbc_head_logits(m._ctx, theta.data_ptr(), n, hh, ww, low.data_ptr(), stream),
                lib.nbc_head_gradient(m._ctx, gl.data_ptr(), n, hh, ww, ws.data_ptr(), need, gt.data_ptr(), stream))
    m = FCNResNet50("fp32").load_state_dict(sd_np).to(DEV)
    assert both(m) == (_lib.NBC_ERR_STATE, _lib.NBC_ERR_STATE)           # no forward yet
    with pytest.raises(RuntimeError):
        m.head_logits(theta)
    m.lowres_logits(frames([1], 96, 128).to(DEV))
    assert both(m) == (_lib.NBC_ERR_STATE, _lib.NBC_ERR_STATE)           # a forward of another shape
    m.lowres_logits(frames([1], H, W).to(DEV))
    assert both(m) == (_lib.NBC_OK, _lib.NBC_OK)
    m.reserve(1, 96, 128)                                                # the plan has been touched since
    assert both(m) == (_lib.NBC_ERR_STATE, _lib.NBC_ERR_STATE)
    dl = DeepLabV3ResNet50("fp32").load_state_dict(synth.make_state_dict("trained_like", seed=7, arch="deeplabv3_resnet50")).to(DEV)
    dl.lowres_logits(frames([1], H, W).to(DEV))
    assert both(dl) == (_lib.NBC_ERR_STATE, _lib.NBC_ERR_STATE)
    assert "NBC_ARCH_FCN_RESNET50 only" in _lib.last_error()
    torch.cuda.synchronize()


# ---- the tap table against the forward's own upsample -----------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(64, 96, 8, 12), (203, 317, 26, 40)])
def test_tap_table_is_the_forwards_upsample(models, shape):
    """One-hot low-resolution planes through nbc_upsample_argmax: the plane of cell (i, j) holds, at (Y, X), the weight the
    forward gives that cell there, which the table states as the product of the row and the column coefficients.  The kernel
    may contract its coefficient expressions into fmas (a few 2^-24 of intermediates below 8, per factor): 2^-18."""
    H, W, h, w = shape
    m = models["fp32"]
    Ay = refit._adjoint_matrices(mdl.bicubic_taps(h, H), h)[0]
    Ax = refit._adjoint_matrices(mdl.bicubic_taps(w, W), w)[0]
    cells = h * w
    worst = 0.0
    per_call = 32 * 3                                                   # three cells per image, one per class plane
    for first in range(0, cells, per_call):
        ids = np.arange(first, min(first + per_call, cells))
        n = (len(ids) + 2) // 3
        low = np.zeros((n * 3, h * w), dtype=np.float32)
        low[np.arange(len(ids)), ids] = 1.0
        _, _, full = m.upsample_argmax(torch.from_numpy(low.reshape(n, 3, h, w)).to(DEV), (H, W), labels_dtype=torch.uint8,
                                       return_logits=True)
        full = full.cpu().numpy().reshape(n * 3, H, W).astype(np.float64)
        for k, cell in enumerate(ids):
            want = Ay[cell // w][:, None] * Ax[cell % w][None, :]
            worst = max(worst, float(np.abs(full[k] - want).max()))
    print("%s: worst |forward - table| %.3g (2^-18 = %.3g)" % (shape, worst, 2.0 ** -18))
    assert worst <= 2.0 ** -18


# ---- the driver ---------------------------------------------------------------------------------------------------------------------
ITEMS = [("epinette_gelee", "a.png", 91), ("epinette_gelee", "b.png", 92), ("sapin", "c.png", 93), ("sapin", "d.png", 94)]
SIZE = (64, 96)


@pytest.fixture(scope="module")
def fitted(tmp_path_factory, sd_np, built_lib):
    """Four synthetic frames whose duals are the labels of a perturbed head theta* = theta0 + noise, and one run of the driver
    on them from theta0 (one rank)."""
    root = str(tmp_path_factory.mktemp("refit_folder"))
    theta0 = refit.theta_of(sd_np)
    star = (theta0 + np.float32(0.02) * synth.normal(11, 3, 1539).astype(np.float32)).astype(np.float32)
    teacher = FCNResNet50("fp32").load_state_dict(refit.replace_head(sd_np, star)).to(DEV)
    for wood, name, idx in ITEMS:
        for sub in ("samples", "duals"):
            os.makedirs(os.path.join(root, sub, wood), exist_ok=True)
        img = synth.make_frame(idx, *SIZE)
        Image.fromarray(img, mode="RGB").save(os.path.join(root, "samples", wood, name))
        labels, _ = teacher.predict_labels(torch.from_numpy(img[None]).to(DEV), labels_dtype=torch.uint8)
        grey = np.array([20, 128, 230], np.uint8)[labels[0].cpu().numpy()]
        Image.fromarray(grey, mode="L").save(os.path.join(root, "duals", wood, name))
    ckpt = os.path.join(root, "best_model.pt")
    torch.save({k: torch.from_numpy(v) for k, v in sd_np.items()}, ckpt)
    out = os.path.join(root, "refit_model.pt")
    stats = refit.refit_folder(root, out, ckpt, loss="ce", iterations=5, precision="fp32", device_index=0, target_size=128)
    log = open(os.path.join(root, refit.LOG_CSV), "rb").read()      # the two-rank run writes the same files again
    summary = json.load(open(os.path.join(root, refit.SUMMARY_JSON)))
    return dict(root=root, ckpt=ckpt, out=out, stats=stats, log=log, summary=summary, theta0=theta0)


def _log_rows(raw: bytes):
    rows = list(csv.reader(raw.decode().splitlines(), delimiter="\t"))
    assert rows[0] == refit.LOG_HEADER
    return rows[1:]


def test_driver_end_to_end(fitted, sd_np):
    rows = _log_rows(fitted["log"])
    summary = fitted["summary"]
    assert fitted["stats"]["summary"] == summary and fitted["stats"]["world"] == 1
    assert [int(r[0]) for r in rows] == list(range(1, len(rows) + 1)) and 2 <= len(rows) <= 2 * 5 + 2
    assert summary["evaluations"] == len(rows) and summary["loss"] == "ce" and summary["table"] == [[1.0] * 3] * 3
    assert summary["images"] == len(ITEMS) and summary["skipped"] == 0 and summary["ranks"] == 1 and summary["precision"] == "fp32"
    for r in rows:
        assert repr(float(r[1])) == r[1] and repr(float(r[2])) == r[2] and float(r[3]) >= 0 and r[4] in ("0", "1")
        assert float(r[1]) == float(r[2])                                # no penalty
    accepted = [float(r[1]) for r in rows if r[4] == "1"]
    assert rows[0][4] == "1" and all(b <= a for a, b in zip(accepted, accepted[1:]))
    assert accepted[-1] < float(rows[0][1])
    assert summary["objective"] == {"before": float(rows[0][1]), "after": accepted[-1]} and accepted[-1] == min(float(r[1]) for r in rows)
    for key in ("before", "after"):
        assert np.array(summary[key]["confusion"]).sum() == len(ITEMS) * SIZE[0] * SIZE[1]
        assert len(summary[key]["iou"]) == len(summary[key]["f1"]) == 3
    # the written checkpoint: the two keys alone have moved, and a fresh model computes head_logits(theta_final) bit for bit
    back = torch.load(fitted["out"], map_location="cpu", weights_only=True)
    assert list(back) == list(sd_np)
    for k, v in sd_np.items():
        assert back[k].dtype == torch.from_numpy(v).dtype and tuple(back[k].shape) == v.shape
        assert (k in (refit.W_KEY, refit.B_KEY)) != bool(torch.equal(back[k], torch.from_numpy(v))), k
    final = refit.theta_of(back)
    x = frames([91, 92], *SIZE).to(DEV)
    fresh = FCNResNet50("fp32").load_state_dict(back).to(DEV)
    old = FCNResNet50("fp32").load_state_dict(sd_np).to(DEV)
    want = fresh.lowres_logits(x)
    old.lowres_logits(x)
    assert _bits(old.head_logits(final)) == _bits(want)
    # every other tool loads it
    st = ev.evaluate_folder(fitted["root"], fitted["out"], precision="fp32", device_index=0, target_size=128)
    assert st["summary"]["images_evaluated"] == len(ITEMS)


def test_two_ranks_write_the_same_bytes(fitted, tmp_path):
    out2 = str(tmp_path / "refit_two_ranks.pt")
    code = ("import sys, torch.distributed as dist\n"
            "sys.path.insert(0, %r)\n"
            "from neuralbarkcalculator_amd import refit\n"
            "dist.init_process_group('gloo')\n"
            "st = refit.refit_folder(%r, %r, %r, loss='ce', iterations=5, precision='fp32', device_index=0, target_size=128)\n"
            "assert st['world'] == 2 and st['images_total'] == %d\n"
            "assert (st['summary'] is not None) == (st['rank'] == 0)\n"
            "dist.destroy_process_group()\n" % (REPO, fitted["root"], out2, fitted["ckpt"], len(ITEMS)))
    script = tmp_path / "run2.py"
    script.write_text(code)
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0", OMP_NUM_THREADS="1")
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK"):
        env.pop(k, None)
    p = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2",
                        "--master-addr", "127.0.0.1", "--master-port", "29703", str(script)],
                       cwd=REPO, env=env, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-3000:]
    assert open(os.path.join(fitted["root"], refit.LOG_CSV), "rb").read() == fitted["log"]
    one = torch.load(fitted["out"], map_location="cpu", weights_only=True)
    two = torch.load(out2, map_location="cpu", weights_only=True)
    assert list(one) == list(two) and all(torch.equal(one[k], two[k]) for k in one)
    assert json.load(open(os.path.join(fitted["root"], refit.SUMMARY_JSON)))["ranks"] == 2
