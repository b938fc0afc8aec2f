"""The host restatements of the classifier.4 refit (neuralbarkcalculator_amd/refit.py) without a GPU: ce_gradient_cpu and
head_gradient_cpu against torch.autograd in float64, the 1x1 low-resolution case, the loss tables, the objective and the
checkpoint writer."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from neuralbarkcalculator_amd import metrics, refit, synth

# both sides are float64 and differ by their summation order only: the project's bound on such a pair
# (tests/test_gpu_pixel_ce.py), relative to the sum of the absolute values of a cell's terms
SUM_RTOL = 1e-9
SHAPES = [(8, 8, 1, 1), (24, 40, 3, 5), (64, 96, 8, 12), (17, 23, 3, 4), (203, 317, 26, 40)]   # (H, W, h, w)
WEIGHTS = (0.40, 2.03, 93.2)


def _case(H, W, h, w, seed):
    rng = np.random.default_rng(seed)
    low = rng.normal(size=(3, h, w)) * 3
    grey = rng.integers(0, 256, size=(H, W), dtype=np.uint8)
    return low, grey


@pytest.mark.parametrize("loss", refit.LOSSES)
@pytest.mark.parametrize("shape", SHAPES)
def test_ce_gradient_cpu_is_autograd_through_the_bicubic_upsample(shape, loss):
    H, W, h, w = shape
    low_np, grey = _case(H, W, h, w, seed=H * 1000 + W)
    T = refit.table_of(loss, WEIGHTS)
    low = torch.tensor(low_np[None], dtype=torch.float64, requires_grad=True)
    full = F.interpolate(low, size=(H, W), mode="bicubic", align_corners=False)
    t = torch.from_numpy(metrics.target_classes(grey).astype(np.int64))[None]
    ce = F.cross_entropy(full, t, reduction="none")
    weight = torch.from_numpy(T)[t, full.argmax(dim=1)]              # a constant of the pixel, as index_select makes it
    (ce * weight).sum().backward()
    want = low.grad[0].numpy()
    taps = (refit.bicubic_taps_cpu(h, H, np.float64), refit.bicubic_taps_cpu(w, W, np.float64))
    got, mag, _ = refit.ce_gradient_cpu(full.detach().numpy()[0], grey, h, w, T, taps, return_abs=True)
    assert got.shape == (3, h, w) and got.dtype == np.float64
    ratio = np.abs(got - want) / (SUM_RTOL * mag)
    print("%s %s: worst |restatement - autograd| %.3g of its bound, largest gradient %.3g" % (shape, loss, ratio.max(), np.abs(want).max()))
    assert np.all(ratio <= 1.0)
    assert np.abs(want).max() > 0


def test_head_gradient_cpu_is_autograd_of_the_linear_head():
    rng = np.random.default_rng(3)
    h, w = 5, 7
    X = rng.normal(size=(512, h, w)).astype(np.float32)
    G = rng.normal(size=(3, h, w)) * 10
    Wt = torch.zeros((3, 512), dtype=torch.float64, requires_grad=True)
    b = torch.zeros(3, dtype=torch.float64, requires_grad=True)
    Xt = torch.from_numpy(X.astype(np.float64)).reshape(512, -1)
    lowres = Wt @ Xt + b[:, None]
    (lowres * torch.from_numpy(G).reshape(3, -1)).sum().backward()
    got, mag = refit.head_gradient_cpu(G, X, return_abs=True)
    assert got.shape == (3, 513)
    assert np.all(np.abs(got[:, :512] - Wt.grad.numpy()) <= SUM_RTOL * mag[:, :512])
    assert np.all(np.abs(got[:, 512] - b.grad.numpy()) <= SUM_RTOL * mag[:, 512])
    theta_order = refit.theta_vector(got)
    assert np.array_equal(theta_order[:1536].reshape(3, 512), got[:, :512]) and np.array_equal(theta_order[1536:], got[:, 512])


@pytest.mark.parametrize("loss", refit.LOSSES)
def test_one_low_resolution_cell_collects_every_pixel(loss):
    """(h, w) = (1, 1): every tap is clamped to the one cell and a pixel's coefficients sum to 1, so grad_lowres is the plain
    sum of g over the pixels."""
    H, W = 8, 8
    rng = np.random.default_rng(11)
    logits = (rng.normal(size=(3, H, W)) * 3).astype(np.float32)
    grey = rng.integers(0, 256, size=(H, W), dtype=np.uint8)
    T = refit.table_of(loss, WEIGHTS)
    for dtype in (np.float32, np.float64):
        taps = (refit.bicubic_taps_cpu(1, H, dtype), refit.bicubic_taps_cpu(1, W, dtype))
        assert (taps[0][0] == 0).all() and taps[0][2].tolist() == [0] and taps[0][3].tolist() == [H - 1]
        got, mag, terms = refit.ce_gradient_cpu(logits, grey, 1, 1, T, taps, return_abs=True)
        g = refit.pixel_gradient_cpu(logits, grey, T)
        # f32 coefficients sum to 1 within 2^-20 per axis (tests/test_refit_abi.py holds the table to that); it is part of
        # the value, not of the summation order
        slack = 0.0 if dtype is np.float64 else 2 * 2.0 ** -20
        assert np.all(np.abs(got[:, 0, 0] - g.sum(axis=(1, 2))) <= (SUM_RTOL + slack) * mag[:, 0, 0])
        assert terms[0, 0, 0] == 16 * H * W


def test_pixel_gradient_definition():
    logits = np.array([[[2.0]], [[-1.0]], [[0.5]]], dtype=np.float32)
    T = np.arange(1.0, 10.0).reshape(3, 3)
    for grey, t in ((10, 0), (100, 1), (250, 2)):
        g = refit.pixel_gradient_cpu(logits, np.array([[grey]], dtype=np.uint8), T)[:, 0, 0]
        q = np.exp(logits[:, 0, 0].astype(np.float64) - 2.0)
        q /= q.sum()
        want = T[t, 0] * (q - np.eye(3)[t])
        assert np.allclose(g, want, rtol=1e-15, atol=0)
        assert abs(g.sum()) <= 1e-15 * T[t, 0]
    # a NaN logit poisons its pixel and no other; the argmax takes the NaN as the maximum
    two = np.zeros((3, 1, 2), dtype=np.float32)
    two[1, 0, 0] = np.nan
    g = refit.pixel_gradient_cpu(two, np.array([[10, 10]], dtype=np.uint8), T)
    assert np.isnan(g[:, 0, 0]).all() and np.isfinite(g[:, 0, 1]).all()


def test_table_of():
    w = np.array(WEIGHTS)
    assert np.array_equal(refit.table_of("ce"), np.ones((3, 3))) and np.array_equal(refit.table_of("ce", w), np.ones((3, 3)))
    for t in range(3):
        for p in range(3):
            assert refit.table_of("weighted_ce", w)[t, p] == w[max(t, p)]
            assert refit.table_of("class_ce", w)[t, p] == w[t]
    assert np.array_equal(refit.table_of("weighted_ce"), refit.table_of("weighted_ce", metrics.REFERENCE_CLASS_WEIGHTS))
    for bad in (("lovasz", w), ("class_ce", (1, 2)), ("class_ce", (1, -2, 3)), ("weighted_ce", (1, np.nan, 3))):
        with pytest.raises(ValueError):
            refit.table_of(*bad)


def test_objective_adds_the_rows_in_order_and_the_penalty():
    rng = np.random.default_rng(5)
    T = refit.table_of("weighted_ce", WEIGHTS)
    rows = [(rng.random((3, 3)) * 100, rng.integers(1, 50, size=(3, 3)), rng.normal(size=(3, 513))) for _ in range(4)]
    theta0 = rng.normal(size=1539).astype(np.float32)
    theta = (theta0 + rng.normal(size=1539).astype(np.float32) * 0.1).astype(np.float32)
    value, data, grad = refit.objective(rows, T, 0.25, theta, theta0)
    P = sum(int(r[1].sum()) for r in rows)
    assert data == pytest.approx(sum(float((T * r[0]).sum()) for r in rows) / P, rel=1e-15)
    d = theta.astype(np.float64) - theta0.astype(np.float64)
    assert value == pytest.approx(data + 0.125 * float(d @ d), rel=1e-15)
    g = sum(r[2] for r in rows)
    want = np.concatenate([g[:, :512].ravel(), g[:, 512]]) / P + 0.25 * d
    assert np.allclose(grad, want, rtol=1e-14, atol=0) and grad.shape == (1539,)
    # the same rows cut as two ranks would hold them, gathered back in list order: the same bits
    again = refit.objective(rows[:1] + rows[1:], T, 0.25, theta, theta0)
    assert again[0] == value and again[2].tobytes() == grad.tobytes()
    with pytest.raises(ValueError):
        refit.objective([], T, 0.0, theta, theta0)


def test_checkpoint_round_trip_changes_the_two_keys_only(tmp_path, sd_np):
    sd = {k: torch.from_numpy(v) for k, v in sd_np.items()}
    theta0 = refit.theta_of(sd)
    assert theta0.dtype == np.float32 and theta0.shape == (1539,)
    assert np.array_equal(theta0[:1536].reshape(3, 512), sd_np["classifier.4.weight"][:, :, 0, 0])
    assert np.array_equal(theta0[1536:], sd_np["classifier.4.bias"])
    theta = (theta0 + np.float32(0.5) * synth.normal(3, 1, 1539).astype(np.float32)).astype(np.float32)
    path = str(tmp_path / "refit_model.pt")
    refit.write_checkpoint(sd, theta, path)
    back = torch.load(path, map_location="cpu", weights_only=True)
    assert list(back) == list(sd)
    for k in sd:
        assert back[k].dtype == sd[k].dtype and tuple(back[k].shape) == tuple(sd[k].shape), k
        if k in (refit.W_KEY, refit.B_KEY):
            assert not torch.equal(back[k], sd[k])
        else:
            assert torch.equal(back[k], sd[k]), k
    assert refit.theta_of(back).tobytes() == theta.tobytes()
    assert torch.equal(sd[refit.W_KEY], torch.from_numpy(sd_np[refit.W_KEY]))          # the input is not written
    # numpy state dicts keep their type too
    back_np = refit.replace_head(sd_np, theta)
    assert list(back_np) == list(sd_np) and back_np[refit.W_KEY].dtype == np.float32 and back_np[refit.W_KEY].shape == (3, 512, 1, 1)
    assert back_np["backbone.conv1.weight"] is sd_np["backbone.conv1.weight"]
    for bad in (theta[:-1], np.zeros(1540, np.float32)):
        with pytest.raises(ValueError):
            refit.replace_head(sd, bad)


def test_driver_refuses_before_any_device(tmp_path):
    for kw, text in [(dict(loss="lovasz"), "loss must be one of"), (dict(l2=-1.0), "--l2 must be"), (dict(l2=float("nan")), "--l2 must be"),
                     (dict(iterations=0), "--iterations must be"), (dict(precision="bf16"), "fp32 or f16x2"),
                     (dict(loss="class_ce", class_weights=(1, 2)), "three finite numbers")]:
        with pytest.raises(ValueError, match=text):
            refit.refit_folder(str(tmp_path), str(tmp_path / "out.pt"), "/nonexistent/ckpt.pt", **kw)
    (tmp_path / "samples").mkdir()
    with pytest.raises(ValueError, match="no sample to fit on"):
        refit.refit_folder(str(tmp_path), str(tmp_path / "out.pt"), "/nonexistent/ckpt.pt")
