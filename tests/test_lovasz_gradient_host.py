"""The host restatements of the Lovasz-Softmax gradient (neuralbarkcalculator_amd/refit.py) without a GPU: against the gradients
the reference's own code returned (tests/golden/lovasz_gradient_ref.npz, scripts/record_lovasz_gradient.py), the tie rule, the
folder's objective for ``lovasz`` and ``mixed``, and the command line."""
import os
import sys

import numpy as np
import pytest

from neuralbarkcalculator_amd import metrics, refit

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
from lovasz_gradient_cases import quantised_image, saturated_image  # noqa: E402

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "lovasz_gradient_ref.npz")
# every quantity is an O(1) float64 number with a handful of roundings (1e-15 is expected); 1e-12 is still six orders below
# the smallest slope of a 384-pixel image
PIN_ATOL = 1e-12
WEIGHTS = (0.40, 2.03, 93.2)


def default_keys(logits, grey):
    import torch
    t = metrics.target_classes(grey)
    onehot = np.arange(3)[:, None, None] == t[None]
    p = torch.softmax(torch.from_numpy(logits), dim=0).numpy()
    return refit.lovasz_keys_cpu(np.abs(onehot.astype(np.float32) - p), onehot), onehot


@pytest.mark.parametrize("k", [0, 1])
def test_slopes_and_gradient_are_the_references(k):
    z = np.load(GOLDEN)
    logits, grey, p, dp, dl = (z["%s_%d" % (name, k)] for name in ("logits", "grey", "probs", "dloss_dprobs", "dloss_dlogits"))
    assert logits.shape == (3, 16, 24) and logits.dtype == np.float32 and p.dtype == dp.dtype == dl.dtype == np.float64
    t = metrics.target_classes(grey)
    present = [c for c in range(3) if (t == c).any()]
    assert present == ([0, 1, 2] if k == 0 else [0, 1])
    keys = np.zeros(p.shape, dtype=np.int64)
    worst = 0.0
    for c in range(3):
        fg = t == c
        e = np.abs(fg.astype(np.float64) - p[c])
        assert np.unique(e).size == e.size                               # the recorder's promise: no two errors of a class tie
        keys[c] = refit.lovasz_keys_cpu(e, fg)
        slopes = refit.lovasz_slopes_cpu(e, fg)
        assert slopes.shape == e.shape and slopes.dtype == np.float64 and (slopes >= 0).all()
        d = -np.sign(fg - p[c]) * slopes / len(present) if c in present else np.zeros_like(slopes)
        worst = max(worst, float(np.abs(d - dp[c]).max()))
    print("image %d: worst |slopes - reference dL/dp| %.3g" % (k, worst))
    assert worst <= PIN_ATOL
    got = refit.lovasz_pixel_gradient_cpu(logits.astype(np.float64), grey, keys=keys)
    print("image %d: worst |restatement - reference dL/dlogits| %.3g, largest %.3g" % (k, np.abs(got - dl).max(), np.abs(dl).max()))
    assert np.abs(got - dl).max() <= PIN_ATOL and np.abs(dl).max() > 1e-4
    # the float32 keys the device sorts order these images the same way: the gradient moves by the Jacobian's float64 rounding only
    assert np.abs(refit.lovasz_pixel_gradient_cpu(logits, grey) - dl).max() <= PIN_ATOL
    # the loss the slopes belong to: sum e * slope per class is the class's term
    terms = [float((np.abs((t == c) - p[c]) * refit.lovasz_slopes_cpu(np.abs((t == c) - p[c]), t == c)).sum()) for c in present]
    assert abs(sum(terms) / len(present) - float(z["loss_%d" % k])) <= PIN_ATOL


@pytest.mark.parametrize("make", [quantised_image, saturated_image])
def test_ties_share_the_mean_slope_of_their_run(make):
    logits, grey = make()
    keys, onehot = default_keys(logits, grey)
    rng = np.random.default_rng(1)
    perm = rng.permutation(grey.size)
    for c in range(3):
        e, fg = refit._decode_keys(keys[c].ravel())
        G = int(fg.sum())
        assert G > 0
        slopes = refit.lovasz_slopes_cpu(e, fg)
        J = lambda n, F: 1.0 - (G - F) / (G + n - F) if n else 0.0
        runs = 0
        seen, fg_seen = 0, 0
        for key in sorted(set(keys[c].ravel().tolist()), reverse=True):        # descending keys: equal e puts foreground first
            members = keys[c].ravel() == key
            n, f = int(members.sum()), int(key & 1)
            runs += n > 1
            want = J(seen + n, fg_seen + f * n) - J(seen, fg_seen)
            if key >> 1 == 0:
                assert (slopes[members] == 0).all()                            # e == 0
            else:
                assert np.unique(slopes[members]).size == 1                    # the slopes of a run are equal
                assert abs(slopes[members].sum() - want) <= 1e-14              # and sum to J(end) - J(start)
            seen, fg_seen = seen + n, fg_seen + f * n
        assert runs > 0                                                        # the image does tie
        # permuting the pixels permutes the slopes exactly
        assert np.array_equal(refit.lovasz_slopes_cpu(e[perm], fg[perm]), slopes[perm])
        assert np.array_equal(refit.lovasz_slopes_cpu(e.astype(np.float64), fg), slopes)   # any float dtype
    g = refit.lovasz_pixel_gradient_cpu(logits, grey)
    flat = lambda a: a.reshape(3, -1)
    H, W = grey.shape
    again = refit.lovasz_pixel_gradient_cpu(flat(logits)[:, perm].reshape(3, H, W), grey.ravel()[perm].reshape(H, W))
    assert np.array_equal(flat(again), flat(g)[:, perm])
    assert np.isfinite(g).all() and np.abs(g.sum(axis=0)).max() <= 1e-15
    if make is saturated_image:
        e, _ = refit._decode_keys(keys.ravel())
        assert set(np.unique(e).tolist()) == {0.0, 1.0}


def test_absent_classes_nan_and_weights():
    rng = np.random.default_rng(9)
    logits = rng.normal(size=(3, 6, 7)).astype(np.float32)
    grey = rng.choice(np.array([10, 128], np.uint8), size=(6, 7))                # class 2 absent
    keys, onehot = default_keys(logits, grey)
    g = refit.lovasz_pixel_gradient_cpu(logits, grey, keys=keys)
    e, fg = refit._decode_keys(keys.reshape(3, -1))
    assert (refit.lovasz_slopes_cpu(e[2], fg[2]) == 0).all()
    # C_p = 2: the class-0 slopes enter halved
    x = logits.astype(np.float64)
    q = np.exp(x - x.max(axis=0))
    q /= q.sum(axis=0)
    d = np.stack([np.where(fg[c], -1.0, 1.0) * refit.lovasz_slopes_cpu(e[c], fg[c]) / 2 for c in range(3)]).reshape(q.shape)
    assert np.allclose(g, q * (d - (d * q).sum(axis=0)), rtol=1e-13, atol=1e-18)
    T = refit.table_of("weighted_ce", WEIGHTS) / 7.0
    both = refit.lovasz_pixel_gradient_cpu(logits, grey, keys=keys, table=T, lovasz_weight=0.5)
    assert np.allclose(both, refit.pixel_gradient_cpu(logits, grey, T) + 0.5 * g, rtol=1e-13, atol=1e-18)
    only = refit.lovasz_pixel_gradient_cpu(logits, grey, table=T, lovasz_weight=0.0)
    assert np.array_equal(only, refit.pixel_gradient_cpu(logits, grey, T))
    low, mag, terms = refit.lovasz_gradient_cpu(logits, grey, 2, 3, table=T, return_abs=True)
    assert low.shape == mag.shape == terms.shape == (3, 2, 3) and (mag >= np.abs(low)).all() and (terms > 8).all()
    assert np.array_equal(refit.lovasz_gradient_cpu(logits, grey, 2, 3, table=T, lovasz_weight=0.0), refit.ce_gradient_cpu(logits, grey, 2, 3, T))
    bad = logits.copy()
    bad[1, 2, 3] = np.nan
    assert np.isnan(refit.lovasz_pixel_gradient_cpu(bad, grey)).all()
    assert np.isnan(refit.lovasz_gradient_cpu(bad, grey, 2, 3)).all()


def _rows(rng, n=4):
    rows = []
    for _ in range(n):
        fg = rng.integers(0, 3, size=3) * rng.integers(1, 40, size=3)
        fg[0] = max(fg[0], 1)
        rows.append((rng.random((3, 3)) * 100, rng.integers(1, 50, size=(3, 3)), rng.normal(size=(3, 513)),
                     np.where(fg > 0, rng.random(3), 0.0), fg))
    return rows


def test_objective_of_the_lovasz_losses():
    rng = np.random.default_rng(5)
    T = refit.table_of("mixed", WEIGHTS)
    assert np.array_equal(T, refit.table_of("weighted_ce", WEIGHTS))
    rows = _rows(rng)
    theta0 = rng.normal(size=1539).astype(np.float32)
    theta = (theta0 + rng.normal(size=1539).astype(np.float32) * 0.1).astype(np.float32)
    d = theta.astype(np.float64) - theta0.astype(np.float64)
    lov = [float(metrics.lovasz_loss(r[3], r[4])) for r in rows]
    mixed = [metrics.mixed_loss(float((T * r[0]).sum()) / int(r[1].sum()), v) for r, v in zip(rows, lov)]
    g = sum(r[2] for r in rows)
    want_grad = np.concatenate([g[:, :512].ravel(), g[:, 512]]) / len(rows) + 0.25 * d
    for loss, per_image in (("lovasz", lov), ("mixed", mixed)):
        value, data, grad = refit.objective(rows, T, 0.25, theta, theta0, loss)
        assert data == pytest.approx(sum(per_image) / len(rows), rel=1e-15)
        assert value == pytest.approx(data + 0.125 * float(d @ d), rel=1e-15)
        assert grad.shape == (1539,) and np.allclose(grad, want_grad, rtol=1e-14, atol=0)
        again = refit.objective(rows[:1] + rows[1:], T, 0.25, theta, theta0, loss)
        assert again[0] == value and again[2].tobytes() == grad.tobytes()
        with pytest.raises(ValueError):
            refit.objective([], T, 0.0, theta, theta0, loss)
    assert refit.loss_means(rows, T) == pytest.approx((sum(lov) / len(rows), sum(mixed) / len(rows)), rel=1e-15)
    # the rows of today give what they gave: the pixel-pooled objective, whether the loss is named or not
    old = [r[:3] for r in rows]
    P = sum(int(r[1].sum()) for r in old)
    for loss in refit.LOSSES:
        Tc = refit.table_of(loss, WEIGHTS)
        value, data, grad = refit.objective(old, Tc, 0.25, theta, theta0)
        assert data == sum(float((Tc * r[0]).sum()) for r in old) / P
        named = refit.objective(old, Tc, 0.25, theta, theta0, loss)
        assert named[0] == value and named[1] == data and named[2].tobytes() == grad.tobytes()


def test_command_line_and_refusals(tmp_path, capsys):
    assert refit.LOVASZ_LOSSES == ("lovasz", "mixed") and set(refit.ALL_LOSSES) == set(refit.LOSSES) | {"lovasz", "mixed"}
    assert refit.LOVASZ_ROW_WIDTH == refit.ROW_WIDTH + 6
    (tmp_path / "samples").mkdir()
    out = str(tmp_path / "out.pt")
    # the new choices parse and get as far as the folder: no sample to fit on
    for loss in ("lovasz", "mixed"):
        with pytest.raises(ValueError, match="no sample to fit on"):
            refit.refit_folder(str(tmp_path), out, "/nonexistent/ckpt.pt", image_loss=loss)
        with pytest.raises(ValueError, match="no sample to fit on"):            # the command line hands them on as image_loss
            refit.main([str(tmp_path), "--out", out, "--loss", loss, "--precision", "fp32"])
    for argv, text in [(["--loss", "focal"], "invalid choice"),
                       (["--loss", "lovasz", "--class_weights", "1", "2", "3"], "need --loss class_ce, weighted_ce or mixed"),
                       (["--loss", "ce", "--class_weights", "1", "2", "3"], "need --loss class_ce, weighted_ce or mixed"),
                       (["--loss", "mixed", "--class_weights", "1", "-2", "3"], ""),
                       (["--loss", "mixed", "--l2", "-1"], "--l2 must be"),
                       (["--loss", "lovasz", "--iterations", "0"], "--iterations")]:
        with pytest.raises(SystemExit) as e:
            refit.main([str(tmp_path), "--out", out] + argv)
        assert e.value.code == 2
        assert text in capsys.readouterr().err
    # the refusals of today still refuse: `loss` names the pixel-pooled family alone, the per-image objectives are `image_loss`
    for kw, text in [(dict(loss="focal"), "loss must be one of"), (dict(loss="lovasz"), "loss must be one of"),
                     (dict(loss="mixed"), "loss must be one of"), (dict(image_loss="ce"), "image_loss must be one of"),
                     (dict(loss="class_ce", image_loss="mixed"), "in place of loss"), (dict(image_loss="mixed", l2=-1.0), "--l2 must be"),
                     (dict(image_loss="lovasz", iterations=0), "--iterations must be"),
                     (dict(image_loss="lovasz", precision="bf16"), "fp32 or f16x2"),
                     (dict(image_loss="mixed", class_weights=(1, 2)), "three finite numbers")]:
        with pytest.raises(ValueError, match=text):
            refit.refit_folder(str(tmp_path), out, "/nonexistent/ckpt.pt", **kw)
    with pytest.raises(ValueError):
        refit.table_of("lovasz")
