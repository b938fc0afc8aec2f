"""The row-step 3x3 kernel's f16x2 arithmetic (the low-piece products P X1 summed apart, unscaled, joined once with 2^-11:
tests/helpers/rowstep_low_sum.py) against float64 on the CPU: every element within the bound of tests/helpers/f32_grade_bound.py
at c = 1, the bound the suite holds the device to at c = 2, left as it is.  Two units on a 3 x 8 map: K = 1 152 (layer2's conv2)
and K = 4 608 (layer4's, dilated), with weights below 2^-3 at the row's scale among them -- the weights whose scaled high piece
P 2^-11 was an f16 subnormal in the loop and is not formed any more."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import f32_grade_bound as fb  # noqa: E402
import rowstep_low_sum as rl  # noqa: E402

COUT, H, W = 5, 3, 8


def make_unit(cin, seed):
    rng = np.random.default_rng(seed)
    w = (rng.standard_normal((COUT, cin, 3, 3)) / np.sqrt(9 * cin)).astype(np.float32)
    small = rng.random(w.shape) < 0.125                  # 2^-19 ... 2^-23 of their size: |P| < 2^-3 at any row's scale
    w = np.where(small, np.ldexp(w, -rng.integers(19, 24, w.shape)), w).astype(np.float32)
    x = rng.standard_normal((1, cin, H, W)).astype(np.float32)
    x = np.where(rng.random(x.shape) < 0.4, np.float32(0), np.abs(x)).astype(np.float32)      # behind a ReLU
    x = fb.join16(*fb.split16(x))                        # as stored
    alpha = rng.uniform(0.5, 2.0, COUT).astype(np.float32) * np.where(rng.random(COUT) < 0.3, -1, 1).astype(np.float32)
    beta = rng.uniform(-0.5, 0.5, COUT).astype(np.float32)
    return x, w, alpha, beta


def test_kstep_order_is_channel_block_kh_kw():
    idx = rl.kstep_indices(128)
    assert len(idx) == 36 and sorted(np.concatenate(idx).tolist()) == list(range(1152))
    assert idx[0][0] == 0 and idx[1][0] == 128 and idx[3][0] == 3 * 128 and idx[9][0] == 32      # kw, kh, then the channel block


@pytest.mark.parametrize("cin,dil,relu", [(128, 1, True), (512, 2, True), (128, 1, False)], ids=["K1152", "K4608-dil2", "K1152-linear"])
def test_every_element_within_the_bound_at_c_1(cin, dil, relu):
    x, w, alpha, beta = make_unit(cin, 11 + cin + dil)
    K = 9 * cin
    y_ref, mag, tiny = fb.conv_unit_reference(x, w, "f16x2", alpha, beta, None, relu, 1, dil, dil)
    p = fb.f16x2_pieces(w)[0].astype(np.float32)
    share = float(((np.abs(p) < 2.0 ** -3) & (p != 0)).mean())
    assert tiny is not None and share >= 0.05, share      # weights with 0 < |P| < 2^-3 take part
    assert (fb.split16(x)[1] != 0).mean() >= 0.25         # and the low-piece products are not all zero
    got = rl.emulate_unit(x, w, alpha, beta, relu, dil)
    assert got.shape == y_ref.shape == (1, COUT, H, W) and np.isfinite(got).all()
    err = np.abs(got.astype(np.float64) - y_ref)
    r = err / fb.unit_bound("f16x2", y_ref, mag, tiny, alpha, beta, None, K, 0, c=1)
    print("K %d dil %d: worst %.4f of the bound (c = 1); weights with 0 < |P| < 2^-3: %.3f" % (K, dil, float(r.max()), share))
    assert float(r.max()) <= 1.0, (K, float(r.max()))

