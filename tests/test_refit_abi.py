"""The classifier.4 refit's C ABI without a GPU: symbols and signatures, nbc_bicubic_taps against its host restatement and the
float64 closed form, and every refusal of nbc_head_logits, nbc_ce_gradient and nbc_head_gradient in front of the device."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from neuralbarkcalculator_amd import _lib, refit
from neuralbarkcalculator_amd import model as mdl

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAKE = 1 << 40                                     # a "device pointer": 256-byte aligned, never dereferenced by a refusal
I32, F32 = C.POINTER(C.c_int32), C.POINTER(C.c_float)
PAIRS = [(1, 8), (3, 24), (5, 40), (8, 64), (12, 96), (3, 17), (4, 23), (26, 203), (40, 317), (128, 1024)]
NEW = ("nbc_head_logits", "nbc_bicubic_taps", "nbc_ce_gradient_workspace_bytes", "nbc_ce_gradient", "nbc_head_gradient_workspace_bytes",
       "nbc_head_gradient")


def test_symbols_and_signatures(built_lib):
    header = open(os.path.join(REPO, "include", "nbc.h")).read()
    flat = re.sub(r"\s+", " ", header)
    for name in NEW:
        assert name in _lib.SIGNATURES and hasattr(built_lib, name) and (" %s(" % name) in flat
    assert _lib.SIGNATURES["nbc_bicubic_taps"] == (C.c_int, [C.c_int, C.c_int, I32, F32, I32, I32])
    assert "int nbc_bicubic_taps(int in_size, int out_size, int32_t* idx, float* coeff, int32_t* lo, int32_t* hi);" in flat
    assert ("int nbc_head_logits(nbc_ctx* ctx, const float* theta_dev, int N, int H, int W, float* logits_lowres_dev, "
            "void* hip_stream);") in flat
    assert "size_t nbc_ce_gradient_workspace_bytes(int N, int H, int W, int h, int w);" in flat
    assert "size_t nbc_head_gradient_workspace_bytes(int N, int H, int W);" in flat
    assert len(_lib.SIGNATURES["nbc_ce_gradient"][1]) == 20 and len(_lib.SIGNATURES["nbc_head_gradient"][1]) == 9
    assert "head_refit.hip" in __import__("neuralbarkcalculator_amd.build", fromlist=["SOURCES"]).SOURCES
    for cite in ("utils.py:151-165", "models.py:121", "DESIGN.md 3.22"):
        assert cite in header


def _closed_form(n_in, n_out):
    """The cubic-convolution weights (A = -0.75) of every output's four taps in float64."""
    s = (n_in / n_out) * (np.arange(n_out) + 0.5) - 0.5
    i0 = np.minimum(np.floor(s), n_in - 1)
    t = np.clip(s - i0, 0.0, 1.0)
    A = -0.75

    def near(x):                                   # |x| <= 1
        return ((A + 2) * x - (A + 3)) * x * x + 1

    def far(x):                                    # 1 < |x| < 2
        return ((A * x - 5 * A) * x + 8 * A) * x - 4 * A
    return np.stack([far(t + 1), near(t), near(1 - t), far(2 - t)], axis=1), i0.astype(np.int64)


@pytest.mark.parametrize("pair", PAIRS)
def test_bicubic_taps(built_lib, pair):
    n_in, n_out = pair
    idx, coeff, lo, hi = mdl.bicubic_taps(n_in, n_out)
    want = refit.bicubic_taps_cpu(n_in, n_out)
    assert idx.dtype == lo.dtype == hi.dtype == np.int32 and coeff.dtype == np.float32
    assert idx.shape == coeff.shape == (n_out, 4) and lo.shape == hi.shape == (n_in,)
    np.testing.assert_array_equal(idx, want[0])
    np.testing.assert_array_equal(lo, want[2])
    np.testing.assert_array_equal(hi, want[3])
    # every output lies in lo .. hi of each of its four taps, and in no other input's range
    touched = np.zeros((n_in, n_out), dtype=bool)
    touched[idx.ravel(), np.repeat(np.arange(n_out), 4)] = True
    ranged = (np.arange(n_out)[None, :] >= lo[:, None]) & (np.arange(n_out)[None, :] <= hi[:, None])
    np.testing.assert_array_equal(touched, ranged)
    # the f32 t carries at most 2^-17 at s < 128, a coefficient's slope in t is below 2, and its own evaluation adds a few
    # 2^-24 of magnitudes below 8
    # (compared per input, as the weight output o puts on input i: where s lies within rounding of an integer the two
    # precisions may name the cell differently, with t near 1 in the one and near 0 in the other, and mean the same weights)
    closed, i0 = _closed_form(n_in, n_out)
    want_w = np.zeros((n_in, n_out))
    np.add.at(want_w, (np.clip(i0[:, None] + np.arange(-1, 3)[None, :], 0, n_in - 1).ravel(), np.repeat(np.arange(n_out), 4)), closed.ravel())
    got_w = np.zeros((n_in, n_out))
    np.add.at(got_w, (idx.ravel(), np.repeat(np.arange(n_out), 4)), coeff.astype(np.float64).ravel())
    assert np.abs(got_w - want_w).max() <= 2.0 ** -14
    assert np.abs(coeff.astype(np.float64).sum(axis=1) - 1.0).max() <= 2.0 ** -20
    assert np.abs(coeff - want[1]).max() <= 2.0 ** -20           # the numpy restatement rounds as the library does


def test_taps_refusals(built_lib):
    idx, coeff, lo, hi = (C.c_int32 * 32)(), (C.c_float * 32)(), (C.c_int32 * 8)(), (C.c_int32 * 8)()

    def refused(rc, text):
        err = _lib.last_error()
        assert rc == _lib.NBC_ERR_INVALID and err.startswith("nbc_bicubic_taps:") and text in err, (rc, err)
    for k in range(4):
        args = [idx, coeff, lo, hi]
        args[k] = None
        refused(built_lib.nbc_bicubic_taps(2, 8, *args), "null argument")
    for n_in, n_out in ((0, 8), (2, 0), (-1, 8), ((1 << 24) + 1, 8), (2, (1 << 24) + 1)):
        refused(built_lib.nbc_bicubic_taps(n_in, n_out, idx, coeff, lo, hi), "1..2^24")
    assert built_lib.nbc_bicubic_taps(2, 8, idx, coeff, lo, hi) == _lib.NBC_OK
    # an input no output touches (more inputs than outputs): lo = 0, hi = -1
    t = mdl.bicubic_taps(64, 2)
    assert ((t[3] == -1) == (t[2] > t[3])).all() and (t[3] == -1).any() and (t[2][t[3] == -1] == 0).all()
    for bad in ((0, 8), (None, 8), ("a", 8), (2, 2 ** 24 + 1)):
        with pytest.raises(ValueError):
            mdl.bicubic_taps(*bad)


def _refused(rc, who, text):
    err = _lib.last_error()
    assert rc == _lib.NBC_ERR_INVALID and err.startswith(who + ":") and text in err, (rc, err, text)


def test_ce_gradient_refusals_come_before_the_device(built_lib):
    """No GPU is here: a call that got past its argument check would fail in the launch (NBC_ERR_HIP) or crash, so a refusal
    with NBC_ERR_INVALID and its message is a refusal in front of the device; a call that passes the check is not made."""
    table = (C.c_double * 9)(*([1.0] * 9))
    N, H, W, h, w = 2, 24, 40, 3, 5
    need = built_lib.nbc_ce_gradient_workspace_bytes(N, H, W, h, w)
    A = lambda x: (x + 255) & ~255
    assert need == A(24 * N * H * W) + A(24 * N * H * w)
    assert built_lib.nbc_ce_gradient_workspace_bytes(1, 3, 3, 1, 1) == A(24 * 10) + A(24 * 3)     # P rounded up to even
    ptr = lambda k: FAKE + (k << 32)
    names = ["logits", "target", "row_idx", "row_coeff", "row_lo", "row_hi", "col_idx", "col_coeff", "col_lo", "col_hi", "ws", "out"]

    def call(N=N, H=H, W=W, h=h, w=w, table=table, bytes_=need, **over):
        p = {name: ptr(k) for k, name in enumerate(names)}
        p.update(over)
        return built_lib.nbc_ce_gradient(p["logits"], p["target"], N, H, W, h, w, p["row_idx"], p["row_coeff"], p["row_lo"], p["row_hi"],
                                         p["col_idx"], p["col_coeff"], p["col_lo"], p["col_hi"], table, p["ws"], bytes_, p["out"], None)
    who = "nbc_ce_gradient"
    for name in names:
        _refused(call(**{name: None}), who, "null argument")
    _refused(call(table=None), who, "null argument")
    for kw in (dict(N=0), dict(N=65536), dict(H=0), dict(W=-1), dict(H=65536, W=32768, h=1, w=1), dict(h=0), dict(w=0),
               dict(h=H + 1), dict(w=W + 1)):
        _refused(call(**kw), who, "bad shape")
        shape = dict(dict(N=N, H=H, W=W, h=h, w=w), **kw)
        assert built_lib.nbc_ce_gradient_workspace_bytes(*[shape[k] for k in "NHWhw"]) == 0
    for name in ("row_idx", "row_coeff", "col_idx", "col_coeff"):
        for off in (4, 8):
            _refused(call(**{name: ptr(3) + off}), who, "16-byte aligned")
    for name in ("logits", "row_lo", "row_hi", "col_lo", "col_hi"):
        _refused(call(**{name: ptr(2) + 2}), who, "4-byte aligned")
    _refused(call(out=ptr(11) + 4), who, "8-byte aligned")
    _refused(call(bytes_=need - 1), who, "workspace of")
    _refused(call(ws=ptr(10) + 128), who, "256-byte aligned")
    # h == H and w == W are inside
    assert built_lib.nbc_ce_gradient_workspace_bytes(1, 8, 8, 8, 8) > 0


def test_head_entries_refuse_before_the_device(built_lib):
    ctx = C.create_string_buffer(1 << 16)             # never read by a refusal: the argument checks come first
    cp = C.cast(ctx, C.c_void_p)
    who = "nbc_head_logits"
    for args in ((None, FAKE, FAKE + 64), (cp, None, FAKE + 64), (cp, FAKE, None)):
        _refused(built_lib.nbc_head_logits(args[0], args[1], 1, 64, 96, args[2], None), who, "null argument")
    _refused(built_lib.nbc_head_logits(cp, FAKE + 2, 1, 64, 96, FAKE + 64, None), who, "4-byte aligned")
    _refused(built_lib.nbc_head_logits(cp, FAKE, 1, 64, 96, FAKE + 65, None), who, "4-byte aligned")
    for n, h, w in ((0, 64, 96), (65536, 64, 96), (1, 0, 96), (1, 64, -1), (1, 65536, 32768)):
        _refused(built_lib.nbc_head_logits(cp, FAKE, n, h, w, FAKE + 64, None), who, "bad shape")
        assert built_lib.nbc_head_gradient_workspace_bytes(n, h, w) == 0
    who = "nbc_head_gradient"
    N, H, W = 3, 203, 317
    need = built_lib.nbc_head_gradient_workspace_bytes(N, H, W)
    assert need == ((8 * 1539 * N * ((26 * 40 + 63) // 64)) + 255) & ~255
    out, g, ws = FAKE + (1 << 32), FAKE, FAKE + (2 << 32)
    for args in ((None, g, ws, out), (cp, None, ws, out), (cp, g, None, out), (cp, g, ws, None)):
        _refused(built_lib.nbc_head_gradient(args[0], args[1], N, H, W, args[2], need, args[3], None), who, "null argument")
    _refused(built_lib.nbc_head_gradient(cp, g + 4, N, H, W, ws, need, out, None), who, "8-byte aligned")
    _refused(built_lib.nbc_head_gradient(cp, g, N, H, W, ws, need, out + 4, None), who, "8-byte aligned")
    for n, h, w in ((0, H, W), (65536, H, W), (N, 0, W), (N, 65536, 32768)):
        _refused(built_lib.nbc_head_gradient(cp, g, n, h, w, ws, need, out, None), who, "bad shape")
    _refused(built_lib.nbc_head_gradient(cp, g, N, H, W, ws, need - 1, out, None), who, "workspace of")
    _refused(built_lib.nbc_head_gradient(cp, g, N, H, W, ws + 64, need, out, None), who, "256-byte aligned")


def test_model_methods_refuse_without_a_device(built_lib):
    import torch
    m = mdl.FCNResNet50("fp32")
    with pytest.raises(RuntimeError):
        m.head_logits(np.zeros(1539, np.float32))
    with pytest.raises(RuntimeError):
        m.head_gradient(torch.zeros((1, 3, 8, 12), dtype=torch.float64))
    with pytest.raises(RuntimeError):
        m.ce_gradient(torch.zeros((1, 3, 64, 96)), torch.zeros((1, 64, 96), dtype=torch.uint8), (8, 12), np.ones(9))
