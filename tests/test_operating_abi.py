"""nbc_offset_sweep and nbc_set_logit_offsets without a GPU: the symbols in the header, the signature table and the library,
the workspace formula the header states, and the argument checks that answer before any device call."""
import ctypes as C
import math
import os
import re

import pytest

from neuralbarkcalculator_amd import _lib
from neuralbarkcalculator_amd import operating as op

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("nbc_offset_sweep", "nbc_offset_sweep_workspace_bytes", "nbc_set_logit_offsets")


def _a256(x):
    return (x + 255) // 256 * 256


def _want_bytes(n, h, w, g1, g2):
    t = (h * w + 4095) // 4096
    return _a256(12 * g1 * (g2 + 1) * n * t)


def _floats(values):
    return (C.c_float * len(values))(*values)


def test_symbols_and_constants_agree(built_lib):
    header = open(os.path.join(ROOT, "include", "nbc.h")).read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    for name in NAMES:
        assert re.search(r"\b%s\s*\(" % name, code), name
        assert name in _lib.SIGNATURES and hasattr(built_lib, name), name
    assert re.search(r"#define NBC_SWEEP_MAX_GRID (\d+)", code).group(1) == "33"
    assert _lib.SWEEP_MAX_GRID == op.MAX_GRID == 33
    assert "A(12 G1 (G2 + 1) N T) bytes" in header               # the formula this file checks is the one the header states


def test_workspace_formula_holds(built_lib):
    f = built_lib.nbc_offset_sweep_workspace_bytes
    for n, h, w in [(1, 1, 1), (1, 4096, 1), (1, 4097, 1), (3, 67, 131), (8, 1024, 1024), (65535, 1, 1), (1, 46340, 46340)]:
        for g1, g2 in [(1, 1), (33, 33), (1, 33), (33, 1), (5, 3)]:
            assert f(n, h, w, g1, g2) == _want_bytes(n, h, w, g1, g2) > 0, (n, h, w, g1, g2)
    assert f(1, 4096, 1, 33, 33) == 13568 and f(1, 4097, 1, 33, 33) == 27136 and f(1, 1, 1, 1, 1) == 256
    for n, h, w in [(0, 8, 8), (-1, 8, 8), (65536, 8, 8), (1, 0, 8), (1, 8, 0), (1, 65536, 32768)]:
        assert f(n, h, w, 33, 33) == 0, (n, h, w)
    for g1, g2 in [(0, 1), (1, 0), (34, 1), (1, 34), (-1, 5)]:
        assert f(1, 64, 64, g1, g2) == 0, (g1, g2)


def test_every_invalid_argument_is_refused_before_the_device_is_touched(built_lib):
    """Fake but aligned device addresses: each call must return NBC_ERR_INVALID from its argument checks alone."""
    fake = 1 << 40
    n, h, w = 2, 16, 16
    grid = [-1.0, 0.0, 0.5]
    need = built_lib.nbc_offset_sweep_workspace_bytes(n, h, w, 3, 3)

    def call(logits=fake, target=fake, N=n, H=h, W=w, b1=grid, G1=None, b2=grid, G2=None, ws=fake, ws_bytes=need, conf=fake):
        p1 = None if b1 is None else _floats(b1)
        p2 = None if b2 is None else _floats(b2)
        return built_lib.nbc_offset_sweep(logits, target, N, H, W, p1, len(b1) if G1 is None else G1, p2,
                                          len(b2) if G2 is None else G2, ws, ws_bytes, conf, None)

    long = [float(i) for i in range(34)]
    bad = [dict(logits=None), dict(target=None), dict(ws=None), dict(conf=None), dict(b1=None, G1=3), dict(b2=None, G2=3),
           dict(N=0), dict(N=-3), dict(N=65536), dict(H=0), dict(W=-1), dict(H=65536, W=32768),
           dict(G1=0), dict(G2=0), dict(b1=long), dict(b2=long), dict(G1=-1),
           dict(b1=[1.0, 0.0, 2.0]), dict(b2=[0.0, 1.0, 0.5]), dict(b1=[0.0, 0.0, 1.0]), dict(b2=[0.0, 1.0, 1.0]),
           dict(b1=[0.0, math.nan, 1.0]), dict(b2=[math.nan, 0.0, 1.0]), dict(b1=[0.0, 1.0, math.inf]), dict(b2=[-math.inf, 0.0, 1.0]),
           dict(ws_bytes=need - 1), dict(ws_bytes=0), dict(ws=fake + 8)]
    for kw in bad:
        assert call(**kw) == _lib.NBC_ERR_INVALID, kw
        assert _lib.last_error().startswith("nbc_offset_sweep:"), kw


def test_set_logit_offsets_refuses_what_is_not_finite(built_lib):
    """The values are checked before the context is looked at, so the refusal shows without a device."""
    for pair in ((math.nan, 0.0), (0.0, math.inf), (-math.inf, 1.0), (math.nan, math.nan)):
        assert built_lib.nbc_set_logit_offsets(None, *pair) == _lib.NBC_ERR_INVALID, pair
        assert _lib.last_error() == "nbc_set_logit_offsets: the offsets must be finite", pair
    assert built_lib.nbc_set_logit_offsets(None, 1.5, -5.5) == _lib.NBC_ERR_INVALID
    assert _lib.last_error() == "nbc_set_logit_offsets: null context"
    from neuralbarkcalculator_amd.model import FCNResNet50
    m = FCNResNet50("fp32")                                      # no context yet: the pair is held for `to`
    for pair in ((math.nan, 0.0), (0.0, math.inf), (-math.inf, 1.0)):
        with pytest.raises(ValueError):
            m.set_logit_offsets(*pair)
    assert m.logit_offsets() == (0.0, 0.0)
    assert m.set_logit_offsets(1.5, -5.5).logit_offsets() == (1.5, -5.5)
    assert m.set_logit_offsets(0, 0).logit_offsets() == (0.0, 0.0)
