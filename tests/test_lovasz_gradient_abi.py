"""nbc_lovasz_gradient's C ABI without a GPU: the symbols and signatures, the workspace formula include/nbc.h states, and
every refusal in front of the device."""
import ctypes as C
import os
import re

import pytest

from neuralbarkcalculator_amd import _lib
from neuralbarkcalculator_amd import model as mdl

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAKE = 1 << 40                                     # a "device pointer": 256-byte aligned, never dereferenced by a refusal
WHO = "nbc_lovasz_gradient"
A = lambda x: (x + 255) & ~255


def test_symbols_and_signatures(built_lib):
    header = open(os.path.join(REPO, "include", "nbc.h")).read()
    flat = re.sub(r"\s+", " ", header)
    for name in (WHO, WHO + "_workspace_bytes"):
        assert name in _lib.SIGNATURES and hasattr(built_lib, name) and (" %s(" % name) in flat
    assert "size_t nbc_lovasz_gradient_workspace_bytes(int N, int H, int W, int h, int w);" in flat
    assert ("const double* table9_host, double lovasz_weight, void* workspace_dev, size_t workspace_bytes, double* terms_dev, "
            "int64_t* fg_counts_dev, double* grad_lowres_dev, uint32_t* keys_dev, double* pixel_grad_dev, void* hip_stream);") in flat
    restype, args = _lib.SIGNATURES[WHO]
    assert restype is C.c_int and len(args) == 25 and args[16] is C.c_double and args[15] == C.POINTER(C.c_double)
    assert "nbc_lovasz_workspace_bytes(N, H, W) + 2 A(12 N P) + A(24 N P) + A(24 N H w)" in flat
    assert "the Lovasz-Softmax gradient and the DeepLab" not in flat          # no longer on the left-out list


@pytest.mark.parametrize("shape", [(1, 1, 1, 1, 1), (2, 24, 40, 3, 5), (3, 3, 2731, 1, 342), (3, 203, 317, 26, 40), (8, 1024, 1024, 128, 128),
                                   (1, 3, 3, 3, 3)])
def test_workspace_formula(built_lib, shape):
    N, H, W, h, w = shape
    P = H * W
    want = built_lib.nbc_lovasz_workspace_bytes(N, H, W) + 2 * A(12 * N * P) + A(24 * N * P) + A(24 * N * H * w)
    assert built_lib.nbc_lovasz_workspace_bytes(N, H, W) > 0
    assert built_lib.nbc_lovasz_gradient_workspace_bytes(N, H, W, h, w) == want


def test_refusals_come_before_the_device(built_lib):
    """No GPU is here: a call that got past its argument check would fail in its first HIP call (NBC_ERR_HIP) or crash, so a
    refusal with NBC_ERR_INVALID and its message is a refusal in front of the device; a call that passes the check is not made."""
    table = (C.c_double * 9)(*([1.0] * 9))
    N, H, W, h, w = 2, 24, 40, 3, 5
    need = built_lib.nbc_lovasz_gradient_workspace_bytes(N, H, W, h, w)
    assert need > 0
    ptr = lambda k: FAKE + (k << 32)
    required = ["logits", "target", "row_idx", "row_coeff", "row_lo", "row_hi", "col_idx", "col_coeff", "col_lo", "col_hi", "ws", "terms",
                "fg", "out"]
    names = required + ["keys", "pix"]

    def call(N=N, H=H, W=W, h=h, w=w, table=table, lam=1.0, bytes_=need, **over):
        p = {name: ptr(k) for k, name in enumerate(names)}
        p.update(over)
        return built_lib.nbc_lovasz_gradient(p["logits"], p["target"], N, H, W, h, w, p["row_idx"], p["row_coeff"], p["row_lo"],
                                             p["row_hi"], p["col_idx"], p["col_coeff"], p["col_lo"], p["col_hi"], table, lam, p["ws"],
                                             bytes_, p["terms"], p["fg"], p["out"], p["keys"], p["pix"], None)

    def refused(rc, text):
        err = _lib.last_error()
        assert rc == _lib.NBC_ERR_INVALID and err.startswith(WHO + ":") and text in err, (rc, err, text)
    for name in required:
        refused(call(**{name: None}), "null argument")
    for kw in (dict(N=0), dict(N=65536), dict(H=0), dict(W=-1), dict(H=65536, W=32768, h=1, w=1), dict(h=0), dict(w=0),
               dict(h=H + 1), dict(w=W + 1)):
        refused(call(**kw), "bad shape")
        shape = dict(dict(N=N, H=H, W=W, h=h, w=w), **kw)
        assert built_lib.nbc_lovasz_gradient_workspace_bytes(*[shape[k] for k in "NHWhw"]) == 0
    for lam in (float("nan"), float("inf"), -float("inf")):
        refused(call(lam=lam), "lovasz_weight must be finite")
    for name in ("row_idx", "row_coeff", "col_idx", "col_coeff"):
        for off in (4, 8):
            refused(call(**{name: ptr(3) + off}), "16-byte aligned")
    for name in ("logits", "row_lo", "row_hi", "col_lo", "col_hi"):
        refused(call(**{name: ptr(2) + 2}), "4-byte aligned")
    for name in ("terms", "fg", "out", "pix"):
        refused(call(**{name: ptr(11) + 4}), "8-byte aligned")
    refused(call(keys=ptr(14) + 2), "keys_dev must be 4-byte aligned")
    refused(call(bytes_=need - 1), "workspace of")
    refused(call(ws=ptr(10) + 128), "256-byte aligned")
    # the nullable ones, null, get as far as the workspace check
    refused(call(table=None, keys=None, pix=None, bytes_=0), "workspace of")
    assert built_lib.nbc_lovasz_gradient_workspace_bytes(1, 8, 8, 8, 8) > 0              # h == H and w == W are inside


def test_model_method_refuses_without_a_device(built_lib):
    import torch
    m = mdl.FCNResNet50("fp32")
    with pytest.raises(RuntimeError):
        m.lovasz_gradient(torch.zeros((1, 3, 64, 96)), torch.zeros((1, 64, 96), dtype=torch.uint8), (8, 12))
