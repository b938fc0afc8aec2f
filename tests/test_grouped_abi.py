"""The two grouped entry points without a GPU: symbols, header text, the workspace formula, and every argument refusal --
NBC_ERR_INVALID (or 0 bytes from the workspace query) before any HIP call, with fake device addresses."""
import os

import pytest

from neuralbarkcalculator_amd import _lib

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAKE = 1 << 40


def _a256(x):
    return (x + 255) // 256 * 256


def _want_bytes(n, h, w, g):
    p, ng, gl = h * w, (n + g - 1) // g, min(g, n)
    s, t = 3 * ng, (gl * p + 8191) // 8192
    return 2 * _a256(12 * n * p) + _a256(1024 * s * t) + _a256(1024 * s) + _a256(4 * s * t) + _a256(8 * s * t) + _a256(4 * ng)


def test_symbols_and_header():
    for name in ("nbc_lovasz_groups_workspace_bytes", "nbc_lovasz_softmax_groups", "nbc_remove_small_zones_groups"):
        assert name in _lib.SIGNATURES
    header = " ".join(open(os.path.join(REPO, "include", "nbc.h")).read().split())
    assert "size_t nbc_lovasz_groups_workspace_bytes(int N, int H, int W, int G);" in header
    assert ("int nbc_lovasz_softmax_groups(const float* logits_full_dev, const uint8_t* target_dev, int N, int H, int W, int G, "
            "void* workspace_dev, size_t workspace_bytes, double* terms_dev, int64_t* counts_dev, void* hip_stream);") in header
    assert ("int nbc_remove_small_zones_groups(nbc_ctx* ctx, void* labels_dev, int labels_dtype, int N, int H, int W, int G, "
            "int min_pixels, int64_t* counts_dev, void* hip_stream);") in header


def test_workspace_formula_and_what_the_query_refuses(built_lib):
    for n, h, w, g in [(1, 1, 1, 1), (5, 33, 65, 2), (5, 203, 317, 8), (8, 1024, 1024, 8), (7, 1, 7, 3), (64, 128, 128, 64),
                       (130, 16, 16, 64), (3, 8192, 1, 2), (65535, 1, 1, 64), (1, 46340, 46340, 64), (2, 46340, 23170, 2)]:
        assert built_lib.nbc_lovasz_groups_workspace_bytes(n, h, w, g) == _want_bytes(n, h, w, g), (n, h, w, g)
        if g == 1:
            assert built_lib.nbc_lovasz_groups_workspace_bytes(n, h, w, 1) == built_lib.nbc_lovasz_workspace_bytes(n, h, w)
    for n, h, w in [(1, 7, 9), (4, 33, 65), (8, 1024, 1024)]:                            # G = 1: the per-image layout
        assert built_lib.nbc_lovasz_groups_workspace_bytes(n, h, w, 1) == built_lib.nbc_lovasz_workspace_bytes(n, h, w)
    for n, h, w, g in [(0, 8, 8, 1), (-1, 8, 8, 2), (65536, 8, 8, 2), (1, 0, 8, 1), (1, 8, 0, 1), (1, 65536, 32768, 1),
                       (4, 8, 8, 0), (4, 8, 8, -1), (4, 8, 8, 65), (2, 46341, 23171, 2), (8, 16384, 16384, 8), (64, 8192, 4096, 64)]:
        assert built_lib.nbc_lovasz_groups_workspace_bytes(n, h, w, g) == 0, (n, h, w, g)
    # the volume that counts is the group's, not the batch's: 9 images of 2^28 pixels in groups of 7 fit, in groups of 8 do not
    assert built_lib.nbc_lovasz_groups_workspace_bytes(9, 16384, 16384, 7) > 0
    assert built_lib.nbc_lovasz_groups_workspace_bytes(9, 16384, 16384, 8) == 0
    assert built_lib.nbc_lovasz_groups_workspace_bytes(7, 16384, 16384, 64) > 0         # g = min(G, N)


def test_lovasz_groups_refuses_before_the_device_is_touched(built_lib):
    n, h, w, g = 5, 16, 16, 2
    need = built_lib.nbc_lovasz_groups_workspace_bytes(n, h, w, g)

    def call(logits=FAKE, target=FAKE, N=n, H=h, W=w, G=g, ws=FAKE, ws_bytes=need, terms=FAKE, counts=FAKE):
        return built_lib.nbc_lovasz_softmax_groups(logits, target, N, H, W, G, ws, ws_bytes, terms, counts, None)

    bad = [dict(logits=None), dict(target=None), dict(ws=None), dict(terms=None), dict(counts=None),
           dict(N=0), dict(N=-3), dict(N=65536), dict(H=0), dict(W=-1), dict(H=65536, W=32768),          # the per-image refusals
           dict(G=0), dict(G=-1), dict(G=65), dict(N=8, H=16384, W=16384, G=8, ws_bytes=1 << 62),          # g H W >= 2^31
           dict(ws_bytes=need - 1), dict(ws_bytes=0), dict(ws=FAKE + 8)]
    for kw in bad:
        assert call(**kw) == _lib.NBC_ERR_INVALID, kw
        assert _lib.last_error().startswith("nbc_lovasz_softmax_groups:"), kw
    # a workspace that serves G = 1 is too small for nothing, one sized for fewer images is
    assert call(ws_bytes=built_lib.nbc_lovasz_groups_workspace_bytes(n - 1, h, w, g)) == _lib.NBC_ERR_INVALID


def test_zones_groups_refuses_before_the_device_is_touched(built_lib):
    def call(ctx=FAKE, labels=FAKE, dtype=_lib.LABEL_U8, N=4, H=64, W=64, G=2, min_pixels=150, counts=None):
        return built_lib.nbc_remove_small_zones_groups(ctx, labels, dtype, N, H, W, G, min_pixels, counts, None)

    bad = [dict(ctx=None), dict(labels=None), dict(dtype=7), dict(dtype=-1),
           dict(N=0), dict(N=-2), dict(N=65536), dict(H=0), dict(W=0), dict(min_pixels=-1), dict(H=65536, W=8), dict(H=65535, W=65535),
           dict(G=0), dict(G=-1), dict(G=65), dict(N=8, H=16384, W=16384, G=8), dict(N=2, H=46341, W=23171, G=2)]
    for kw in bad:
        assert call(**kw) == _lib.NBC_ERR_INVALID, kw
        assert _lib.last_error().startswith("nbc_remove_small_zones_groups:"), kw
    # the order of the refusals: null argument, shape, group, dtype
    for kw, text in [(dict(labels=None, N=0, G=0, dtype=7), "null argument"), (dict(N=0, G=0, dtype=7), "bad shape"),
                     (dict(G=0, dtype=7), "bad group: 1 <= G <= 64 and g * H * W < 2^31 for the g = min(G, N) images of a group"),
                     (dict(dtype=7), "bad labels_dtype")]:
        assert call(**kw) == _lib.NBC_ERR_INVALID, kw
        assert _lib.last_error() == "nbc_remove_small_zones_groups: " + text, kw


def test_remove_small_zones_refuses_before_the_context_is_read(built_lib):
    """The per-image entry point with a fake context: every refusal by its whole text, in the order null argument, shape, dtype."""
    def call(ctx=FAKE, labels=FAKE, dtype=_lib.LABEL_I64, N=2, H=64, W=64, min_pixels=150):
        return built_lib.nbc_remove_small_zones(ctx, labels, dtype, N, H, W, min_pixels, 0, None, None)

    for kw, text in [(dict(ctx=None), "null argument"), (dict(labels=None), "null argument"), (dict(labels=None, N=0, dtype=7), "null argument"),
                     (dict(N=0), "bad shape"), (dict(N=65536), "bad shape"), (dict(H=0), "bad shape"), (dict(W=-1), "bad shape"),
                     (dict(min_pixels=-1), "bad shape"), (dict(N=0, dtype=7), "bad shape"),
                     (dict(dtype=7), "bad labels_dtype"), (dict(dtype=-1), "bad labels_dtype")]:
        assert call(**kw) == _lib.NBC_ERR_INVALID, kw
        assert _lib.last_error() == "nbc_remove_small_zones: " + text, kw
