"""A numpy restatement of the flip views (include/nbc.h: nbc_tta_views, nbc_tta_merge), written from the
definition alone: the views of a mask in ascending bit order, the view-major stack, the un-flipping, and the f32 mean in the
stated order -- adds in view order, one division by float32(V).  The views' own figures go through vote_oracle."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import vote_oracle as vo  # noqa: E402

IDENTITY, HFLIP, VFLIP, HVFLIP, FLIPS = 1, 2, 4, 8, 15
NAMED = {"hflip": 3, "vflip": 5, "flips": 15}


def view_bits(mask):
    """The bit numbers (0..3) of the views of a mask, in the order of the stack."""
    assert 1 <= int(mask) <= 15
    return [b for b in range(4) if (int(mask) >> b) & 1]


def mirrors(bit):
    """(rows mirrored, columns mirrored) of view bit 0..3: identity, hflip (columns), vflip (rows), both."""
    return bit in (2, 3), bit in (1, 3)


def flip(a, bit, row_axis, col_axis):
    rows, cols = mirrors(bit)
    if rows:
        a = np.flip(a, axis=row_axis)
    if cols:
        a = np.flip(a, axis=col_axis)
    return a


def stack(x, mask):
    """x: uint8 [N,H,W,3] or float32 [N,3,H,W] -> the stack [V*N, ...], entry j * N + i = view j of image i."""
    x = np.asarray(x)
    row_axis, col_axis = (1, 2) if x.dtype == np.uint8 else (2, 3)
    return np.ascontiguousarray(np.concatenate([flip(x, b, row_axis, col_axis) for b in view_bits(mask)]))


def align(lowres_views, n, mask):
    """float32 [V*N,3,h,w] (view j in view j's orientation) -> the un-flipped views [V,N,3,h,w].  A flip is its own inverse."""
    bits = view_bits(mask)
    v = np.asarray(lowres_views).reshape((len(bits), n) + tuple(lowres_views.shape[-3:]))
    return np.ascontiguousarray(np.stack([flip(v[j], b, 2, 3) for j, b in enumerate(bits)]))


def merge(aligned):
    """[V,N,3,h,w] float32 -> m = (((a_0 + a_1) + a_2) + a_3) / float32(V), every operation rounded to f32 on its own; V = 1
    is the view itself."""
    aligned = np.asarray(aligned, dtype=np.float32)
    s = aligned[0].copy()
    if aligned.shape[0] == 1:
        return s
    with np.errstate(all="ignore"):                  # inf - inf and overflow are part of the definition: NaN and inf
        for j in range(1, aligned.shape[0]):
            s = (s + aligned[j]).astype(np.float32)
        return (s / np.float32(aligned.shape[0])).astype(np.float32)


def view_figures(view_labels):
    """The views' final label maps uint8 [V,N,H,W] -> (counts int64 [V,N,3], support uint8 [N,H,W], stats int64 [N,10]) with
    D = V, through vote_oracle."""
    view_labels = np.asarray(view_labels)
    v = view_labels.shape[0]
    counts = np.stack([[np.bincount(img.reshape(-1), minlength=3)[:3] for img in view_labels[j]] for j in range(v)]).astype(np.int64)
    words = vo.tally(view_labels)
    _, support, _, _ = vo.decode(words, v)
    return counts, support, vo.stats(words, v)
