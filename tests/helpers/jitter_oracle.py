"""A numpy restatement of the colour-jitter views (include/nbc.h: nbc_jitter_views, nbc_views_mean), written
from the definition alone: a view is saturation_s(contrast_c(brightness_b(frame))) on uint8, each step
blend(degenerate, image, f) = float32(d) + f * float32(i - d) clamped to 0..255 and truncated; the view-major stack; and the
f32 mean in the stated order -- adds in view order, one division by float32(V).  The views' own figures go through
vote_oracle."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import vote_oracle as vo  # noqa: E402

TRAINING = ((1.0, 1.0, 1.0), (0.9, 1.0, 1.0), (1.1, 1.0, 1.0), (1.0, 1.0, 0.8), (1.0, 1.0, 1.2))
TRAINING_NAMES = ["identity", "b0.9", "b1.1", "s0.8", "s1.2"]


def factors_of(views):
    """float32 [V,3] of "training" or of a sequence of (b, c, s) triples."""
    return np.array(TRAINING if isinstance(views, str) and views == "training" else views, dtype=np.float32).reshape(-1, 3)


def blend(degenerate, image, f):
    """uint8 arrays (broadcast against each other) and a float32 factor -> uint8: one f32 multiply, one f32 add."""
    f = np.float32(f)
    d = np.asarray(degenerate).astype(np.int32)
    i = np.asarray(image).astype(np.int32)
    prod = (f * (i - d).astype(np.float32)).astype(np.float32)
    t = (d.astype(np.float32) + prod).astype(np.float32)
    out = np.where(t <= 0, np.float32(0), np.where(t >= 255, np.float32(255), t))
    return np.broadcast_to(out.astype(np.int32).astype(np.uint8), np.broadcast(d, i).shape).copy()     # float -> int truncates


def grey(img):
    """uint8 [...,3] -> the grey L = (19595 R + 38470 G + 7471 B + 32768) >> 16 as uint8 [...]."""
    a = np.asarray(img).astype(np.int64)
    return ((19595 * a[..., 0] + 38470 * a[..., 1] + 7471 * a[..., 2] + 32768) >> 16).astype(np.uint8)


def mean_grey(img):
    """m = floor((2 S + H W) / (2 H W)) of one image uint8 [H,W,3]: the rounded mean grey, an exact half rounded up."""
    g = grey(img)
    s, px = int(g.astype(np.int64).sum()), int(g.size)
    return (2 * s + px) // (2 * px)


def brightness(img, f):
    return img.copy() if np.float32(f) == np.float32(1) else blend(np.uint8(0), img, f)


def contrast(img, f):
    return img.copy() if np.float32(f) == np.float32(1) else blend(np.uint8(mean_grey(img)), img, f)


def saturation(img, f):
    return img.copy() if np.float32(f) == np.float32(1) else blend(grey(img)[..., None], img, f)


def view(img, triple):
    """One image uint8 [H,W,3] under one (b, c, s)."""
    b, c, s = (np.float32(v) for v in triple)
    return saturation(contrast(brightness(np.asarray(img, dtype=np.uint8), b), c), s)


def stack(x, views):
    """x uint8 [N,H,W,3] -> the stack [V*N,H,W,3], entry j * N + i = view j of image i (m of the contrast step per image)."""
    x = np.asarray(x, dtype=np.uint8)
    return np.ascontiguousarray(np.stack([view(img, t) for t in factors_of(views) for img in x]))


def mean(lowres_views):
    """[V,N,3,h,w] float32 -> m = (((v_0 + v_1) + v_2) + ...) / float32(V), every operation rounded to f32 on its own; V = 1
    is the view itself."""
    a = np.asarray(lowres_views, dtype=np.float32)
    s = a[0].copy()
    if a.shape[0] == 1:
        return s
    with np.errstate(all="ignore"):                  # inf - inf and overflow are part of the definition: NaN and inf
        for j in range(1, a.shape[0]):
            s = (s + a[j]).astype(np.float32)
        return (s / np.float32(a.shape[0])).astype(np.float32)


def view_figures(view_labels):
    """The views' final label maps uint8 [V,N,H,W] -> (counts int64 [V,N,3], support uint8 [N,H,W], stats int64 [N,10]) with
    D = V, through vote_oracle."""
    view_labels = np.asarray(view_labels)
    v = view_labels.shape[0]
    counts = np.stack([[np.bincount(img.reshape(-1), minlength=3)[:3] for img in view_labels[j]] for j in range(v)]).astype(np.int64)
    words = vo.tally(view_labels)
    _, support, _, _ = vo.decode(words, v)
    return counts, support, vo.stats(words, v)
