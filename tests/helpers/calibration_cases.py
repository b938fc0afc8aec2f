"""The inputs of the softmax-census tests, and their host census, computed once per (shape, seed) and shared.

Logits of an ``[n,3,h,w]`` batch: seeded normal values scaled by 4; on every 7th pixel (flat index i % 7 == 0) one class
leads the two others by 45 or more, so that its probability saturates (q = 65535, bin 255, and q = 0, bin 0, for the others);
on i % 7 == 1 the three logits are equal bit for bit; on i % 7 == 2 two of them are (the pair rotates with i) and the third is
the random value.  The grey duals are seeded integers 0..255."""
import functools

import numpy as np

from neuralbarkcalculator_amd import calibration as cal

# (n, h, w) -> seed: seeds for which census_cpu's margin exceeds MARGIN (test_calibration_host.py asserts it without a GPU)
SHAPES = {(1, 7, 13): 1, (3, 33, 65): 2, (2, 203, 317): 3, (1, 520, 1024): 4}
MARGIN = 1e-7


def make(n, h, w, seed):
    rng = np.random.default_rng(seed)
    logits = (rng.normal(size=(n, 3, h, w)) * 4).astype(np.float32)
    grey = rng.integers(0, 256, size=(n, h, w), dtype=np.uint8)
    flat = logits.reshape(n, 3, h * w)
    i = np.arange(h * w)
    sat = i % 7 == 0
    lead = (i // 7) % 3
    for c in range(3):
        flat[:, c, sat] = np.where(lead[sat] == c, 25.0, -20.0 - (i[sat] % 5)).astype(np.float32)
    tie3 = i % 7 == 1
    flat[:, 1, tie3] = flat[:, 0, tie3]
    flat[:, 2, tie3] = flat[:, 0, tie3]
    tie2 = i % 7 == 2
    pair = (i // 7) % 3                               # the class left out of the tie
    for c in range(3):
        a, b = [k for k in range(3) if k != c]
        sel = tie2 & (pair == c)
        flat[:, b, sel] = flat[:, a, sel]
    return logits, grey


@functools.lru_cache(maxsize=None)
def case(n, h, w, seed=None):
    """``(logits, grey, (rows, plane, margin) with the target, (rows, plane, margin) without)``; read-only arrays."""
    seed = SHAPES[(n, h, w)] if seed is None else seed
    logits, grey = make(n, h, w, seed)
    with_t, without = cal.census_cpu(logits, grey), cal.census_cpu(logits, None)
    for a in (logits, grey) + with_t[:2] + without[:2]:
        a.setflags(write=False)
    return logits, grey, with_t, without
