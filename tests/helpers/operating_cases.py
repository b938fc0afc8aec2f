"""Shared inputs of the nbc_offset_sweep tests: per shape, logits and a grey mask built once, and per (shape, grid) the host
table of operating.sweep_cpu, computed once and shared.

The logits are half random normal x 4 and half multiples of 0.5 in [-8, 8] -- on the default grid those give exact ties
x2 + b2 == x0 and x1 + b1 == x0 at many points, where the first maximum must win --, with NaN and +-inf pixels mixed in at
fixed places (every class, alone and together)."""
import functools

import numpy as np

from neuralbarkcalculator_amd import operating as op

# the smallest shapes at which tiling, tails and alignment can go wrong: one pixel; exactly one tile of 4096; one pixel past
# a tile on a single row; 8777 pixels, odd, so that the planes' byte offsets run through all four residues mod 16 over the
# three images; a second odd batch
SHAPES = [(1, 1, 1), (1, 64, 64), (1, 1, 4097), (3, 67, 131), (2, 33, 65)]
GRIDS = {
    "default": (op.parse_grid(op.DEFAULT_GRID), op.parse_grid(op.DEFAULT_GRID)),
    "zero": (np.zeros(1, np.float32), np.zeros(1, np.float32)),
    "1x33": (np.zeros(1, np.float32), op.parse_grid(op.DEFAULT_GRID)),
    "33x1": (op.parse_grid(op.DEFAULT_GRID), np.zeros(1, np.float32)),
    "uneven": (np.array([-3.25, -1.0, 0.0, 0.125, 6.5], np.float32), np.array([-5.5, 0.0, 2.75], np.float32)),
}
SPECIALS = [(np.nan, 0.0, 0.0), (0.0, np.nan, 0.0), (0.0, 0.0, np.nan), (np.nan, np.nan, 1.0), (np.nan, np.nan, np.nan),
            (np.inf, 0.0, 0.0), (0.0, np.inf, -1.0), (0.0, 1.0, np.inf), (-np.inf, -np.inf, -np.inf), (0.0, 0.0, -np.inf),
            (np.inf, np.inf, np.inf), (1.0, np.nan, np.inf), (-np.inf, 0.5, np.nan)]


@functools.lru_cache(maxsize=None)
def inputs(n, h, w):
    """(logits f32 [n,3,h,w], grey u8 [n,h,w]), read-only."""
    rng = np.random.default_rng(1000 * n + 10 * h + w)
    p = h * w
    logits = (rng.standard_normal((n, 3, p)) * 4).astype(np.float32)
    ties = rng.random((n, p)) < 0.5
    half = (rng.integers(-16, 17, size=(n, 3, p)) * 0.5).astype(np.float32)
    logits = np.where(ties[:, None, :], half, logits)
    if p >= 64:                                      # the specials at fixed places of every image, the last pixel among them
        for i in range(n):
            for k, vals in enumerate(SPECIALS):
                q = (k * 37 + i * 11) % (p - 1) if k else p - 1
                logits[i, :, q] = vals
    grey = np.array([0, 63, 64, 128, 191, 192, 255], np.uint8)[rng.integers(0, 7, size=(n, p))]
    logits, grey = logits.reshape(n, 3, h, w), grey.reshape(n, h, w)
    logits.setflags(write=False)
    grey.setflags(write=False)
    return logits, grey


@functools.lru_cache(maxsize=None)
def table(n, h, w, grid):
    """operating.sweep_cpu of inputs(n, h, w) on GRIDS[grid]: int64 [n,G1,G2,3,3], read-only."""
    logits, grey = inputs(n, h, w)
    t = op.sweep_cpu(logits, grey, *GRIDS[grid])
    t.setflags(write=False)
    return t
