"""The one labelling rule of csrc/components.hpp at every place it applies, exhaustively: every assignment of a window of
2 rows x 4 columns (the whole support of the row rule -- W / E / N / NW / NE -- and of the column rule -- the 2x2 block
across the border plus the straight neighbours), everything else background, at four placements relative to the 32-pixel
tile grid.  Packing: a cell of 64x64 pixels (2x2 tiles) holds one window of each placement, all four with the cell's
assignment; they lie 16 or more pixels apart and never touch.  The cells tile maps of grid x grid cells.
label_zones (three values per pixel, 3^8 assignments) against zones.zones_cpu, remove_small_zones (two values, both
polarities, 2^8 assignments) against postprocess.remove_small_zones.  Integer work: every comparison is exact."""
import numpy as np
import pytest
import torch

from neuralbarkcalculator_amd import zones
from neuralbarkcalculator_amd.model import FCNResNet50
from neuralbarkcalculator_amd.postprocess import remove_small_zones

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CELL = 64
PLACEMENTS = {"inside a tile": (10, 10), "across a horizontal border": (31, 10), "across a vertical border": (10, 30),
              "across a tile corner": (31, 30)}                    # the window's first row and column within the cell


@pytest.fixture(scope="module")
def model(built_lib, sd_np):
    return FCNResNet50("bf16").load_state_dict(sd_np).to(DEV)


def packed_windows(values, grid):
    """uint8 maps [images, grid * 64, grid * 64]: cell k (row-major over images, cell rows, cell columns) carries assignment
    k -- pixel j of the window, row-major, is values[digit j of k in base len(values)] -- at each of the four placements;
    values[0] is the background.  len(values) ** 8 must fill whole images."""
    base = len(values)
    n = base ** 8
    images, rest = divmod(n, grid * grid)
    assert rest == 0
    digits = (np.arange(n)[:, None] // base ** np.arange(8)) % base
    windows = np.asarray(values, np.uint8)[digits].reshape(n, 2, 4)
    cells = np.full((n, CELL, CELL), values[0], np.uint8)
    for y, x in PLACEMENTS.values():
        cells[:, y:y + 2, x:x + 4] = windows
    return cells.reshape(images, grid, grid, CELL, CELL).transpose(0, 1, 3, 2, 4).reshape(images, grid * CELL, grid * CELL)


def count_pairs(maps, values):
    """The number of distinct (placement, assignment) pairs read back from the maps; asserts that nothing else is set."""
    images, side, _ = maps.shape
    grid = side // CELL
    cells = maps.reshape(images, grid, CELL, grid, CELL).transpose(0, 1, 3, 2, 4).reshape(-1, CELL, CELL).copy()
    digit = np.full(256, -1, np.int64)
    digit[np.asarray(values)] = np.arange(len(values))
    pairs = 0
    for y, x in PLACEMENTS.values():
        d = digit[cells[:, y:y + 2, x:x + 4].reshape(-1, 8)]
        assert (d >= 0).all()
        pairs += np.unique((d * len(values) ** np.arange(8)).sum(axis=1)).size
        cells[:, y:y + 2, x:x + 4] = values[0]
    assert (cells == values[0]).all()
    return pairs


def test_packing_holds_every_pair():
    """The packing itself: cell k carries assignment k at all four placements, and count_pairs reads them back."""
    maps = packed_windows((0, 2), 16)
    assert maps.shape == (1, 1024, 1024) and count_pairs(maps, (0, 2)) == 4 * 256
    assert maps[0, 10:12, 10:14].sum() == 0 and maps[0, 10:12, 64 + 10:64 + 14].tolist() == [[2, 0, 0, 0], [0, 0, 0, 0]]


def test_label_zones_on_every_window(model):
    maps = packed_windows((0, 1, 2), 27)                           # 9 maps of 1728 x 1728
    assert count_pairs(maps, (0, 1, 2)) == 4 * 3 ** 8
    want = zones.zones_cpu(maps)
    cap = max(len(z) for z in want)
    t = torch.from_numpy(maps).to(DEV)
    rows, num = model.label_zones(t, cap=cap)
    torch.cuda.synchronize()
    rows, num = rows.cpu().numpy(), num.cpu().numpy()
    for i, z in enumerate(want):
        assert int(num[i]) == len(z), f"map {i}: {int(num[i])} zones, zones_cpu has {len(z)}"
        if not np.array_equal(rows[i, :len(z)], z):
            bad = int(np.flatnonzero((rows[i, :len(z)] != z).any(axis=1))[0])
            y, x = divmod(int(z[bad, 0]), maps.shape[2])
            raise AssertionError(f"map {i}: row {bad} differs (the zone that starts at y {y} x {x}, cell-local {y % CELL} {x % CELL}): "
                                 f"got {rows[i, bad].tolist()}, want {z[bad].tolist()}")
    assert sum(len(z) for z in want) > 4 * 3 ** 8                  # more than one zone per window on average


@pytest.mark.parametrize("min_pixels", [2, 3, 5])
def test_remove_small_zones_on_every_window(model, min_pixels):
    """Both polarities: windows of 2 in a map of 0 (phase 0 decides: which non-zero components are small) and windows of 0
    in a map of 1 (phase 1 decides: which background components are small)."""
    set_in_zero, zero_in_set = packed_windows((0, 2), 16), packed_windows((1, 0), 16)
    assert count_pairs(set_in_zero, (0, 2)) == 4 * 256 and count_pairs(zero_in_set, (1, 0)) == 4 * 256
    maps = np.concatenate([set_in_zero, zero_in_set])
    want = remove_small_zones(maps, min_pixels)
    t = torch.from_numpy(maps).to(DEV)
    got, counts = model.remove_small_zones(t, min_pixels=min_pixels)
    torch.cuda.synchronize()
    got = got.cpu().numpy()
    if not np.array_equal(got, want):
        i, y, x = (int(v[0]) for v in np.nonzero(got != want))
        raise AssertionError(f"map {i}: {int((got != want).sum())} pixels differ, first at y {y} x {x} (cell-local {y % CELL} {x % CELL})")
    assert counts.cpu().tolist() == [[int((w == c).sum()) for c in range(3)] for w in want]
    for i in range(2):                                             # the threshold decides: some windows flip, some stay
        changed = int((want[i] != maps[i]).sum())
        assert 0 < changed < int((maps[i] != maps[i, 0, 0]).sum())
