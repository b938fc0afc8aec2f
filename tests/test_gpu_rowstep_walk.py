"""The tile walk of the row-step 3x3 kernel (csrc/conv3x3_rows.hip, tiles 18 and 20, "f16x2"): a launch has one block per
compute unit at the most, block b computes tiles b, b + blocks, ..., and its loader waves request the next tile's table and
first row-step while the MFMA waves are in the epilogue.  Which block computes which tile must change no bit.

References, none of them recorded from the code under test:
  * tile 18 against tile 20 of the same forward (the same K order per output, two tile shapes with two different walks:
    rows x 4 or 2 channel tiles of 128 against row pairs x 8 or 4 channel tiles of 64);
  * a batch against its images run one by one, where each single image gives every block ONE tile (33 map rows: 136 tiles
    of a 512-channel layer) and the batch gives a block two or three;
  * the CPU oracle under the layer tolerance of tests/test_gpu_parity.py.
The units: layer4.{0,1,2}.conv2 (512 -> 512 channels, dilation 2, 4, 4) and classifier.0 (2048 -> 512, dilation 1) on
128-pixel-wide maps of a 1024-pixel-wide image (eight channel tiles of 64 on tile 20), and layer3's conv2 (256 channels,
dilation 1 and 2) beside them.  Tile counts follow from the device's compute units, so a case means the same on another chip
and is skipped where its premise (more tiles than compute units) does not hold.
"""
import numpy as np
import pytest
import torch

from neuralbarkcalculator_amd.model import FCNResNet50
from test_gpu_parity import DEV, LAYER_RTOL_FP32, frames

pytestmark = pytest.mark.gpu

UNITS_512 = {"backbone.layer4.0.conv2": 2, "backbone.layer4.1.conv2": 4, "backbone.layer4.2.conv2": 4, "classifier.0": 1}   # name: dilation
UNITS_256 = {"backbone.layer3.0.conv2": 1, "backbone.layer3.1.conv2": 2, "backbone.layer3.5.conv2": 2}


def pairs_of(rows, dil):
    """Row pairs (oy, oy + dil) of a map of `rows` rows: rowstep_pairs of the kernel's file."""
    groups = rows // (2 * dil)
    rem = rows - groups * 2 * dil
    return groups * dil + min(rem, dil)


def tiles20(n, rows, dil, co=512):
    return n * pairs_of(rows, dil) * (co // 64)


def tile_at(tl, nblk, tiles_n):
    """Tile tl of a launch -> (channel tile, row or pair index over the batch): the kernel's XCD-aware index map."""
    q, rr, xcd = nblk >> 3, nblk & 7, tl & 7
    bid = (xcd * (q + 1) if xcd < rr else rr * (q + 1) + (xcd - rr) * q) + (tl >> 3)
    return bid % tiles_n, bid // tiles_n


def cus():
    return torch.cuda.get_device_properties(DEV).multi_processor_count


@pytest.fixture(scope="module")
def model(built_lib, sd_np):
    m = FCNResNet50("f16x2").load_state_dict(sd_np).to(DEV)
    m.set_keep_activations(True)
    yield m
    m.set_keep_activations(False)


def run_units(m, x, tile):
    """The units' outputs (f32 NCHW) of one forward of x with the row-step layers on `tile`."""
    n, rows = x.shape[0], x.shape[2] // 8
    m.set_conv_tile(tile)
    m.lowres_logits(x.to(DEV))
    torch.cuda.synchronize()
    out = {}
    for name in list(UNITS_512) + list(UNITS_256):
        co = 512 if name in UNITS_512 else 256
        out[name] = m.read_activation(name, n * co * rows * 128).copy()
        assert out[name].shape == (n, co, rows, 128), (name, out[name].shape)
    m.set_conv_tile(-1)
    return out


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


@pytest.mark.parametrize("n,rows,min_per_block,max_per_block", [(1, 1, 1, 1), (1, 33, 1, 1), (1, 65, 1, 2), (1, 129, 2, 3), (2, 65, 2, 3)])
def test_tile_20_and_tile_18_agree_bit_for_bit_however_many_tiles_a_block_walks(model, n, rows, min_per_block, max_per_block):
    """Map rows 1, 33, 65 and 129 (and a batch of two at 65, where a block's walk crosses from one image into the next): 8, 136,
    264, 520 and 528 tiles of a 512-channel layer on tile 20 -- on 256 compute units one tile per block, one, one or two (the
    first eight blocks take a second), two or three, and two or three."""
    count = tiles20(n, rows, 1)
    assert all(tiles20(n, rows, d) == count for d in (2, 4)), "odd map rows: the same pair count at every dilation"
    blocks = min(count, cus())
    lo, hi = count // blocks, -(-count // blocks)
    print("map rows", rows, "batch", n, "tiles", count, "blocks", blocks, "tiles per block", lo, "to", hi)
    if max_per_block > 1 and count <= cus():
        pytest.skip("%d tiles on %d compute units: no block walks" % (count, cus()))
    if cus() == 256:
        assert (lo, hi) == (min_per_block, max_per_block)
    x = frames(range(40, 40 + n), 8 * rows, 1024)
    t20, t18 = run_units(model, x, 20), run_units(model, x, 18)
    for name in t20:
        assert np.isfinite(t20[name]).all() and float(np.abs(t20[name]).max()) > 0, name
        assert same_bits(t20[name], t18[name]), "%s: tile 20 and tile 18 differ (%d rows, batch %d)" % (name, rows, n)


@pytest.mark.parametrize("n", [2, 4])
@pytest.mark.parametrize("tile", [20, 18])
def test_a_walking_batch_equals_its_images_run_with_one_tile_per_block(model, n, tile):
    """33 map rows: one image is 136 tiles (tile 20) or 132 (tile 18) of a 512-channel layer, a tile per block; a batch of two or
    four is 272 / 264 or 544 / 528, which 256 blocks walk.  The batch must hold the single images' bits."""
    rows = 33
    single, batch = tiles20(1, rows, 1), tiles20(n, rows, 1)
    if not single <= cus() < batch:
        pytest.skip("%d and %d tiles on %d compute units: not one tile per block against a walk" % (single, batch, cus()))
    x = frames(range(50, 50 + n), 8 * rows, 1024)
    whole = run_units(model, x, tile)
    for i in range(n):
        one = run_units(model, x[i:i + 1], tile)
        for name in one:
            assert same_bits(whole[name][i:i + 1], one[name]), "%s: image %d of a batch of %d (tile %d)" % (name, i, n, tile)


def test_walk_against_the_oracle_with_an_odd_last_pair_as_a_second_tile(oracle_model, model):
    """65 map rows: the last pair of classifier.0 (dilation 1) is row 64 and a row below the image, which is computed on
    zero rows and not stored; on 256 compute units that pair's eighth channel tile is tile 263, the SECOND tile of block 7,
    whose loaders ran ahead into it.  Every unit against the oracle under the layer tolerance, the last map row on its own as
    well."""
    from oracle.fcn_resnet50_oracle import layer_outputs
    rows = 65
    count, n_cus = tiles20(1, rows, 1), cus()
    if count <= n_cus:
        pytest.skip("%d tiles on %d compute units: no block walks" % (count, n_cus))
    last = pairs_of(rows, 1) - 1
    assert 2 * last + 1 >= rows, "the last pair's second row lies below the image"
    later = [tl for tl in range(n_cus, count) if tile_at(tl, count, 8)[1] == last]
    print("tiles of the odd last pair that are not a block's first:", later)
    if not later:
        pytest.skip("no tile of the odd last pair is a block's second on %d compute units" % n_cus)
    x = frames([60], 8 * rows, 1024)
    ref = layer_outputs(oracle_model, x)
    for tile in (20, 18):
        got = run_units(model, x, tile)
        for name, have in got.items():
            want = ref[name].numpy()
            scale = float(np.abs(want).max())
            err = float(np.abs(have - want).max()) / scale
            err_last = float(np.abs(have[:, :, -1] - want[:, :, -1]).max()) / scale
            print("tile", tile, name, "rel err", err, "last row", err_last)
            assert err <= LAYER_RTOL_FP32, "%s: rel err %g (tile %d)" % (name, err, tile)
            assert float(np.abs(have[:, :, -1]).max()) > 0, name
