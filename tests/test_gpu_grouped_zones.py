"""remove_small_zones on [B,H,W] batches on the GPU (nbc_remove_small_zones_groups, csrc/small_zones.hip) against the host
restatement postprocess.remove_small_zones_grouped (scipy's 18-neighbourhood, the call skimage makes for a 3-D array with
connectivity=2).  Integer work: every comparison is exact."""
import os
import sys

import numpy as np
import pytest
import torch

from neuralbarkcalculator_amd import _lib
from neuralbarkcalculator_amd.model import FCNResNet50
from neuralbarkcalculator_amd.postprocess import remove_small_zones, remove_small_zones_grouped

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import grouped_cases as gc  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
GUARD = 64


@pytest.fixture(scope="module")
def model(built_lib, sd_np):
    return FCNResNet50("bf16").load_state_dict(sd_np).to(DEV)


def run_groups(model, labels_np, group, min_pixels=150, dtype=torch.uint8, stream=None):
    """One nbc_remove_small_zones_groups call on labels placed between guard bytes: (labels, counts) numpy."""
    n, h, w = labels_np.shape
    item = 8 if dtype == torch.int64 else 1
    buf = torch.full((GUARD + n * h * w * item + GUARD,), 0xA5, dtype=torch.uint8, device=DEV)
    body = buf[GUARD: GUARD + n * h * w * item]
    body.copy_(torch.from_numpy(np.ascontiguousarray(labels_np)).to(dtype).to(DEV).view(torch.uint8).reshape(-1))
    counts = torch.full((n * 3 + 8,), -77, dtype=torch.int64, device=DEV)
    s = stream if stream is not None else torch.cuda.current_stream(DEV)
    if stream is not None:
        stream.wait_stream(torch.cuda.current_stream(DEV))
    _lib.check(model._lib.nbc_remove_small_zones_groups(model._ctx, buf.data_ptr() + GUARD, _lib.LABEL_I64 if dtype == torch.int64 else _lib.LABEL_U8,
                                                        n, h, w, group, min_pixels, counts.data_ptr() + 8 * 4, s.cuda_stream),
               "nbc_remove_small_zones_groups")
    s.synchronize()
    raw, c = buf.cpu().numpy(), counts.cpu().numpy()
    assert (raw[:GUARD] == 0xA5).all() and (raw[-GUARD:] == 0xA5).all()
    assert (c[:4] == -77).all() and (c[-4:] == -77).all()
    out = raw[GUARD:-GUARD].view(np.int64 if dtype == torch.int64 else np.uint8).reshape(n, h, w)
    return out.astype(np.uint8), c[4:-4].reshape(n, 3)


def bincounts(labels):
    return [[int((l == c).sum()) for c in range(3)] for l in labels]


@pytest.mark.parametrize("dtype", [torch.uint8, torch.int64])
def test_offset_table(model, dtype):
    for dy, dx in gc.OFFSETS:
        labels, want = gc.offset_case(dy, dx)
        got, counts = run_groups(model, labels, 2, 2, dtype)
        np.testing.assert_array_equal(got, want, err_msg=str((dy, dx)))
        assert counts.tolist() == bincounts(want)
        assert not run_groups(model, labels, 1, 2, dtype)[0].any()                 # apart, each pixel is alone


@pytest.mark.parametrize("dtype", [torch.uint8, torch.int64])
def test_blob_table(model, dtype):
    for planes, group, survive in gc.BLOB_TABLE:
        got, counts = run_groups(model, gc.blob_planes(planes), group, 150, dtype)
        np.testing.assert_array_equal(got, gc.blob_planes(survive), err_msg=str((planes, group)))
        assert counts.tolist() == bincounts(gc.blob_planes(survive))


@pytest.fixture(scope="module")
def random_cases():
    """(labels, {(G, min_pixels): the host restatement}) per shape and class-0 share, computed once."""
    out = []
    for n, h, w in gc.RANDOM_SHAPES:
        for share in gc.RANDOM_SHARES:
            labels = gc.random_labels(n, h, w, share)
            out.append((labels, {(g, mp): remove_small_zones_grouped(labels, g, mp) for g in gc.RANDOM_GROUPS for mp in (2, 150)}))
    return out


@pytest.mark.parametrize("min_pixels", [2, 150])
@pytest.mark.parametrize("group", gc.RANDOM_GROUPS)
def test_random_labels_equal_the_host_restatement(model, random_cases, group, min_pixels):
    differs = 0
    for labels, wants in random_cases:
        want = wants[(group, min_pixels)]
        for dtype in (torch.uint8, torch.int64):
            got, counts = run_groups(model, labels, group, min_pixels, dtype)
            assert got.tobytes() == want.tobytes(), (labels.shape, group, min_pixels, int((got != want).sum()))
            assert counts.tolist() == bincounts(want)
        differs += int((want != wants[(1, min_pixels)]).sum())
    assert (differs > 0) == (group > 1)                                            # the batch axis matters


def test_group_of_one_is_the_per_image_call(model, random_cases):
    for labels, wants in random_cases:
        for mp in (2, 150):
            t = torch.from_numpy(labels).to(DEV)
            per_image, per_counts = model.remove_small_zones(t.clone(), min_pixels=mp)
            got, counts = run_groups(model, labels, 1, mp)
            assert got.tobytes() == per_image.cpu().numpy().tobytes() and counts.tolist() == per_counts.cpu().tolist()
            assert got.tobytes() == remove_small_zones(labels, mp).tobytes()


def test_a_groups_bytes_do_not_depend_on_the_call_or_the_stream(model, random_cases):
    labels, wants = random_cases[1]                                                # 7 x 33 x 65, share 0.45
    group = 3
    whole, _ = run_groups(model, labels, group)
    side = torch.cuda.Stream(DEV)
    for a in range(0, len(labels), group):
        alone, _ = run_groups(model, labels[a:a + group], group)
        assert alone.tobytes() == whole[a:a + group].tobytes()
        other, _ = run_groups(model, labels[a:a + group], group, stream=side)
        assert other.tobytes() == alone.tobytes()
    assert whole.tobytes() == wants[(group, 150)].tobytes()


def test_model_method_validates(model):
    labels = torch.from_numpy(gc.random_labels(4, 33, 65, 0.45)).to(DEV)
    out, counts = model.remove_small_zones_groups(labels.clone(), 2)
    assert out.shape == labels.shape and counts.dtype == torch.int64 and tuple(counts.shape) == (4, 3)
    assert out.cpu().numpy().tobytes() == remove_small_zones_grouped(labels.cpu().numpy(), 2).tobytes()
    # the context's workspace grows and is reused: small, larger, small again on one object, as on fresh ones
    m = model.clone_shared()
    for sl in (slice(0, 2), slice(0, 4), slice(1, 3)):
        got, got_counts = m.remove_small_zones_groups(labels[sl].clone(), 2, min_pixels=6)
        want, want_counts = model.clone_shared().remove_small_zones_groups(labels[sl].clone(), 2, min_pixels=6)
        assert torch.equal(got, want) and torch.equal(got_counts, want_counts) and not torch.equal(got, labels[sl])
    for bad in (labels[0], labels.float(), labels.cpu(), labels[:, :, ::2], labels[:0]):
        with pytest.raises(ValueError):
            model.remove_small_zones_groups(bad, 2)
    for group in (0, 65, -1, 2.0, True, None):
        with pytest.raises(ValueError):
            model.remove_small_zones_groups(labels.clone(), group)
    with pytest.raises(ValueError):
        model.remove_small_zones_groups(labels.clone(), 2, min_pixels=-1)
