"""The cover tests/test_gpu_conv_matrix.py gives, as host arithmetic (tests/helpers/conv_matrix.py): which tile of the
convolution menu lands on which form of layer in which precision, over the cases of that test.  Needs the built library (the
menu and the plans come through its C ABI) and no GPU.  Run with -s, the printed ledger is the record of what the GPU test
runs.

Left out on purpose: the row-step tiles (18 - 20, kinds 1 / 2) need 128-pixel-wide maps, which no case here has;
test_row_resident_3x3_kernel_layer_by_layer and tests/test_gpu_rowstep_walk.py own them.  Per-image BatchNorm (the raw
convolutions) stays with test_tiles_do_not_change_the_bits."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import conv_matrix as cm  # noqa: E402

# the generic tiles each precision does NOT have (ConvTile::s[precision] == 0): nothing may be parametrised over these
NO_SUCH_TILE = {"fp32": [3, 12, 14, 15, 16, 17], "bf16": [14, 15, 16, 17], "f16x2": [2, 3, 4, 11, 12]}


@pytest.fixture(scope="module", autouse=True)
def _lib(built_lib):
    return built_lib


def coverage_problems(fits=cm.library_fits, say=None):
    """What the cases leave uncovered under the `fits` rule, as a list of sentences (empty: full cover)."""
    problems = []
    cases = cm.flat_cases()
    led = cm.ledger(cases, fits)
    for p in cm.PRECISIONS:
        for t in cm.tiles_of(p):
            if not any(k[0] == p and k[1] == t for k in led):
                problems.append("%s tile %d lands on no layer of any case" % (p, t))
    for arch, precisions, shapes in cm.CASES:
        form = cm.forms(arch)
        for p in precisions:
            mine = cm.ledger([(arch, p, s) for s in shapes], fits)
            for f in sorted(set(form.values())):
                ran = sorted(k[1] for k in mine if k[2] == f)
                # the tiles the form's layers admit at all: a form whose output channels leave one tile may run on one
                admits = {t for o in cm.conv_launches(arch, p, *shapes[0]) if form[o["name"]] == f
                          for t in cm.tiles_of(p) if cm.library_fits(p, t, o["co"], cm.planned_kind(p, o))}
                need = min(2, len(admits))
                if len(admits) < 2 and say:
                    say("%s %s: form %s admits the single tile %s" % (arch, p, f, sorted(admits)))
                if len(ran) < need:
                    problems.append("%s %s: form %s runs on tiles %s only" % (arch, p, f, ran))
    for arch, p, (n, h, w) in cases:
        planned = [o["tile"] for o in cm.conv_launches(arch, p, n, h, w)]
        lists = [cm.install_list(arch, p, n, h, w, t, fits) for t in cm.tiles_of(p)]
        if not all(took for _, took in lists):
            problems.append("%s: a tile of the precision lands on no layer" % cm.case_id((arch, p, (n, h, w))))
        if all(tiles == planned for tiles, _ in lists):
            problems.append("%s runs planned tiles only" % cm.case_id((arch, p, (n, h, w))))
    return problems


def test_the_menu_has_the_holes_the_matrix_leaves_out():
    assert sorted(cm.PRECISIONS) == sorted(NO_SUCH_TILE)
    for p in cm.PRECISIONS:
        assert cm.missing_tiles(p) == NO_SUCH_TILE[p], p
        assert not set(cm.tiles_of(p)) & set(NO_SUCH_TILE[p]), p
        assert sorted(cm.tiles_of(p) + NO_SUCH_TILE[p]) == cm.generic_tile_ids(), p
    print("generic tiles per precision:", {p: len(cm.tiles_of(p)) for p in cm.PRECISIONS})


def test_no_case_plans_a_row_step_tile():
    for arch, p, (n, h, w) in cm.flat_cases():
        for o in cm.conv_launches(arch, p, n, h, w):
            assert cm.planned_kind(p, o) == 0, (arch, p, (n, h, w), o["name"], o["tile"])
        for o in cm.conv_launches(arch, p, n, h, w, keep=False):
            assert cm.planned_kind(p, o) == 0, (arch, p, (n, h, w), o["name"], o["tile"])


def test_forms_follow_the_topology_and_the_plan():
    """The gated form is exactly the convolutions the plan launches on gated weights, the identity forms exactly those it
    gives a `res` buffer, and each network has the forms its layer table says."""
    for arch, precisions, shapes in cm.CASES:
        for o in cm.conv_launches(arch, precisions[0], *shapes[0]):
            f = cm.form_of(o["unit"])
            assert (".gated" in f) == ("gate" in o), (arch, o["name"], f)
            assert ("+id" in f) == ("res" in o), (arch, o["name"], f)
    resnet = {"stem", "1x1", "1x1s2", "1x1+id", "1x1+id.bigw", "3x3", "3x3s2", "3x3d2", "3x3d4"}
    aspp = {"3x3d12", "3x3d24", "3x3d36"}
    mbconv = {"stem.asym", "1x1", "1x1.gated", "1x1.gated+id", "3x3"}
    assert set(cm.forms("fcn_resnet50").values()) == resnet
    assert set(cm.forms("deeplabv3_resnet50").values()) == resnet | aspp
    assert set(cm.forms("fcn_efficientnet_b0").values()) == mbconv
    assert set(cm.forms("deeplabv3_efficientnet_b0").values()) == mbconv | aspp
    bigw = [n for n, f in cm.forms("fcn_resnet50").items() if f.endswith(".bigw")]
    assert bigw == ["backbone.layer4.%d.conv3" % i for i in range(3)]


def test_install_lists_of_hand_worked_cases():
    # fp32 tile 5 (128 x 256) on FCN-ResNet-50 at 2 x 104 x 136: every layer whose Cout divides by 256, nothing else
    blocks = {1: 3, 2: 4, 3: 6, 4: 3}
    want = []
    for li in (1, 2, 3, 4):
        for bi in range(blocks[li]):
            p = "backbone.layer%d.%d." % (li, bi)
            if li >= 3:                                            # planes 256 / 512
                want += [p + "conv1", p + "conv2"]
            if bi == 0:
                want.append(p + "downsample.0")
            want.append(p + "conv3")                               # 256 / 512 / 1024 / 2048
    want.append("classifier.0")                                    # 512
    tiles, took = cm.install_list("fcn_resnet50", "fp32", 2, 104, 136, 5)
    assert took == want
    planned = [o["tile"] for o in cm.conv_launches("fcn_resnet50", "fp32", 2, 104, 136)]
    names = [o["name"] for o in cm.conv_launches("fcn_resnet50", "fp32", 2, 104, 136)]
    assert tiles == [5 if n in want else t for n, t in zip(names, planned)]
    assert [t for n, t in zip(names, tiles) if n not in want] == [t for n, t in zip(names, planned) if n not in want]
    assert 5 not in [t for n, t in zip(names, planned) if n not in want]

    # fp32 tile 2 (256 x 128) on fcn_efficientnet_b0 at 1 x 128 x 128: the PADDED channel counts decide.  Expand convolutions
    # of 96 -> 128 (block 1), 240 -> 256 (4, 5), 480 -> 512 (6 - 8), 1152 (12 - 15); not 144 -> 192 (2, 3) nor 672 -> 704
    # (9 - 11).  Project convolutions to 80 -> 128 (5 - 7) and 112 -> 128 (8 - 10).  The head convolution, 1280; not
    # classifier.0 (320), nor the stem (32 -> 64).
    b = "backbone.model._blocks.%d.%s"
    want = ([b % (1, "_expand_conv"), b % (4, "_expand_conv")]
            + [b % (i, c) for i in (5, 6, 7) for c in ("_expand_conv", "_project_conv")]
            + [b % (8, "_expand_conv"), b % (8, "_project_conv"), b % (9, "_project_conv"), b % (10, "_project_conv")]
            + [b % (i, "_expand_conv") for i in (12, 13, 14, 15)] + ["backbone.model._conv_head"])
    assert cm.install_list("fcn_efficientnet_b0", "fp32", 1, 128, 128, 2)[1] == want

    # bf16 tile 3 (256 x 256) on DeepLabV3-ResNet-50 at 2 x 104 x 136: the trunk as in the first case, and in the head the four
    # ASPP convolutions, the projection and classifier.1 (all 256); the pooling branch is no convolution launch
    took = cm.install_list("deeplabv3_resnet50", "bf16", 2, 104, 136, 3)[1]
    trunk = cm.install_list("fcn_resnet50", "fp32", 2, 104, 136, 5)[1][:-1]
    assert took == trunk + ["classifier.0.convs.%d.0" % i for i in range(4)] + ["classifier.0.project.0", "classifier.1"]

    # a tile the precision does not have fits nothing: the list is the plan's
    tiles, took = cm.install_list("fcn_resnet50", "f16x2", 2, 104, 136, 2)
    assert took == [] and tiles == [o["tile"] for o in cm.conv_launches("fcn_resnet50", "f16x2", 2, 104, 136)]


def test_the_cases_cover_the_matrix(capsys):
    notes = []
    problems = coverage_problems(say=notes.append)
    led = cm.ledger(cm.flat_cases())
    with capsys.disabled():
        print()
        for note in notes:
            print(note)
        print("precision tile form -> layers over the %d cases" % len(cm.flat_cases()))
        for (p, t, f), n in sorted(led.items(), key=lambda kv: (cm.PRECISIONS.index(kv[0][0]), kv[0][1], kv[0][2])):
            print("%-6s %2d  %-14s %4d" % (p, t, f, n))
    assert not problems, "\n".join(problems)
    # the counts the GPU test's last check reproduces: every generic (precision, tile) of the menu
    assert {p: len({k[1] for k in led if k[0] == p}) for p in cm.PRECISIONS} == {p: len(cm.tiles_of(p)) for p in cm.PRECISIONS}


def test_the_coverage_check_fails_when_no_tile_ever_fits():
    """The check's own logic: under a stand-in rule that never accepts a tile (what conv_tile_ok regressing to "never" would
    look like to a lenient test), every line of the cover is reported missing."""
    def never(precision, tile, cout_pad, kind):
        return False

    assert cm.ledger(cm.flat_cases(), never) == {}
    problems = coverage_problems(never)
    assert len([s for s in problems if "lands on no layer of any case" in s]) == sum(len(cm.tiles_of(p)) for p in cm.PRECISIONS)
    assert len([s for s in problems if "runs planned tiles only" in s]) == len(cm.flat_cases())
    assert any("runs on tiles [] only" in s for s in problems)
    with pytest.raises(AssertionError):
        assert not problems, "\n".join(problems)


def test_the_bit_comparison_sees_what_a_float_comparison_does_not():
    a = np.arange(2 * 3 * 4 * 5, dtype=np.float32).reshape(2, 3, 4, 5)
    a[0, 0, 0, 0] = np.nan
    assert cm.first_difference(a, a.copy()) is None
    b = a.copy()
    b[1, 2, 0, 3] = np.nextafter(b[1, 2, 0, 3], np.float32(np.inf))
    b[1, 2, 3, 4] += np.float32(1)
    assert cm.first_difference(b, a) == ((1, 2, 0, 3), 2)
    z = np.zeros((1, 1, 2, 2), np.float32)
    assert cm.first_difference(-z, z) == ((0, 0, 0, 0), z.size)            # signed zeros
    n = z.copy()
    n.view(np.uint32)[...] = np.float32(np.nan).view(np.uint32)
    q = n.copy()
    q.view(np.uint32)[0, 0, 1, 1] ^= 1                                     # another NaN payload
    assert cm.first_difference(q, n) == ((0, 0, 1, 1), 1)
    assert cm.first_difference(z, z[:, :, :1]) is not None                 # a shape mismatch is a difference
