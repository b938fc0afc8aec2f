"""The exact gather probe: a checkpoint under which every conv unit's stored output is known to the bit from the operands it
read, in every precision and under any order of summation.  Host only (numpy).

Every conv row o is one-hot: a single weight +-1 at one K position (kh, kw, ci), zeros elsewhere.  f16x2 packs it as
P = +-2^14, Q = 0; the accumulator is +-2^14 x 2^a of one stored input value -- exact, since the join of its pieces is exact in
f32 and every other product is 0; fp32 and bf16 multiply by +-1.  Every BatchNorm has running_mean 0 and
running_var = f32(1) - f32(1e-5), for which f32(var + eps) = 1 and 1 / sqrt(.) = 1 exactly (asserted below), a weight that is a
power of two and a bias that is a dyadic value of 20 significant bits, mostly positive -- so a tap that reads padding still
stores a non-zero value with a non-zero low piece, and the ReLU takes both branches.  The stored output is then
f32(+-x 2^g + beta) (the epilogue's fma: the product is exact, one rounding), one f32 add of the identity, the ReLU, and the
store's rounding: split16 (f16x2), round to nearest even to bf16, or nothing (fp32).  `expected_unit` restates these steps in
numpy f32; the comparison is uint32 equality.  bn3 and downsample.1 have weight 2^-2 so that the residual streams stay bounded
over 16 blocks.

In round r row o of a unit with K = Cin k k selects K position (o + r Cout) mod K in the packer's (kh, kw, ci) order; ROUNDS = 9
rounds hit every K position of every unit with K <= 9 Cout (all but the K = 18 432 units: classifier.0 and the ASPP 3x3
branches).  For those, with q = o + r Cout and S = K / 32 K-steps, the row selects K-step q mod S and channel slot
(q + q // S) mod 32 in it: every K-step (a tap x a 32-channel block), every slot, every residue of the K-step index mod 8 (the
flush cadence).  tests/test_gather_probe_cover.py computes the cover.

Known limit: Q = 0 here, so the weights' low piece (the product Q X0) is not probed; the bound of f32_grade_bound.py holds it,
and rejects a Q X0 product lost in a single K-step only for K up to about 150 (the fault table of
tests/test_f32_grade_bound.py): beyond that such a loss is seen by neither.  An exact probe with Q != 0 needs X1 = 0 in every tensor, which the store does not preserve.
The ASPP pooling branch keeps f32 weights and a mean over the map: not exact, covered by the bound only."""
import numpy as np

import f32_grade_bound as fb
import operand_bound as ob
from neuralbarkcalculator_amd import synth, topology

ROUNDS = 9
SLOTS = 32
PROBE_VAR = np.float32(1) - np.float32(1e-5)
assert np.float32(PROBE_VAR + ob.BN_EPS) == np.float32(1) and np.float32(1) / np.sqrt(np.float32(PROBE_VAR + ob.BN_EPS)) == np.float32(1)
STREAM_LOG2_GAIN = -2                   # bn3 and downsample.1
NEGATIVE_SHARE = 0.25                   # of the rows' signs; of the biases 1 / 8


def is_long(u):
    return u.cin * u.k * u.k > ROUNDS * u.cout


def positions(u, r):
    """K position (packer order: (kh k + kw) Cin + ci) that each of the unit's Cout rows selects in round r"""
    K = u.cin * u.k * u.k
    q = np.arange(u.cout, dtype=np.int64) + r * u.cout
    if not is_long(u):
        return q % K
    assert K % SLOTS == 0
    steps = K // SLOTS
    return (q % steps) * SLOTS + (q + q // steps) % SLOTS


def _uniform(seed, arch, ui, r, what, n):
    return synth.uniform01(seed, 100000 * topology.arch_index(arch) + 1000 * ui + 10 * r + what, n)


def signs(arch, ui, u, r, seed=0):
    return np.where(_uniform(seed, arch, ui, r, 0, u.cout) < NEGATIVE_SHARE, -1.0, 1.0).astype(np.float32)


def log2_gain(u):
    return STREAM_LOG2_GAIN if u.bn.endswith((".bn3", ".downsample.1")) else 0


def biases(arch, ui, u, r, seed=0):
    """m 2^-20 with 2^19 <= m < 2^20 odd: in [0.5, 1), 20 significant bits; one in eight negative"""
    m = (2 ** 19 + np.floor(_uniform(seed, arch, ui, r, 1, u.cout) * 2 ** 18).astype(np.int64) * 2 + 1).astype(np.float64)
    neg = _uniform(seed, arch, ui, r, 2, u.cout) < 0.125
    return (np.where(neg, -m, m) * 2.0 ** -20).astype(np.float32)


def probe_state_dict(arch, r, seed=0):
    """(state_dict, {unit name: (positions, signs)}) of round r; classifier.4 keeps small dense f32 weights (not probed)."""
    units = {u.name: (i, u) for i, u in enumerate(topology.conv_units(arch))}
    sd, sel = {}, {}
    for key, shape, dtype in topology.state_dict_spec(arch):
        sd[key] = np.zeros(shape, dtype=np.int64 if dtype == "int64" else np.float32)
    for name, (ui, u) in units.items():
        if u.bn is None:
            sd[name + ".weight"][:] = (synth.normal(seed, 7, u.cout * u.cin).reshape(u.cout, u.cin, 1, 1) * 2.0 ** -6).astype(np.float32)
            continue
        pos, sg = positions(u, r), signs(arch, ui, u, r, seed)
        tap, ci = pos // u.cin, pos % u.cin
        sd[name + ".weight"][np.arange(u.cout), ci, tap // u.k, tap % u.k] = sg
        sd[u.bn + ".weight"][:] = np.float32(2.0 ** log2_gain(u))
        sd[u.bn + ".bias"][:] = biases(arch, ui, u, r, seed)
        sd[u.bn + ".running_var"][:] = PROBE_VAR
        sel[name] = (pos, sg)
    return sd, sel


def gather(x, u, pos):
    """(values [N, Cout, Ho, Wo] each row's K position selects from x [N, Cin, H, W] (0 from padding), the same shape of flags:
    the tap lies outside the image)"""
    n, _, h, w = x.shape
    ho = (h + 2 * u.pad - u.dil * (u.k - 1) - 1) // u.stride + 1
    wo = (w + 2 * u.pad - u.dil * (u.k - 1) - 1) // u.stride + 1
    xp = np.pad(x, ((0, 0), (0, 0), (u.pad, u.pad), (u.pad, u.pad)))
    out = np.empty((n, u.cout, ho, wo), x.dtype)
    outside = np.empty((u.cout, ho, wo), bool)
    tap, ci = pos // u.cin, pos % u.cin
    for t in np.unique(tap):
        rows = np.nonzero(tap == t)[0]
        y0, x0 = (t // u.k) * u.dil, (t % u.k) * u.dil
        ys, xs = y0 + u.stride * np.arange(ho), x0 + u.stride * np.arange(wo)
        out[:, rows] = xp[:, ci[rows]][:, :, ys][:, :, :, xs]
        oy, ox = (ys < u.pad) | (ys >= u.pad + h), (xs < u.pad) | (xs >= u.pad + w)
        outside[rows] = (oy[:, None] | ox[None, :])[None]
    return out, outside


def store(v, precision):
    if precision == "f16x2":
        return fb.join16(*fb.split16(v))
    if precision == "bf16":
        return ob.bf16_round(v)
    assert precision == "fp32", precision
    return v


def expected_unit(x, u, pos, sg, beta, res, precision):
    """What the unit stores, to the bit: numpy f32 operation by operation"""
    g, _ = gather(np.ascontiguousarray(x, dtype=np.float32), u, pos)
    v = g * (sg * np.float32(2.0 ** log2_gain(u))).reshape(1, -1, 1, 1) + np.asarray(beta, np.float32).reshape(1, -1, 1, 1)
    if res is not None:
        v = v + np.asarray(res, dtype=np.float32)
    if u.relu:
        v = np.maximum(v, np.float32(0))
    assert v.dtype == np.float32
    return store(v, precision)


def ingested(x, precision):
    """The stem's operand: the frame as the ingest kernel stores it (its definition of the stored pixel)"""
    return store(np.ascontiguousarray(x, dtype=np.float32), precision)


def simulate(arch, sd, sel, reads, x, precision):
    """{op: the tensor it would store} of the whole probe network on the CPU, every unit by `expected_unit` on its producers'
    simulated tensors (the max-pool 3 x 3 / 2; the DeepLabV3 pooling branch and concat in plain f32: not probed)"""
    acts = {"ingest": ingested(x, precision)}
    for u in topology.conv_units(arch):
        if u.bn is None:
            continue
        if u.pooled:
            src = acts[reads[("classifier.0.convs.4", "in")]]
            z = src.mean(axis=(2, 3), dtype=np.float32) @ sd[u.name + ".weight"].reshape(u.cout, u.cin).T
            acts["classifier.0.convs.4"] = store(np.maximum(z + sd[u.bn + ".bias"], 0).astype(np.float32)[:, :, None, None], precision)
            continue
        if u.name == "classifier.0.project.0":
            b = [acts[reads[("classifier.0.concat", "cat%d" % i)]] for i in range(5)]
            acts["classifier.0.concat"] = np.concatenate(b[:4] + [np.broadcast_to(b[4], b[0].shape)], axis=1)
        res = acts[reads[(u.name, "res")]] if u.residual else None
        acts[u.name] = expected_unit(acts[reads[(u.name, "in")]], u, *sel[u.name], sd[u.bn + ".bias"], res, precision)
        if u.name == "backbone.conv1":
            c = np.pad(acts[u.name], ((0, 0), (0, 0), (1, 1), (1, 1)), constant_values=-np.inf)
            ho, wo = (c.shape[2] - 3) // 2 + 1, (c.shape[3] - 3) // 2 + 1
            acts["backbone.maxpool"] = np.max([c[:, :, i: i + 2 * ho: 2, j: j + 2 * wo: 2] for i in range(3) for j in range(3)], axis=0)
    return acts


def low_piece_share(x):
    """share of the elements whose f16x2 low piece is not zero"""
    return float((fb.split16(x)[1] != 0).mean())


def border_share(u, pos, h, w):
    """(share of the outputs at image-border pixels whose selected tap lies outside the image, border outputs) on an h x w input.
    A border pixel whose whole window lies inside the image does not count: the bottom row and right column of a stride-2 3x3
    convolution on an even-sized map (layer2.0.conv2 at every shape the probe runs) have no tap to lose."""
    _, outside = gather(np.zeros((1, u.cin, h, w), np.float32), u, pos)
    ho, wo = outside.shape[1:]
    border = np.zeros((ho, wo), bool)
    border[[0, -1], :] = True
    border[:, [0, -1]] = True
    first_y, first_x = u.stride * np.arange(ho) - u.pad, u.stride * np.arange(wo) - u.pad
    span = u.dil * (u.k - 1)
    reach = ((first_y < 0) | (first_y + span >= h))[:, None] | ((first_x < 0) | (first_x + span >= w))[None, :]
    border &= reach
    return float(outside[:, border].mean()), int(border.sum()) * u.cout


def first_difference(got, want, u, pos, tile):
    """None where the tensors agree word for word, else the message that names the place"""
    a, b = got.view(np.uint32), want.view(np.uint32)
    if a.shape == b.shape and np.array_equal(a, b):
        return None
    if a.shape != b.shape:
        return "%s: shape %s, expected %s" % (u.name, a.shape, b.shape)
    diff = a != b
    n, c, y, x = (int(i) for i in np.argwhere(diff)[0])
    p = int(pos[c])
    return "%s tile %s: %d of %d words differ, the first at (n, c, y, x) = %s: got %r (%08x), expected %r (%08x); its row selects " \
           "K position %d = (kh %d, kw %d, ci %d), K-step %d" % (u.name, tile, int(diff.sum()), diff.size, (n, c, y, x), float(got[n, c, y, x]),
                                                                 int(a[n, c, y, x]), float(want[n, c, y, x]), int(b[n, c, y, x]), p,
                                                                 p // u.cin // u.k, p // u.cin % u.k, p % u.cin, p // SLOTS)
