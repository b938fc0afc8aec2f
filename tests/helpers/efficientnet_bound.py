"""The EfficientNet kernels (csrc/efficientnet.hip, fp32) on the operands they read: the definition of every op in float64 on the
tensors read_activation returns in keep mode, and a bound on every output element, derived from the roundings the arithmetic
performs and from nothing the code under test returned.  Host only (numpy, torch on the CPU).  The conv units on conv_dma use
f32_grade_bound.conv_unit_reference / fp32_unit_bound unchanged, classifier.4 operand_bound.head_reference and the ASPP pooling
branch f32_grade_bound.pooled_reference; this file adds what only these networks have.

What is stored (read_activation, keep mode): _conv_stem and _expand_conv BEFORE their swish (dwconv applies it while staging),
_depthwise_conv after BatchNorm and swish, _se_expand the gate [N, C, 1, 1], _project_conv with its identity added, _conv_head
AFTER its swish (the swish runs in place in the conv's buffer: conv + swish is one unit here).  The gated weights and the squeeze
partials have no readable buffer; they are checked through what reads them.

u = 2^-24, gamma(n) = n u / (1 - n u).  Two figures can be neither derived nor found in the project, and are granted, not
measured, as ACCUMULATION_FACTOR is: the error of the device's expf and of the f32 division inside sigmoid (EXPF_ULPS, DIV_ULPS
below, each with its reason).  One ulp of an f32 value is at most 2 u of it, so

    sigmoid_f(x) = 1 / (1 + expf(-x))      |rel| <= gamma(2 EXPF_ULPS + 1 + 2 DIV_ULPS)     expf, the addition, the division;
                                            the error of expf reaches 1 + e scaled by e / (1 + e) < 1
    swish_f(x)   = x sigmoid_f(x)          |rel| <= gamma(2 EXPF_ULPS + 1 + 2 DIV_ULPS + 1)  and the product

  and absolutely SIGMOID_FLOOR = 2^-126, SWISH_FLOOR = 2^-119 where those do not hold: for x <= -87.4 the true sigmoid is below
  2^-126, the smallest normal f32: expf(-x) overflows or 1 / (1 + e) is subnormal, and the kernel may store +-0 or a subnormal
  with an absolute error of up to 2^-126.  |x| e^x falls for x < -1, so |swish(x)| <= 87.4 * 2^-126 < 2^-119 there.

dwconv.  v_ref = alpha sum w swish64(x~) + beta over the k x k window (a tap outside the image reads 0; without in_swish, x~
itself), y_ref = swish64(v_ref); A = sum |w| |swish64(x~)|, a = |alpha| A' with A' = (1 + s) A + SWISH_FLOOR sum |w| the
magnitudes the kernel summed (s the staging swish's relative error):

    E_v = |alpha| (s A + SWISH_FLOOR sum |w|)               the staging swish, relative to each term
        + gamma(k k) a                                       k k fmas in one chain
        + (1 + PAIR_ROUNDINGS) u ((1 + gamma(k k)) a + |beta|)   the epilogue fma and the roundings inside (alpha, beta)
    |y - y_ref| <= L E_v + s' (|y_ref| + L E_v) + SWISH_FLOOR     L = 1.1 > sup |swish'| = 1.0998 (at x = 2.3994), s' the
                                                                  output swish's own relative error

se_excite.  gate_ref in float64 from the stored depthwise output y~: m = mean over Ho Wo, r = W_r m + b_r, s = swish64(r),
q = W_e s + b_e, gate = sigmoid64(q).  Every level's bound carries the one before it through the magnitudes |W|, through L for
swish and through 1/4 = sup sigmoid' for the sigmoid; the counts (MEAN_*, SE_REDUCE_*, SE_EXPAND_*) stand next to the code they
count below.

project conv.  Evaluated per image on float32(W gate[n]) with the gate as read back: that one rounded product is what
gate_weights_kernel stores, so it is the held weight and fp32_unit_bound needs no further term (`gated_weights`).

emulate_dwconv / emulate_se_gate are the kernels' arithmetic on the CPU in numpy float32, operation by operation (an fma as the
float64 product and sum rounded to f32, as f32_grade_bound.emulate_unit_f16x2 has it; np.exp on float32 for expf), with seeded
faults; tests/test_efficientnet_bound.py shows that the bounds hold for the faithful arithmetic and reject each fault."""
from collections import namedtuple

import numpy as np

import f32_grade_bound as fb
import operand_bound as ob

U = ob.U
gamma = ob.gamma

# Granted, not measured.  HIP's math documentation gives expf a maximum error of 1 ulp; 2 are granted, the tests print what 1
# would have given.
EXPF_ULPS = 2.0
# The division.  build.py compiles .hip files with -O3 and neither -ffast-math nor -fno-hip-fp32-correctly-rounded-divide-sqrt:
# the compiler's default stands, which is a correctly rounded f32 division (0.5 ulp).  The compile line does not SAY so, and the
# grade HIP documents for the division without that default is 2.5 ulp: that is granted, and the tests print what a correctly
# rounded division would have given.
DIV_ULPS = 2.5
Grade = namedtuple("Grade", "expf_ulps div_ulps")
GRANTED = Grade(EXPF_ULPS, DIV_ULPS)
TIGHT = Grade(1.0, 0.5)
ULP = 2                                 # one ulp of an f32 value is at most 2 u of it
SIGMOID_ADD = 1                         # 1 + e
SWISH_PRODUCT = 1                       # x * sigmoid
SIGMOID_FLOOR = 2.0 ** -126             # the smallest normal f32: below it the kernel may hold 0
SWISH_FLOOR = 2.0 ** -119               # 87.4 * 2^-126 < 2^-119
SWISH_LIPSCHITZ = 1.1                   # sup |swish'| = 1.0998
SIGMOID_LIPSCHITZ = 0.25

# dwconv_kernel: a block owns TH x 16 output pixels x 32 channels (TH 8 at stride 1, 4 at stride 2), 8 pixel groups
DW_TW = 16
DW_CB = 32
DW_TH = {1: 8, 2: 4}
DW_GROUPS = 8
# se_excite_kernel
SE_WAVES = 4
SE_LANES = 64
SE_TREE = 6                             # wave_sum: the xor butterfly over 64 lanes
# the mean, two levels.  First (dwconv): a thread adds its TH * 16 / 8 pixels in a chain (`sum += v`), lane 0 of a channel the 8
# groups in a chain (7).  Second (se_excite): a wave its ceil(T / 4) tiles at most in a chain, wave 0 the four (3), the product
# with inv_hw (1), inv_hw = float(1) / float(hw) itself rounded on the host (1).  And one more: .hip files are compiled with
# the compiler's default fp-contract, which may fuse swish's product into `sum += v`; the partial then carries the unrounded
# product, at most u |v| from the stored value the reference sums.
MEAN_GROUP_CHAIN = DW_GROUPS - 1
MEAN_WAVE_CHAIN = SE_WAVES - 1
MEAN_SCALE = 2
MEAN_CONTRACTION = 1
# _se_reduce: lane l fmas channels l, l + 64, ... of the padded C in a chain (C_pad / 64), the tree (6), the bias add (1)
SE_REDUCE_BIAS = 1
# _se_expand: cse fmas in one chain, the bias add (1)
SE_EXPAND_BIAS = 1
# the depthwise epilogue: one fma, then the pair as every unit has it
DW_EPILOGUE = ob.EPILOGUE_ROUNDINGS + ob.PAIR_ROUNDINGS

DW_FAULTS = ("pads_swapped", "no_in_swish", "tap", "channel", "ragged_pixels")
SE_FAULTS = ("tile_area", "last_tile", "gate_channel")
FAULTS = DW_FAULTS + SE_FAULTS

# The cases tests/test_gpu_efficientnet_operands.py runs: (arch, (N, H, W)).  tests/test_efficientnet_bound.py asserts, without
# a GPU, what they contain between them (the cover ledger), so the list cannot thin out unnoticed.
B0F, B0D, B5F, B5D = "fcn_efficientnet_b0", "deeplabv3_efficientnet_b0", "fcn_efficientnet_b5", "deeplabv3_efficientnet_b5"
GPU_CASES = [(B0F, (2, 104, 136)), (B0F, (3, 32, 32)), (B0D, (1, 203, 317)), (B0D, (1, 40, 56)),
             (B5F, (2, 104, 136)), (B5D, (1, 72, 200))]


def sigmoid_rel(g=GRANTED):
    return gamma(ULP * g.expf_ulps + SIGMOID_ADD + ULP * g.div_ulps)


def swish_rel(g=GRANTED):
    return gamma(ULP * g.expf_ulps + SIGMOID_ADD + ULP * g.div_ulps + SWISH_PRODUCT)


def sigmoid64(x):
    x = np.asarray(x, dtype=np.float64)
    with np.errstate(over="ignore"):
        return 1.0 / (1.0 + np.exp(-x))


def swish64(x):
    x = np.asarray(x, dtype=np.float64)
    return x * sigmoid64(x)


def _per_channel(v):
    return np.asarray(v, dtype=np.float64).reshape(1, -1, 1, 1)


def pad64(c):
    return -(-c // SE_LANES) * SE_LANES


def dw_out(size, k, stride, pads):
    return (size + pads[0] + pads[1] - k) // stride + 1


def dw_tiles(stride, ho, wo):
    """(tile columns, tile rows) of a depthwise output map: dwconv_tiles_x and launch_dw's grid.y"""
    return -(-wo // DW_TW), -(-ho // DW_TH[stride])


def reads_after_pad(size, k, stride, pads):
    """whether the last output row (column) of a map of `size` input rows reads a row past the image's last one"""
    return (dw_out(size, k, stride, pads) - 1) * stride - pads[0] + k - 1 >= size


def swish_after(v_ref, e_v, g=GRANTED):
    """A swish on a value known to e_v: (y_ref, bound)"""
    y = swish64(v_ref)
    reach = SWISH_LIPSCHITZ * np.asarray(e_v, dtype=np.float64)
    return y, reach + swish_rel(g) * (np.abs(y) + reach) + SWISH_FLOOR


def dwconv_reference(x, w, alpha, beta, stride, pads, in_swish):
    """x: the stored input [N, C, Hi, Wi] f32 as read back; w: the checkpoint's [C, 1, k, k].  Returns v_ref (before the output
    swish), A = sum |w| |swish64(x~)| and sum |w| per channel, all float64."""
    w64 = np.asarray(w, dtype=np.float32).astype(np.float64)
    c, k = w64.shape[0], w64.shape[-1]
    s = np.asarray(x, dtype=np.float32).astype(np.float64)
    if in_swish:
        s = swish64(s)
    sp = np.pad(s, ((0, 0), (0, 0), (pads[0], pads[1]), (pads[0], pads[1])))
    ho, wo = dw_out(s.shape[2], k, stride, pads), dw_out(s.shape[3], k, stride, pads)
    z = np.zeros(s.shape[:2] + (ho, wo))
    mag = np.zeros_like(z)
    for kh in range(k):                                     # tap by tap (a grouped float64 conv2d of torch takes far longer)
        for kw in range(k):
            win = sp[:, :, kh: kh + (ho - 1) * stride + 1: stride, kw: kw + (wo - 1) * stride + 1: stride]
            wt = w64[:, 0, kh, kw].reshape(1, c, 1, 1)
            z += wt * win
            mag += np.abs(wt) * np.abs(win)
    v = z * _per_channel(alpha) + _per_channel(beta)
    return v, mag, np.abs(w64).sum(axis=(1, 2, 3))


def dwconv_bound(v_ref, A, wsum, alpha, beta, k, in_swish, g=GRANTED):
    """(y_ref, bound) of the depthwise unit's stored output"""
    al = np.abs(_per_channel(alpha))
    s = swish_rel(g) if in_swish else 0.0
    floor = SWISH_FLOOR * _per_channel(wsum) if in_swish else 0.0
    A = np.asarray(A, dtype=np.float64)
    staged = al * (s * A + floor)
    a = al * ((1.0 + s) * A + floor)
    e_v = staged + gamma(k * k) * a + DW_EPILOGUE * U * ((1.0 + gamma(k * k)) * a + np.abs(_per_channel(beta)))
    return swish_after(v_ref, e_v, g)


def mean_roundings(stride, tiles):
    return DW_TH[stride] * DW_TW // DW_GROUPS + MEAN_GROUP_CHAIN + -(-tiles // SE_WAVES) + MEAN_WAVE_CHAIN + MEAN_SCALE + MEAN_CONTRACTION


def gate_reference(y, wr, br, we, be, stride, g=GRANTED):
    """The SE gate from the stored depthwise output y [N, C, Ho, Wo]: (gate_ref, bound), each [N, C, 1, 1].  wr [cse, C, 1, 1],
    we [C, cse, 1, 1] and the biases are the checkpoint's."""
    y64 = np.asarray(y, dtype=np.float32).astype(np.float64)
    n, c, ho, wo = y64.shape
    tx, ty = dw_tiles(stride, ho, wo)
    wr2 = np.asarray(wr, dtype=np.float32).astype(np.float64).reshape(-1, c)
    cse = wr2.shape[0]
    we2 = np.asarray(we, dtype=np.float32).astype(np.float64).reshape(c, cse)
    br64, be64 = np.asarray(br, dtype=np.float64), np.asarray(be, dtype=np.float64)
    m = y64.mean(axis=(2, 3))
    e_m = gamma(mean_roundings(stride, tx * ty)) * np.abs(y64).mean(axis=(2, 3))
    r = m @ wr2.T + br64
    e_r = gamma(pad64(c) // SE_LANES + SE_TREE + SE_REDUCE_BIAS) * ((np.abs(m) + e_m) @ np.abs(wr2).T + np.abs(br64)) + e_m @ np.abs(wr2).T
    s, e_s = swish_after(r, e_r, g)
    q = s @ we2.T + be64
    e_q = gamma(cse + SE_EXPAND_BIAS) * ((np.abs(s) + e_s) @ np.abs(we2).T + np.abs(be64)) + e_s @ np.abs(we2).T
    gate = sigmoid64(q)
    reach = SIGMOID_LIPSCHITZ * e_q
    bound = reach + sigmoid_rel(g) * (gate + reach) + SIGMOID_FLOOR
    return gate.reshape(n, c, 1, 1), bound.reshape(n, c, 1, 1)


def gated_weights(w, gate_n):
    """float32(W gate[n]) [Co, Ci, 1, 1]: what gate_weights_kernel stores for one image, from the gate as read back [Ci]"""
    w2 = np.asarray(w, dtype=np.float32).reshape(w.shape[0], -1)
    out = w2 * np.asarray(gate_n, dtype=np.float32).reshape(1, -1)
    assert out.dtype == np.float32
    return out.reshape(w.shape[0], -1, 1, 1)


def project_reference(x, w, gate, alpha, beta, res, c=fb.ACCUMULATION_FACTOR, c_tight=1):
    """The project conv per image on its gated weights: (y_ref, bound at c, bound at c_tight) [N, Co, H, W]"""
    ys, b2, b1 = [], [], []
    for i in range(x.shape[0]):
        r = None if res is None else res[i:i + 1]
        y, mag, _ = fb.conv_unit_reference(x[i:i + 1], gated_weights(w, gate[i].reshape(-1)), "fp32", alpha, beta, r, False, 1, 0, 1)
        ys.append(y)
        b2.append(fb.fp32_unit_bound(y, mag, alpha, beta, r, x.shape[1], c))
        b1.append(fb.fp32_unit_bound(y, mag, alpha, beta, r, x.shape[1], c_tight))
    return np.concatenate(ys), np.concatenate(b2), np.concatenate(b1)


# ---- the kernels' arithmetic on the CPU ---------------------------------------------------------------------------------------
def fma32(a, b, c):
    """fmaf: the product of two f32 values is exact in float64; the sum is rounded to float64, then to f32"""
    return (np.asarray(a, np.float32).astype(np.float64) * np.asarray(b, np.float32).astype(np.float64)
            + np.asarray(c, np.float32).astype(np.float64)).astype(np.float32)


def sigmoid_f32(x):
    x = np.asarray(x, dtype=np.float32)
    with np.errstate(over="ignore"):
        e = np.exp(-x)
        out = np.float32(1.0) / (np.float32(1.0) + e)
    assert e.dtype == np.float32 and out.dtype == np.float32
    return out


def swish_f32(x):
    x = np.asarray(x, dtype=np.float32)
    return x * sigmoid_f32(x)


def tile_partials(v, stride, valid_hw):
    """The squeeze's first level as dwconv_kernel sums it: v [N, C, TY TH, TX 16] f32 over the whole tile grid, of which
    valid_hw = (Ho, Wo) is the map (None: every pixel counts -- the "ragged_pixels" fault).  Thread g of a channel adds pixels
    g PPT .. (g + 1) PPT - 1 of the tile (p = row * 16 + column) in order, then the eight groups are added in order.  Returns
    [N, T, C] with t = tile row * TX + tile column."""
    n, c, hh, ww = v.shape
    th = DW_TH[stride]
    ty, tx = hh // th, ww // DW_TW
    if valid_hw is not None:
        keep = np.zeros((hh, ww), bool)
        keep[:valid_hw[0], :valid_hw[1]] = True
        v = np.where(keep, v, np.float32(0.0))              # the kernel skips them; adding +0 leaves the same bits but for -0
    t = v.reshape(n, c, ty, th, tx, DW_TW).transpose(0, 2, 4, 1, 3, 5).reshape(n, ty * tx, c, DW_GROUPS, th * DW_TW // DW_GROUPS)
    s = np.zeros(t.shape[:-1], np.float32)
    for q in range(t.shape[-1]):
        s = s + t[..., q]
    out = s[..., 0]
    for j in range(1, DW_GROUPS):
        out = out + s[..., j]
    assert out.dtype == np.float32
    return out


def emulate_dwconv(x, w, alpha, beta, stride, pads, in_swish, fault=None):
    """dwconv_kernel on the CPU: (y [N, C, Ho, Wo], partials [N, T, C]).  fault:
      "pads_swapped"   top / left take the after-pad;
      "no_in_swish"    staging without the deferred swish;
      "tap"            pixels of the last column lose the left-hand tap of the middle kernel row (a tap inside the image);
      "channel"        scale / shift from the neighbouring channel;
      "ragged_pixels"  a ragged tile's out-of-range pixels summed into the partial (y itself is untouched)."""
    assert fault is None or fault in DW_FAULTS, fault
    x = np.asarray(x, dtype=np.float32)
    w = np.asarray(w, dtype=np.float32)
    n, c, hi, wi = x.shape
    k = w.shape[-1]
    ho, wo = dw_out(hi, k, stride, pads), dw_out(wi, k, stride, pads)
    tx, ty = dw_tiles(stride, ho, wo)
    gh, gw = ty * DW_TH[stride], tx * DW_TW                   # the tile grid's extent in output pixels
    before = pads[1] if fault == "pads_swapped" else pads[0]
    s = swish_f32(x) if in_swish and fault != "no_in_swish" else x
    need_h, need_w = (gh - 1) * stride + k, (gw - 1) * stride + k
    sp = np.zeros((n, c, max(need_h, before + hi), max(need_w, before + wi)), np.float32)     # outside the image: 0
    sp[:, :, before: before + hi, before: before + wi] = s

    def window(kh, kw):
        return sp[:, :, kh: kh + (gh - 1) * stride + 1: stride, kw: kw + (gw - 1) * stride + 1: stride]

    wc = w.reshape(1, c, k, k)
    acc = np.zeros((n, c, gh, gw), np.float32)
    lost = np.zeros((n, c, gh, gw), np.float32)               # the same chain without the tap the fault loses
    for kh in range(k):
        for kw in range(k):
            acc = fma32(window(kh, kw), wc[:, :, kh, kw, None, None], acc)
            if fault == "tap" and (kh, kw) != (k // 2, 0):
                lost = fma32(window(kh, kw), wc[:, :, kh, kw, None, None], lost)
    if fault == "tap":
        assert wo >= 2                                        # the tap lies inside the image
        acc[..., wo - 1] = lost[..., wo - 1]
    al, be = np.asarray(alpha, dtype=np.float32), np.asarray(beta, dtype=np.float32)
    if fault == "channel":
        al, be = np.roll(al, 1), np.roll(be, 1)
    v = swish_f32(fma32(acc, al.reshape(1, -1, 1, 1), be.reshape(1, -1, 1, 1)))
    assert v.dtype == np.float32
    return np.ascontiguousarray(v[:, :, :ho, :wo]), tile_partials(v, stride, None if fault == "ragged_pixels" else (ho, wo))


def emulate_se_gate(partials, ho, wo, stride, wr, br, we, be, fault=None):
    """se_excite_kernel on the CPU from the first level's partials [N, T, C]: the gate [N, C, 1, 1].  fault:
      "tile_area"     the mean divided by the tiles' area instead of Ho Wo;
      "last_tile"     the last tile's partial left out;
      "gate_channel"  the gate of the neighbouring channel."""
    assert fault is None or fault in SE_FAULTS, fault
    p = np.asarray(partials, dtype=np.float32)
    n, tiles, c = p.shape
    assert tiles == int(np.prod(dw_tiles(stride, ho, wo)))
    hw = tiles * DW_TH[stride] * DW_TW if fault == "tile_area" else ho * wo
    inv_hw = np.float32(1.0) / np.float32(hw)
    part = []
    for wv in range(SE_WAVES):
        s = np.zeros((n, c), np.float32)
        for t in range(wv * tiles // SE_WAVES, (wv + 1) * tiles // SE_WAVES):
            if not (fault == "last_tile" and t == tiles - 1):
                s = s + p[:, t]
        part.append(s)
    mean = (((part[0] + part[1]) + part[2]) + part[3]) * inv_hw
    assert mean.dtype == np.float32
    cp = pad64(c)
    wr2 = np.zeros((np.asarray(wr).shape[0], cp), np.float32)
    wr2[:, :c] = np.asarray(wr, dtype=np.float32).reshape(-1, c)
    cse = wr2.shape[0]
    mp = np.zeros((n, cp), np.float32)
    mp[:, :c] = mean
    acc = np.zeros((n, cse, SE_LANES), np.float32)
    for i in range(0, cp, SE_LANES):                        # lane l: channels l, l + 64, ... in order
        acc = fma32(wr2[None, :, i: i + SE_LANES], mp[:, None, i: i + SE_LANES], acc)
    off = SE_LANES // 2
    while off >= 1:                                         # the xor butterfly, offsets 32 down to 1: lane 0's value
        acc = acc + acc[..., np.arange(SE_LANES) ^ off]
        off //= 2
    red = swish_f32(acc[..., 0] + np.asarray(br, dtype=np.float32)[None])
    we2 = np.asarray(we, dtype=np.float32).reshape(c, cse)
    q = np.zeros((n, c), np.float32)
    for j in range(cse):
        q = fma32(we2[None, :, j], red[:, None, j], q)
    gate = sigmoid_f32(q + np.asarray(be, dtype=np.float32)[None])
    if fault == "gate_channel":
        gate = np.roll(gate, 1, axis=1)
    assert gate.dtype == np.float32
    return gate.reshape(n, c, 1, 1)
