"""A bf16 kernel on the operands it read: the definition in float64 and a bound on every output element, derived from the
roundings the arithmetic performs and from nothing the code under test returned.  Host only (numpy, torch on the CPU).

A bf16 conv unit reads bf16 activations x^ and bf16 weights w^, sums their products in f32 (a product of two bf16 values has
16 significant bits: exact in f32), applies its f32 (alpha, beta) pair with one fma, adds the bf16 residual, takes the ReLU and
stores bf16, rounded to nearest even.  With u = 2^-24, u_b = 2^-8 (bf16 keeps 8 significant bits), K = Cin k k and
A = sum |w^| |x^|, every stored element y satisfies

    |y - y_ref| <= u_b |y_ref| + (1 + u_b) [ c K u |alpha| A + 6 u (|alpha| A + |beta| + |res|) ] + 2^-120

  K u A        K f32 additions in any order (Higham, Accuracy and Stability of Numerical Algorithms, section 4.2);
  c = 2        granted, not measured: the matrix pipe's internal summation is not documented to round every addition to nearest;
  6 u          the epilogue's fma (1), the residual add (1), and up to four f32 roundings inside the pair -- invstd's sqrt and
               division, alpha's product, beta's product and difference reach a value through at most four of them
               (PAIR_ROUNDINGS); where the restated pair equals the packer's bit for bit this part is slack;
  u_b |y_ref|  the store, and (1 + u_b) because it rounds the computed value, not y_ref;
  2^-120       an absolute floor for flushed subnormals.

The other ops follow the same rule -- n roundings of u times the sum of magnitudes, plus u_b |y| where the result is stored
as bf16 --, each count next to its constant below.

emulate_unit is the kernel's arithmetic on the CPU with four seeded faults; tests/test_operand_bound.py uses it to show that
the bound holds for the faithful arithmetic and rejects each fault.  No GPU run of a broken kernel is needed for that."""
import numpy as np
import torch
import torch.nn.functional as F

U = 2.0 ** -24
U_B = 2.0 ** -8
FLOOR = 2.0 ** -120
BN_EPS = np.float32(1e-5)
# the matrix pipe's accumulation: c K u A
ACCUMULATION_FACTOR = 2
# behind the accumulation: the epilogue's fma, the residual add, four inside (alpha, beta)
EPILOGUE_ROUNDINGS = 1
RESIDUAL_ROUNDINGS = 1
PAIR_ROUNDINGS = 4
UNIT_ROUNDINGS = EPILOGUE_ROUNDINGS + RESIDUAL_ROUNDINGS + PAIR_ROUNDINGS
# classifier.4 (head1x1): f32 weights on the stored features, K fmas and adds in a chain and a tree (at most K roundings on any
# path), the bias add, and one of slack: (K + 2) u (sum |w x| + |bias|)
HEAD_EXTRA_ROUNDINGS = 2
FAULTS = ("truncate", "kstep", "alpha", "tap")


def gamma(n):
    """n roundings of u compounded: (1 + u)^n - 1 <= n u / (1 - n u)."""
    return n * U / (1.0 - n * U)


def bf16_round(a):
    """float32 -> the nearest bf16 (ties to even, NaN stays NaN), returned as float32: f32_to_bf16 of csrc/nbc_net.cpp."""
    bits = np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)
    nan = (bits & np.uint32(0x7fffffff)) > np.uint32(0x7f800000)
    rounded = (bits + (np.uint32(0x7fff) + ((bits >> np.uint32(16)) & np.uint32(1)))) & np.uint32(0xffff0000)
    return np.where(nan, (bits & np.uint32(0xffff0000)) | np.uint32(0x00400000), rounded).astype(np.uint32).view(np.float32)


def bf16_truncate(a):
    """float32 -> bf16 by dropping the low 16 bits (the fault a 16-bit shift in the store would be)."""
    bits = np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)
    return (bits & np.uint32(0xffff0000)).view(np.float32)


def bf16_weights(w):
    """The checkpoint's f32 weights as the packer stores them: torch.bfloat16 (round to nearest even), as a float32 tensor."""
    return torch.from_numpy(np.ascontiguousarray(w, dtype=np.float32)).to(torch.bfloat16).to(torch.float32)


def bn_pair(gamma_, bias, mean, var, eps=BN_EPS):
    """(alpha, beta) as nbc_pack_weights computes them, in float32 operation by operation."""
    g, b, mu, v = (np.asarray(t, dtype=np.float32) for t in (gamma_, bias, mean, var))
    invstd = np.float32(1.0) / np.sqrt(v + np.float32(eps))
    alpha = g * invstd
    beta = b - mu * alpha
    assert invstd.dtype == alpha.dtype == beta.dtype == np.float32
    return alpha, beta


def _per_channel(v):
    return np.asarray(v, dtype=np.float64).reshape(1, -1, 1, 1)


def conv_unit_reference(x, w, alpha, beta, res, relu, stride, pad, dil):
    """x, res: float32 arrays that hold bf16 values (as read back); w: f32 checkpoint weights, rounded here.  Returns
    y_ref = act(z alpha + beta + res) in float64 with z = sum w^ x^ from a float64 conv2d, and A = sum |w^| |x^| (float32
    conv2d: a magnitude)."""
    xh, wh = torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)), bf16_weights(w)
    with torch.no_grad():
        z = F.conv2d(xh.double(), wh.double(), stride=stride, padding=pad, dilation=dil).numpy()
        mag = F.conv2d(xh.abs(), wh.abs(), stride=stride, padding=pad, dilation=dil).numpy()
    y = z * _per_channel(alpha) + _per_channel(beta)
    if res is not None:
        y = y + np.asarray(res, dtype=np.float64)
    if relu:
        y = np.maximum(y, 0.0)
    return y, mag


def bf16_unit_bound(y_ref, A, alpha, beta, res, K, c=ACCUMULATION_FACTOR):
    a = np.abs(_per_channel(alpha)) * np.asarray(A, dtype=np.float64)
    r = 0.0 if res is None else np.abs(np.asarray(res, dtype=np.float64))
    return (U_B * np.abs(y_ref) + (1.0 + U_B) * (c * K * U * a + UNIT_ROUNDINGS * U * (a + np.abs(_per_channel(beta)) + r))
            + FLOOR)


def head_reference(x, w, bias):
    """classifier.4 on the stored features: (y_ref, bound) with the checkpoint's f32 weights [3, K, 1, 1]."""
    w2 = np.asarray(w, dtype=np.float64).reshape(w.shape[0], -1)
    x64 = np.asarray(x, dtype=np.float64)
    y = np.einsum("ok,nkhw->nohw", w2, x64) + _per_channel(bias)
    mag = np.einsum("ok,nkhw->nohw", np.abs(w2), np.abs(x64)) + np.abs(_per_channel(bias))
    return y, (w2.shape[1] + HEAD_EXTRA_ROUNDINGS) * U * mag + FLOOR


def pooled_reference(x, w, alpha, beta):
    """The ASPP pooling branch on the stored trunk x [N, K, H, W]: the mean over H W pixels, the 1x1 conv with the
    checkpoint's f32 weights [Cout, K, 1, 1], the pair, the ReLU, the bf16 store.  Roundings on the way to the f32 value: H W
    for the mean (H W - 1 additions in two levels and the division), K for the conv (K fmas and additions in a chain and a
    tree: at most K on any path), compounded: gamma(H W + K) |alpha| A with A = sum |w| mean|x|; then UNIT_ROUNDINGS less the
    residual's, and the store.  Returns (y_ref, bound), each [N, Cout, 1, 1]."""
    n, k, h, wd = x.shape
    w2 = np.asarray(w, dtype=np.float64).reshape(w.shape[0], k)
    x64 = np.asarray(x, dtype=np.float64)
    z = x64.mean(axis=(2, 3)) @ w2.T
    a = np.abs(x64).mean(axis=(2, 3)) @ np.abs(w2).T * np.abs(np.asarray(alpha, dtype=np.float64))
    al, be = np.asarray(alpha, dtype=np.float64), np.asarray(beta, dtype=np.float64)
    y = np.maximum(z * al + be, 0.0)
    bound = U_B * np.abs(y) + (1.0 + U_B) * (gamma(h * wd + k) * a + (UNIT_ROUNDINGS - RESIDUAL_ROUNDINGS) * U * (a + np.abs(be))) + FLOOR
    return y.reshape(n, -1, 1, 1), bound.reshape(n, -1, 1, 1)


def emulate_unit(x, w, alpha, beta, res, relu, stride, pad, dil, fault=None):
    """The kernel's arithmetic on the CPU: bf16 operands, an f32 conv2d, the f32 fma with the pair, the f32 residual add, the
    ReLU, round to nearest even to bf16.  fault:
      "truncate"  the store drops the low 16 bits instead of rounding;
      "kstep"     one K-step (64 bf16 channels of one tap: channels 64..127 of the centre tap) is left out;
      "alpha"     alpha is taken from the neighbouring channel;
      "tap"       pixels of the last column lose the left-hand tap of the middle row of a 3x3 kernel (a tap inside the image)."""
    assert fault is None or fault in FAULTS, fault
    xh, wh = torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)), bf16_weights(w)
    k = wh.shape[-1]
    kw = dict(stride=stride, padding=pad, dilation=dil)
    with torch.no_grad():
        if fault == "kstep":
            assert wh.shape[1] >= 128
            wh = wh.clone()
            wh[:, 64:128, k // 2, k // 2] = 0.0
        z = F.conv2d(xh, wh, **kw)
        if fault == "tap":
            assert k == 3
            less = wh.clone()
            less[:, :, 1, 0] = 0.0
            z[..., -1] = F.conv2d(xh, less, **kw)[..., -1]
    al = np.roll(np.asarray(alpha, dtype=np.float32), 1) if fault == "alpha" else alpha
    # fma: the product of two f32 values is exact in float64; the sum is rounded to float64, then to f32
    v = (z.numpy().astype(np.float64) * _per_channel(al) + _per_channel(beta)).astype(np.float32)
    if res is not None:
        v = v + np.asarray(res, dtype=np.float32)
    if relu:
        v = np.maximum(v, np.float32(0.0))
    assert v.dtype == np.float32
    return bf16_truncate(v) if fault == "truncate" else bf16_round(v)
