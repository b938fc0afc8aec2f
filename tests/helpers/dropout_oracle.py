"""A numpy restatement of the library's Dropout draw (include/nbc.h, nbc_dropout_draws): Philox4x32-10,
the threshold T, the keep factor m, the per-element keep flags, and the masked classifier.4 on the CPU oracle's features.
Nothing here calls the library."""
from __future__ import annotations

import numpy as np
import torch
import torch.nn.functional as F

M0, M1 = 0xD2511F53, 0xCD9E8D57
W0, W1 = 0x9E3779B9, 0xBB67AE85
MASK32 = 0xFFFFFFFF
CIN = 512


def philox4x32_10(counter, key):
    """counter: four uint32 arrays (or ints) of one shape, key: two ints -> uint32 array [..., 4]."""
    c = [np.asarray(v, dtype=np.uint64) & np.uint64(MASK32) for v in counter]
    c = list(np.broadcast_arrays(*c))
    k0, k1 = int(key[0]) & MASK32, int(key[1]) & MASK32
    for _ in range(10):
        p0 = np.uint64(M0) * c[0]
        p1 = np.uint64(M1) * c[2]
        n0 = (p1 >> np.uint64(32)) ^ c[1] ^ np.uint64(k0)
        n2 = (p0 >> np.uint64(32)) ^ c[3] ^ np.uint64(k1)
        c = [n0, p1 & np.uint64(MASK32), n2, p0 & np.uint64(MASK32)]
        k0, k1 = (k0 + W0) & MASK32, (k1 + W1) & MASK32
    return np.stack(c, axis=-1).astype(np.uint32)


def threshold(p: float) -> int:
    """T = floor(p * 2^32) in double."""
    return int(np.floor(np.float64(p) * np.float64(4294967296.0)))


def keep_scale(p: float) -> np.float32:
    """m = float32(1) / float32(1.0 - p)."""
    return np.float32(1.0) / np.float32(np.float64(1.0) - np.float64(p))


def words(seed: int, image_id: int, draw: int, first_element: int, count: int) -> np.ndarray:
    """The random word of elements first_element .. first_element + count - 1 (uint32 [count])."""
    q0, q1 = first_element >> 2, (first_element + count + 3) >> 2
    quads = np.arange(q0, max(q1, q0 + 1), dtype=np.uint64)
    r = philox4x32_10((quads, draw, image_id & MASK32, image_id >> 32), (seed & MASK32, seed >> 32)).reshape(-1)
    off = first_element - 4 * q0
    return r[off:off + count]


def keep_flags(seed: int, image_id: int, draw: int, p: float, first_element: int, count: int) -> np.ndarray:
    """uint8 [count]: 1 = kept (word >= T)."""
    return (words(seed, image_id, draw, first_element, count).astype(np.uint64) >= np.uint64(threshold(p))).astype(np.uint8)


def keep_image(seed: int, image_id: int, draw: int, p: float, h: int, w: int) -> np.ndarray:
    """The keep flags of one image as bool [512, h, w] (element = (y * w + x) * 512 + c)."""
    k = keep_flags(seed, image_id, draw, p, 0, h * w * CIN).reshape(h, w, CIN)
    return np.ascontiguousarray(k.transpose(2, 0, 1)).astype(bool)


@torch.no_grad()
def features(oracle, x: torch.Tensor) -> torch.Tensor:
    """The input of classifier.4: post-BatchNorm, post-ReLU [N, 512, h, w]."""
    hd = oracle.classifier
    return hd[2](hd[1](hd[0](oracle.backbone(x))))


@torch.no_grad()
def masked_lowres(oracle, feats: torch.Tensor, keep: np.ndarray, p: float) -> torch.Tensor:
    """classifier.4 on feats * (m * keep): keep bool [N, 512, h, w]."""
    factor = torch.from_numpy(np.where(keep, keep_scale(p), np.float32(0)).astype(np.float32)).to(feats.dtype)
    return oracle.classifier[4](feats * factor)


@torch.no_grad()
def draw_lowres(oracle, feats: torch.Tensor, ids, seed: int, draw: int, p: float) -> torch.Tensor:
    n, _, h, w = feats.shape
    keep = np.stack([keep_image(seed, int(ids[i]), draw, p, h, w) for i in range(n)])
    return masked_lowres(oracle, feats, keep, p)


def by_hand(weight: np.ndarray, bias: np.ndarray, feats: np.ndarray, keep: np.ndarray, p: float):
    """The definition in float64 on given f32 operands: weight [3, 512], bias [3], feats [N, 512, h, w] (f32), keep bool of
    that shape.  Returns (logits f64 [N, 3, h, w], magnitude f64 [N, 3, h, w] = sum_c |w X m keep| + |bias|)."""
    masked = feats.astype(np.float64) * np.where(keep, np.float64(keep_scale(p)), 0.0)
    w64 = weight.reshape(3, CIN).astype(np.float64)
    logits = np.einsum("kc,nchw->nkhw", w64, masked) + bias.astype(np.float64)[None, :, None, None]
    mag = np.einsum("kc,nchw->nkhw", np.abs(w64), np.abs(masked)) + np.abs(bias.astype(np.float64))[None, :, None, None]
    return logits, mag


@torch.no_grad()
def upsample_labels(lowres: torch.Tensor, size):
    logits = F.interpolate(lowres, size=tuple(size), mode="bicubic", align_corners=False)
    return torch.argmax(logits, dim=1), logits
