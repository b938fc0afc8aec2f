"""The label volumes the grouped remove_small_zones tests share (tests/test_grouped_host.py on the host restatement,
tests/test_gpu_grouped_zones.py on the device): hand-made tables whose answer follows from the 18-neighbourhood alone, and random
label maps."""
import numpy as np

OFFSETS = [(dy, dx) for dy in (-1, 0, 1) for dx in (-1, 0, 1)]


def offset_case(dy, dx):
    """A 2x5x5 volume for ``min_pixels=2`` as one group: a Bark pixel at (0,2,2), a Node pixel at (1, 2+dy, 2+dx).  Returns
    (labels, expected): linked through the batch axis iff |dy| + |dx| <= 1 -- then both survive, else both are removed."""
    labels = np.zeros((2, 5, 5), dtype=np.uint8)
    labels[0, 2, 2] = 1
    labels[1, 2 + dy, 2 + dx] = 2
    return labels, labels.copy() if abs(dy) + abs(dx) <= 1 else np.zeros_like(labels)


def blob_planes(planes):
    """Four 40x70 planes, a 10x10 Bark blob at rows 5..14, columns 30..39 (across the 32-column tile border) in ``planes``."""
    labels = np.zeros((4, 40, 70), dtype=np.uint8)
    for b in planes:
        labels[b, 5:15, 30:40] = 1
    return labels


# (planes with the blob, G, planes whose blob survives a threshold of 150): 100 pixels alone, 200 or 300 linked
BLOB_TABLE = [((0, 1, 2, 3), 2, (0, 1, 2, 3)), ((0, 1, 2, 3), 3, (0, 1, 2)), ((0, 1, 2, 3), 1, ()),
              ((1, 2), 2, ()), ((1, 2), 4, (1, 2))]

RANDOM_SHAPES = [(7, 33, 65), (2, 70, 200)]
RANDOM_SHARES = [0.3, 0.45, 0.6]
RANDOM_GROUPS = [1, 2, 3, 7, 8]


def random_labels(n, h, w, share0, seed=0):
    """uint8 [n,h,w]: class 0 with probability ``share0``, classes 1 and 2 mixed over the rest."""
    rng = np.random.default_rng(1000 * n + 10 * h + w + int(100 * share0) + seed)
    u = rng.random((n, h, w))
    return np.where(u < share0, 0, np.where(rng.random((n, h, w)) < 0.7, 1, 2)).astype(np.uint8)
