"""Post-processing that sits between the argmax and the statistics in the reference.

``remove_small_zones`` restates /root/reference/src/bark_calculator/utils.py:135-148 (called at
``models.py:271``) on top of ``scipy.ndimage.label`` -- scikit-image, which the reference uses, is not
importable in the GPU image.  Semantics (pinned by fixtures generated with scikit-image 0.18.3,
``tests/golden/small_zones_*.npz``): with ``m = (labels == 0)`` (the "Nothing" mask),

1. ``remove_small_holes(m, area_threshold=150, connectivity=2)``: 8-connected components of ``~m``
   smaller than 150 pixels are filled (become background);
2. ``remove_small_objects(m, min_size=150, connectivity=2)``: 8-connected components of the
   *filled* ``m`` smaller than 150 pixels are removed;
3. background pixels that left the mask become class 1 (Bark); non-background pixels that
   joined it become class 0.

The reference applies it to the whole ``[1,H,W]`` batch array with a 3-D structuring element whose
in-plane slice is the 8-neighbourhood; with batch size 1 (``models.py:249-250``) that equals the
per-image 2-D operation done here.

``remove_small_zones_grouped`` is the same function on a batch of more than one image, as ``PixelWiseF1`` calls it on the
``[B,H,W]`` argmax of a validation batch (utils.py:211-214).  There the 3-D structuring element matters:
``connectivity=2`` on a 3-D array is ``generate_binary_structure(3, 2)``, the 18-neighbourhood, so a zone of image b is
linked to images b - 1 and b + 1 through the pixel at its place and that pixel's four edge neighbours, and the threshold
counts the voxels of the linked component.  It labels with the very call ``skimage.morphology.remove_small_objects`` makes
for an n-D array; scikit-image itself is not importable here, so no fixture could be recorded from the reference's own
function for more than one image -- with ``group=1`` it is ``remove_small_zones``, which the fixtures pin.
"""
from __future__ import annotations

import numpy as np
from scipy import ndimage

SMALL_ZONE_PIXELS = 150          # utils.py:140,143 (the README says 100; the code wins)
_EIGHT = np.ones((3, 3), dtype=bool)


def _drop_small_components(mask: np.ndarray, min_size: int) -> np.ndarray:
    """skimage.morphology.remove_small_objects(mask, min_size, connectivity=2) for a 2-D bool array."""
    lab, n = ndimage.label(mask, structure=_EIGHT)
    if n == 0:
        return mask.copy()
    sizes = np.bincount(lab.ravel())
    too_small = sizes < min_size
    too_small[0] = False
    out = mask.copy()
    out[too_small[lab]] = False
    return out


def remove_small_zones(labels: np.ndarray, min_pixels: int = SMALL_ZONE_PIXELS) -> np.ndarray:
    """labels: integer ``[H,W]`` or ``[N,H,W]`` class map; returns a new array of the same dtype."""
    labels = np.asarray(labels)
    if labels.ndim == 3:
        return np.stack([remove_small_zones(l, min_pixels) for l in labels])
    if labels.ndim != 2:
        raise ValueError("labels must be [H,W] or [N,H,W]")
    bg = labels == 0
    filled = ~_drop_small_components(~bg, min_pixels)        # remove_small_holes
    kept = _drop_small_components(filled, min_pixels)         # remove_small_objects
    out = labels.copy()
    out[(~kept) & (labels == 0)] = 1
    out[kept & (out != 0)] = 0
    return out


def _drop_small_components_3d(mask: np.ndarray, min_size: int) -> np.ndarray:
    """skimage.morphology.remove_small_objects(mask, min_size, connectivity=2) for a 3-D bool array."""
    lab, n = ndimage.label(mask, structure=ndimage.generate_binary_structure(3, 2))
    if n == 0:
        return mask.copy()
    too_small = np.bincount(lab.ravel()) < min_size
    too_small[0] = False
    out = mask.copy()
    out[too_small[lab]] = False
    return out


def remove_small_zones_grouped(labels: np.ndarray, group: int, min_pixels: int = SMALL_ZONE_PIXELS) -> np.ndarray:
    """``remove_small_zones`` as the reference runs it on batches: ``labels`` integer ``[N,H,W]``; consecutive groups of
    ``group`` images (the last may be shorter) each go through the three steps as one 3-D array.  Returns a new array."""
    labels = np.asarray(labels)
    group = int(group)
    if labels.ndim != 3:
        raise ValueError("labels must be [N,H,W]")
    if group < 1:
        raise ValueError("group must be >= 1")
    out = labels.copy()
    for a in range(0, len(labels), group):
        vol = labels[a:a + group]
        bg = vol == 0
        filled = ~_drop_small_components_3d(~bg, min_pixels)      # remove_small_holes
        kept = _drop_small_components_3d(filled, min_pixels)       # remove_small_objects
        res = vol.copy()
        res[(~kept) & (vol == 0)] = 1
        res[kept & (res != 0)] = 0
        out[a:a + group] = res
    return out
