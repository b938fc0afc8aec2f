"""The two tie images of the Lovasz-Softmax gradient tests (tests/test_lovasz_gradient_host.py on the restatement,
tests/test_gpu_lovasz_gradient.py on the device)."""
import numpy as np

GREYS = np.array([10, 128, 250], np.uint8)


def quantised_image(H=12, W=20, seed=3):
    """Logits that are multiples of 0.5 in [-2, 2]: many pixels share a softmax, so many errors tie, in both fg values."""
    rng = np.random.default_rng(seed)
    return (rng.integers(-4, 5, size=(3, H, W)) * 0.5).astype(np.float32), rng.choice(GREYS, size=(H, W))


def saturated_image(H=12, W=20, seed=4):
    """Logits of +-60: the float32 softmax is exactly 0 or 1, so e is exactly 0 (a right pixel) or exactly 1 (a wrong one)."""
    rng = np.random.default_rng(seed)
    hot = rng.integers(0, 3, size=(H, W))
    logits = np.where(np.arange(3)[:, None, None] == hot[None], 60.0, -60.0).astype(np.float32)
    return logits, rng.choice(GREYS, size=(H, W))
