"""Helpers of the colour-match tests (test infrastructure): the seeded cases, the masks of the region threshold and the
synthetic picture of the check of purpose.  The definition itself is `fie_amd/colour.py`; nothing here restates it."""
import numpy as np

SIZES = [(1, 1), (3, 5), (17, 31), (64, 64), (250, 333)]
AMOUNTS = [1, 128, 256]


def case(h, w, seed):
    """(E, S, L): S random bytes, E the source under a per-channel cast of (0.8x + 30, 1.1x - 10, x + 6) plus noise, L a random mask of L values
    on either side of 128 that leaves a good half outside."""
    rng = np.random.default_rng(seed)
    s = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    gain, off = np.array([0.8, 1.1, 1.0]), np.array([30.0, -10.0, 6.0])
    e = np.clip(np.rint(s * gain + off + rng.normal(0, 2, s.shape)), 0, 255).astype(np.uint8)
    inside = rng.random((h, w)) < 0.4
    l = np.where(inside, rng.integers(128, 256, (h, w)), rng.integers(0, 128, (h, w))).astype(np.uint8)
    return e, s, l


def mask_with_background(h, w, n_bg):
    """u8 [h, w]: 255 everywhere but n_bg pixels of 0, spread over the image."""
    l = np.full(h * w, 255, np.uint8)
    l[(np.arange(n_bg) * (h * w)) // max(n_bg, 1)] = 0
    assert int((l < 128).sum()) == n_bg
    return l.reshape(h, w)


def disks_on_gradient(size=96, seed=5):
    """The synthetic picture of the check of purpose: filled disks on a colour gradient."""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:size, 0:size].astype(np.float64) / size
    img = np.stack([40 + 170 * xx, 60 + 120 * yy, 200 - 150 * xx * yy], axis=2)
    for _ in range(5):
        cx, cy, r = rng.uniform(0.1, 0.9), rng.uniform(0.1, 0.9), rng.uniform(0.06, 0.18)
        img[(xx - cx) ** 2 + (yy - cy) ** 2 < r * r] = rng.uniform(20, 235, 3)
    return np.clip(np.rint(img), 0, 255).astype(np.uint8)


def cast(img, gain, offset):
    return np.clip(np.rint(img.astype(np.float64) * np.asarray(gain) + np.asarray(offset)), 0, 255).astype(np.uint8)
