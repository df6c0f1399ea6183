"""Edge-budget Canny restated in numpy -- TEST INFRASTRUCTURE ONLY.

Rules 1-5 of the definition on top of the numpy Canny oracle (oracle/canny.py, imported read-only): the ridge magnitudes, the budget, the pair
of thresholds and the edge map.  The budget and rule 4 are the product's own integer functions (fie_amd/canny_auto.py): one statement of each.
Also the synthetic images the CPU and GPU tests share.
"""
import numpy as np

import fie_amd  # noqa: F401
from fie_amd import canny_auto as hcanny
from oracle import canny as ocanny

FLOOR, MAX_MAGNITUDE = 16, 2040
budget = hcanny.budget


def ridge(rgb_u8):
    """u8 [H, W, 3] -> int64 [H, W]: the L1 Sobel magnitude where the pixel passes the non-maximum-suppression direction test of
    oracle.canny.canny (which gates the same test with `mag > low`), 0 elsewhere."""
    gray = ocanny.rgb_to_gray(rgb_u8)
    dx, dy = ocanny.sobel3(gray)
    mag = np.abs(dx) + np.abs(dy)
    m = np.pad(mag, 1, mode="constant")
    c = m[1:-1, 1:-1]
    left, right, up, down = m[1:-1, :-2], m[1:-1, 2:], m[:-2, 1:-1], m[2:, 1:-1]
    ul, ur, dl, dr = m[:-2, :-2], m[:-2, 2:], m[2:, :-2], m[2:, 2:]
    x = np.abs(dx).astype(np.int64)
    y = np.abs(dy).astype(np.int64) << ocanny.CANNY_SHIFT
    tg22x = x * ocanny.TG22
    tg67x = tg22x + (x << (ocanny.CANNY_SHIFT + 1))
    horiz = y < tg22x
    vert = (~horiz) & (y > tg67x)
    diag = ~(horiz | vert)
    neg = (dx ^ dy) < 0
    keep = (horiz & (c > left) & (c >= right)) | (vert & (c > up) & (c >= down)) | \
           (diag & np.where(neg, (c > ur) & (c > dl), (c > ul) & (c > dr)))
    return np.where(keep, c, 0).astype(np.int64)


def thresholds(rgb_u8, seeds, lo=100, hi=200):
    """(low, high) under a budget of `seeds` strong seeds and the ratio lo / hi (swapped when lo > hi)."""
    if lo > hi:
        lo, hi = hi, lo
    hist = np.bincount(ridge(rgb_u8).ravel(), minlength=MAX_MAGNITUDE + 2)
    above = np.concatenate([np.cumsum(hist[::-1])[::-1][1:], [0]])          # above[h] = #{r > h}
    high = next(h for h in range(FLOOR, MAX_MAGNITUDE + 1) if above[h] <= seeds)
    return hcanny.low_of(high, lo, hi), high


def canny_auto(rgb_u8, seeds, lo=100, hi=200):
    """-> (u8 [H, W, 3] edge map, (low, high)): rule 5, the oracle's Canny under the picked pair."""
    low, high = thresholds(rgb_u8, seeds, lo, hi)
    return ocanny.canny_rgb(rgb_u8, low, high), (low, high)


# ---- the images of the tests
def disks_float(seed, h=256, w=256, disks=12, sigma=5.0):
    """The generator of tests/test_ops_gpu.py::test_canny_device_bit_exact as floats, before the clip to u8: a low-frequency colour field,
    `disks` filled disks, Gaussian noise of `sigma`."""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float32)
    img = np.stack([128 + 100 * np.sin(xx / rng.uniform(5, 30) + rng.uniform(0, 6)) * np.cos(yy / rng.uniform(5, 30)) for _ in range(3)], 2)
    for _ in range(disks):
        cx, cy, r = rng.uniform(0, w), rng.uniform(0, h), rng.uniform(1, max(2, min(h, w) / 4))
        img[((xx - cx) ** 2 + (yy - cy) ** 2) < r * r] = rng.uniform(0, 255, 3)
    return img + rng.normal(0, sigma, img.shape)


def to_u8(x):
    return np.round(x).clip(0, 255).astype(np.uint8)


def low_contrast(x):
    """The float image, as far as it is visible (0 .. 255), squeezed to a quarter of its contrast around mid grey."""
    return 128 + (x.clip(0, 255) - 128) / 4


def clutter(seed, h=256, w=256):
    """One disks image under Gaussian noise of sigma 40."""
    return to_u8(disks_float(seed, h, w) + np.random.default_rng(1000 + seed).normal(0, 40, (h, w, 3)))


def stripes(h, w, width=2):
    """Vertical stripes `width` pixels wide: every ridge pixel has one magnitude.  Two pixels wide, all interior columns have the same magnitude
    and the suppression keeps one column of the image; three wide, it keeps one column per stripe edge: a third of the pixels in one histogram bin."""
    a = np.zeros((h, w, 3), np.uint8)
    a[:, (np.arange(w) // width) % 2 == 1] = 200
    return a


def long_chain(h=64, w=1024):
    """The image of tests/test_ops_gpu.py::test_canny_device_long_chain: a ridge of magnitude 120 along the whole width, one strong seed at its left end."""
    img = np.full((h, w, 3), 100, np.uint8)
    img[h // 2:, :, :] = 130
    img[h // 2:, :8, :] = 200
    return img


def flat(h, w):
    return np.full((h, w, 3), 77, np.uint8)


def plus_minus_one(h, w, seed=0):
    """Grey levels 127 / 128 / 129 at random: quantisation noise alone."""
    g = np.random.default_rng(seed).integers(127, 130, (h, w)).astype(np.uint8)
    return np.stack([g, g, g], 2)
