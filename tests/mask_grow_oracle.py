"""`mask_grow` restated in numpy: what fie_mask_grow_u8 and every layer above it are held to, byte for byte.

    m(q) = (mask_l(q) >= 128); p, q range over the pixels of the H x W mask only
    r > 0   out(p) = 255 iff some q has m(q) and (px - qx)^2 + (py - qy)^2 <= r^2        nothing grows in from outside the image
    r < 0   out(p) = 255 iff every q with (px - qx)^2 + (py - qy)^2 <= r^2 has m(q)      the image border does not erode: ~grow(~m, -r)
    r = 0   the mask as it was passed, greys included (nothing is launched)

The OR of the zero-padded binary mask shifted over every (dx, dy) of the lattice disk (`grow_literal`; `grow` takes the shifts of one dy
together): integers only."""
import math

import numpy as np

MAX_GROW = 64


def disk(radius):
    """bool [2R + 1, 2R + 1]: the lattice points with dx^2 + dy^2 <= R^2."""
    R = abs(int(radius))
    yy, xx = np.mgrid[-R:R + 1, -R:R + 1]
    return yy * yy + xx * xx <= R * R


def grow_literal(mask_l, r):
    """The definition word for word: one shifted OR per lattice point of the disk (0.25 s at 512 x 512, r = 64)."""
    mask_l = np.asarray(mask_l)
    r = int(r)
    if r == 0:
        return mask_l.copy()
    R = abs(r)
    a = mask_l >= 128 if r > 0 else mask_l < 128
    h, w = a.shape
    p = np.zeros((h + 2 * R, w + 2 * R), bool)
    p[R:R + h, R:R + w] = a
    out = np.zeros((h, w), bool)
    for dy in range(-R, R + 1):
        for dx in range(-R, R + 1):
            if dx * dx + dy * dy <= R * R:
                out |= p[R + dy:R + dy + h, R + dx:R + dx + w]
    if r < 0:
        out = ~out
    return out.astype(np.uint8) * 255


def grow(mask_l, r):
    """grow_literal with the ORs over dx of one dy taken together: dx^2 + dy^2 <= R^2 is |dx| <= isqrt(R^2 - dy^2), and the OR over a run of
    columns is a difference of row prefix counts.  The same integers, 2R + 1 steps instead of about pi R^2."""
    mask_l = np.asarray(mask_l)
    r = int(r)
    if r == 0:
        return mask_l.copy()
    R = abs(r)
    a = mask_l >= 128 if r > 0 else mask_l < 128
    h, w = a.shape
    c = np.zeros((h + 2 * R, w + 2 * R + 1), np.int32)                   # c[y, x]: set pixels of padded row y in columns < x
    c[R:R + h, R + 1:R + 1 + w] = np.cumsum(a, axis=1)
    c[R:R + h, R + 1 + w:] = c[R:R + h, R + w:R + w + 1]
    out = np.zeros((h, w), bool)
    for dy in range(-R, R + 1):
        k = math.isqrt(R * R - dy * dy)
        rows = c[R + dy:R + dy + h]
        out |= rows[:, R + k + 1:R + k + 1 + w] > rows[:, R - k:R - k + w]
    if r < 0:
        out = ~out
    return out.astype(np.uint8) * 255


def random_mask(h, w, density, seed):
    return (np.random.default_rng(seed).random((h, w)) < density).astype(np.uint8) * 255


def grey_ramp(h, w):
    """Greys 120 .. 135 across both axes: the threshold 128 falls inside the image."""
    return (120 + (np.arange(w)[None, :] + 3 * np.arange(h)[:, None]) % 16).astype(np.uint8)


def points_mask(h, w):
    """One pixel in each corner and one at the centre."""
    m = np.zeros((h, w), np.uint8)
    for y, x in ((0, 0), (0, w - 1), (h - 1, 0), (h - 1, w - 1), (h // 2, w // 2)):
        m[y, x] = 255
    return m
