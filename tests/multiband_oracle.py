"""Numpy restatement of the one-sided multi-band paste-back: Laplacian pyramids of the difference edit - source and of the
binary mask, the one-sided weight per level, the collapse and the final clamp / composite.  Integer arithmetic throughout (the optional feathered
composite restates image_ops.h::blend_u8 in float32), so the device agrees with it bit for bit.  `dtype` is the integer type every level is held
in: int32 is what the device uses, int64 is the run the overflow test compares it with."""
import numpy as np

K5 = (1, 4, 6, 4, 1)
MAX_LEVELS = 6


def binarise(mask_l):
    """u8 / bool [H, W] -> bool [H, W]: the edited region, L >= 128."""
    m = np.asarray(mask_l)
    return m if m.dtype == np.bool_ else m >= 128


def reduce(g):
    """[h, w, ...] -> [(h + 1) >> 1, (w + 1) >> 1, ...]: the 5x5 binomial at the even positions, indices clamped, one rounding of the 2-D sum."""
    h, w = g.shape[:2]
    h2, w2 = (h + 1) >> 1, (w + 1) >> 1
    ys = [np.clip(2 * np.arange(h2) + i, 0, h - 1) for i in range(-2, 3)]
    xs = [np.clip(2 * np.arange(w2) + j, 0, w - 1) for j in range(-2, 3)]
    rows = sum(K5[i] * g[ys[i]] for i in range(5))
    return (sum(K5[j] * rows[:, xs[j]] for j in range(5)) + 128) >> 8


def _expand_axis(g, n, axis):
    i = np.arange(n)
    Y = i >> 1
    np_ = g.shape[axis]
    lo, hi = np.clip(Y - 1, 0, np_ - 1), np.clip(Y + 1, 0, np_ - 1)
    take = lambda idx: np.take(g, idx, axis=axis)
    shape = [1] * g.ndim
    shape[axis] = n
    odd = (i & 1).astype(bool).reshape(shape)
    return np.where(odd, 4 * take(Y) + 4 * take(hi), take(lo) + 6 * take(Y) + take(hi))


def expand(g, h, w):
    """[hp, wp, ...] -> [h, w, ...]: per axis 1-6-1 at even and 4-4 at odd output indices, indices clamped, one rounding of the 2-D sum."""
    return (_expand_axis(_expand_axis(g, h, 0), w, 1) + 32) >> 6


def weight(G):
    """The one-sided ramp: 0 where the blurred mask is at most a half, 256 well inside."""
    return np.maximum(0, 2 * G - 256)


def blend_u8(m, d, s):
    """image_ops.h::blend_u8 in float32: m f32 [H, W], d f32 [H, W, 3], s u8 [H, W, 3]."""
    m = np.asarray(m, np.float32)[..., None]
    d = np.asarray(d, np.float32)
    sf = s.astype(np.float32)
    mix = np.rint(m * d + (np.float32(1) - m) * sf)          # f32 products and sum, round half to even: rintf
    return np.where(m <= 0, s, np.where(m >= 1, np.rint(d), mix).astype(np.uint8)).astype(np.uint8)


def pyramids(edit, source, mask_l, levels, dtype=np.int32):
    """-> (D, G): lists of levels 0 .. L of the difference (x16) and of the mask (x256)."""
    if not 1 <= levels <= MAX_LEVELS:
        raise ValueError(f"levels={levels}: 1..{MAX_LEVELS}")
    D = [16 * (np.asarray(edit, np.uint8).astype(dtype) - np.asarray(source, np.uint8).astype(dtype))]
    G = [256 * binarise(mask_l).astype(dtype)]
    for _ in range(levels):
        D.append(reduce(D[-1]))
        G.append(reduce(G[-1]))
    return D, G


def multiband(edit, source, mask_l, levels=4, alpha=None, dtype=np.int32):
    """edit, source u8 [H, W, 3], mask_l u8 / bool [H, W] -> u8 [H, W, 3]: B, or with `alpha` (f32 [H, W], the feathered mask_px)
    blend_u8(alpha, B, source)."""
    source = np.asarray(source, np.uint8)
    D, G = pyramids(edit, source, mask_l, levels, dtype)
    C = (weight(G[levels])[..., None] * D[levels] + 128) >> 8
    for k in range(levels - 1, -1, -1):
        h, w = G[k].shape
        lap = D[k] - expand(D[k + 1], h, w)
        C = ((weight(G[k])[..., None] * lap + 128) >> 8) + expand(C, h, w)
    B = np.clip(source.astype(dtype) + ((C + 8) >> 4), 0, 255)
    assert C.dtype == dtype
    if alpha is None:
        return B.astype(np.uint8)
    return blend_u8(alpha, B.astype(np.float32), source)


# ---- the cases both halves of the suite run
SIZES = [(1, 1), (5, 7), (24, 40), (72, 88), (64, 64), (33, 130)]


def case_images(h, w, seed):
    rng = np.random.default_rng(seed)
    return rng.integers(0, 256, (h, w, 3), dtype=np.uint8), rng.integers(0, 256, (h, w, 3), dtype=np.uint8)


def blob_mask(h, w, seed):
    """A random blob: low-pass noise thresholded at its median, as L values on either side of 128."""
    rng = np.random.default_rng(seed)
    n = rng.standard_normal((h + 8, w + 8))
    k = np.ones(9) / 9.0
    n = np.apply_along_axis(lambda r: np.convolve(r, k, "valid"), 1, n)
    n = np.apply_along_axis(lambda r: np.convolve(r, k, "valid"), 0, n)
    inside = n >= np.median(n)
    return np.where(inside, rng.integers(128, 256, (h, w)), rng.integers(0, 128, (h, w))).astype(np.uint8)
