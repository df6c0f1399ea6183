"""The canvas of an outpainting edit restated in numpy: what fie_outpaint_canvas_rgb_u8 and every layer above it are held
to, byte for byte.  Written from the definition by index arithmetic:

    margins = (left, top, right, bottom), Hc = top + H + bottom, Wc = left + W + right
    canvas[y][x]      = src[clamp(y - top, 0, H - 1)][clamp(x - left, 0, W - 1)]
    canvas_mask[y][x] = 255 outside the source rectangle, mask[y - top][x - left] as passed inside it (0 without a mask)
"""
import numpy as np

MAX_OUTPAINT = 4096


def _indices(shape, margins):
    """(rows, cols, inside): the source row of every canvas row, the source column of every canvas column, and which canvas pixels lie in the
    source rectangle."""
    h, w = shape
    left, top, right, bottom = margins
    assert h >= 1 and w >= 1 and all(0 <= m <= MAX_OUTPAINT for m in margins) and any(margins)
    ys, xs = np.arange(top + h + bottom) - top, np.arange(left + w + right) - left
    inside = ((ys >= 0) & (ys < h))[:, None] & ((xs >= 0) & (xs < w))[None, :]
    return np.clip(ys, 0, h - 1), np.clip(xs, 0, w - 1), inside


def canvas(src, margins):
    """uint8 [H, W, 3] -> uint8 [Hc, Wc, 3]: the source with its edge pixels replicated into the margins."""
    src = np.asarray(src)
    assert src.dtype == np.uint8 and src.ndim == 3 and src.shape[2] == 3
    rows, cols, _ = _indices(src.shape[:2], margins)
    return np.ascontiguousarray(src[rows[:, None], cols[None, :]])


def canvas_mask(mask, shape, margins):
    """uint8 [H, W] or None, shape = (H, W) -> uint8 [Hc, Wc]: 255 in the margins, the mask as passed (greys included) or 0 over the source."""
    rows, cols, inside = _indices(shape, margins)
    if mask is None:
        inner = np.zeros(inside.shape, np.uint8)
    else:
        mask = np.asarray(mask)
        assert mask.dtype == np.uint8 and mask.shape == tuple(shape)
        inner = mask[rows[:, None], cols[None, :]]
    return np.where(inside, inner, np.uint8(255)).astype(np.uint8)


def grey_mask(h, w, seed=0):
    """A mask with every kind of value: a block of 255, a block of greys on both sides of 128, random bytes in one corner, 0 elsewhere."""
    rng = np.random.default_rng(seed + 131 * h + w)
    m = np.zeros((h, w), np.uint8)
    m[h // 4:h // 2 + 1, w // 4:w // 2 + 1] = 255
    m[h // 2:, : w // 3 + 1] = rng.choice(np.array([1, 64, 127, 128, 200, 254], np.uint8), size=m[h // 2:, : w // 3 + 1].shape)
    m[: h // 4 + 1, w - w // 4 - 1:] = rng.integers(0, 256, m[: h // 4 + 1, w - w // 4 - 1:].shape, dtype=np.uint8)
    return m
