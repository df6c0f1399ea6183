"""Numpy restatement of the masked-content modes: the push-pull fill, the edge-map clear and the three latent rules.
Integer arithmetic throughout the fill, so the device agrees with it bit for bit.  `fill` is the vectorised form (loops over levels, slices
inside a level); `fill_loops` states the same definition cell by cell in plain Python, for the small cases that pin `fill` itself."""
import numpy as np


def binarise(mask_l):
    """u8 / bool [H, W] -> bool [H, W]: the hole, L >= 128."""
    m = np.asarray(mask_l)
    return m if m.dtype == np.bool_ else m >= 128


def _push(S, w):
    h, wd = w.shape
    h2, w2 = (h + 1) >> 1, (wd + 1) >> 1
    Sp = np.zeros((2 * h2, 2 * w2, 3), np.uint32)
    wp = np.zeros((2 * h2, 2 * w2), np.uint32)
    Sp[:h, :wd] = S
    wp[:h, :wd] = w
    return (Sp[0::2, 0::2] + Sp[0::2, 1::2] + Sp[1::2, 0::2] + Sp[1::2, 1::2],
            wp[0::2, 0::2] + wp[0::2, 1::2] + wp[1::2, 0::2] + wp[1::2, 1::2])


def _neighbours(n, n_parent):
    i = np.arange(n)
    a = i >> 1
    return a, np.clip(a + np.where(i & 1, 1, -1), 0, n_parent - 1)


def fill(src, mask_l):
    """src u8 [H, W, 3], mask_l u8 / bool [H, W] -> u8 [H, W, 3]: the hole filled, known pixels byte-identical."""
    src = np.asarray(src, np.uint8)
    m = binarise(mask_l)
    w = (~m).astype(np.uint32)
    levels = [(src.astype(np.uint32) * w[..., None], w)]
    while levels[-1][1].shape != (1, 1):
        levels.append(_push(*levels[-1]))
    C = None
    for S, w in reversed(levels):
        known = w > 0
        ww = np.where(known, w, 1).astype(np.int64)
        Ck = (256 * S.astype(np.int64) + (ww >> 1)[..., None]) // ww[..., None]
        if C is None:
            Ck[~known] = 32768
        else:
            Y, Y2 = _neighbours(w.shape[0], C.shape[0])
            X, X2 = _neighbours(w.shape[1], C.shape[1])
            up = (9 * C[Y][:, X] + 3 * C[Y][:, X2] + 3 * C[Y2][:, X] + C[Y2][:, X2] + 8) >> 4
            Ck = np.where(known[..., None], Ck, up)
        C = Ck
    return np.where(m[..., None], (C + 128) >> 8, src).astype(np.uint8)


def fill_loops(src, mask_l):
    """fill() cell by cell (slow: small images only)."""
    src = np.asarray(src, np.uint8)
    m = binarise(mask_l)
    H, W = m.shape
    S = [[[0 if m[y, x] else int(src[y, x, c]) for c in range(3)] for x in range(W)] for y in range(H)]
    w = [[0 if m[y, x] else 1 for x in range(W)] for y in range(H)]
    levels = [(S, w, H, W)]
    while (levels[-1][2], levels[-1][3]) != (1, 1):
        S, w, h, wd = levels[-1]
        h2, w2 = (h + 1) >> 1, (wd + 1) >> 1
        S2 = [[[0, 0, 0] for _ in range(w2)] for _ in range(h2)]
        ws2 = [[0] * w2 for _ in range(h2)]
        for y in range(h):
            for x in range(wd):
                ws2[y >> 1][x >> 1] += w[y][x]
                for c in range(3):
                    S2[y >> 1][x >> 1][c] += S[y][x][c]
        levels.append((S2, ws2, h2, w2))
    C = None
    for k in range(len(levels) - 1, -1, -1):
        S, w, h, wd = levels[k]
        Ck = [[None] * wd for _ in range(h)]
        for y in range(h):
            for x in range(wd):
                if w[y][x] > 0:
                    Ck[y][x] = [(256 * S[y][x][c] + (w[y][x] >> 1)) // w[y][x] for c in range(3)]
                elif C is None:
                    Ck[y][x] = [32768] * 3
                else:
                    hp, wp = levels[k + 1][2], levels[k + 1][3]
                    Y, X = y >> 1, x >> 1
                    Y2 = min(max(Y + (1 if y & 1 else -1), 0), hp - 1)
                    X2 = min(max(X + (1 if x & 1 else -1), 0), wp - 1)
                    Ck[y][x] = [(9 * C[Y][X][c] + 3 * C[Y][X2][c] + 3 * C[Y2][X][c] + C[Y2][X2][c] + 8) >> 4 for c in range(3)]
        C = Ck
    out = src.copy()
    for y in range(H):
        for x in range(W):
            if m[y, x]:
                out[y, x] = [(C[y][x][c] + 128) >> 8 for c in range(3)]
    return out


def clear_edges(ctl, mask_l):
    """ctl u8 [H, W, 3] -> the edge map with every pixel of the hole set to 0."""
    return np.where(binarise(mask_l)[..., None], 0, np.asarray(ctl, np.uint8)).astype(np.uint8)


def latent_mask(mask_l):
    """m_lat[y, x] = m_px[8y, 8x]."""
    return binarise(mask_l)[::8, ::8]


def initial_latents(mode, original, n_init, m_lat, sqrt_1mab):
    """The initial latents of a mode.  original: f32 [hw, 4], what fie_latent_prep_src writes (sqrt_ab z0 + sqrt_1mab n_init); n_init: f32 [4, hw];
    m_lat: bool [hw].  Outside the mask every mode keeps `original`; inside, latent_noise is n_init itself and latent_nothing the single f32
    product sqrt_1mab * n_init."""
    original = np.asarray(original, np.float32)
    n = np.asarray(n_init, np.float32).T
    if mode in ("original", "fill"):
        return original.copy()
    inside = {"latent_noise": n, "latent_nothing": np.float32(sqrt_1mab) * n}[mode]
    return np.where(np.asarray(m_lat, bool)[:, None], inside, original).astype(np.float32)


# ---- the cases both halves of the suite run (tests/test_masked_content_cpu.py on the restatement, tests/test_masked_content_gpu.py on the device)
def case_image(h, w, seed):
    return np.random.default_rng(seed).integers(0, 256, (h, w, 3), dtype=np.uint8)


def case_masks(h, w, seed):
    """A one-pixel hole, a rectangle touching a corner, everything but one known pixel, all ones, all zeros, a checkerboard, and L values
    127 / 128 on either side of the threshold."""
    rng = np.random.default_rng(seed)
    hole = np.zeros((h, w), np.uint8)
    hole[h // 2, w // 2] = 255
    corner = np.zeros((h, w), np.uint8)
    corner[:max(1, h // 2), :max(1, 2 * w // 3)] = 255
    one_known = np.full((h, w), 255, np.uint8)
    one_known[h - 1, w // 3] = 0
    yy, xx = np.mgrid[0:h, 0:w]
    return {"hole": hole, "corner": corner, "one_known": one_known, "ones": np.full((h, w), 255, np.uint8), "zeros": np.zeros((h, w), np.uint8),
            "checker": (((yy + xx) & 1) * 255).astype(np.uint8), "threshold": rng.choice(np.array([127, 128], np.uint8), (h, w))}
