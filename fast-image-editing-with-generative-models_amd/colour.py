"""Colour match: the definition, in Python integers.

An edit's colour cast is pulled back to its source by a per-channel affine map from first and second moments (Reinhard's statistics transfer, in
RGB), measured where the picture was not supposed to change.  This module holds the range of the amount and the definition as a numpy / Python-int
restatement: the statistics, the region rule, the gain, the 3 x 256 LUT and the matched image.  It is the reference a device op is to be pinned
against byte for byte; the device op, its C ABI and the editor's setting are NOT in the tree (DESIGN.md section 24 says why), and nothing in the
product calls this module yet.
"""
import numpy as np

MAX_PIXELS = 1 << 22
GAIN_ONE, GAIN_MIN, GAIN_MAX = 1024, 512, 2048          # Q10
REGIONS = ("image", "background")                        # report word 0


def check(amount):
    """None, or the amount as a float in (0, 1]; anything else is a ValueError."""
    if amount is None:
        return None
    if isinstance(amount, bool) or not isinstance(amount, (int, float)) or not 0.0 < float(amount) <= 1.0:
        raise ValueError(f"colour_match={amount!r}: None, or a number in (0, 1] (how far the edit's colours are pulled back to the source's; "
                         "front ends use 1.0)")
    return float(amount)


def amount_q8(amount):
    """The amount the device is handed: a = round(256 * amount), at least 1."""
    return max(1, int(round(256 * check(amount))))


def _images(edit, source, mask_l):
    e, s = np.asarray(edit), np.asarray(source)
    if e.dtype != np.uint8 or s.dtype != np.uint8 or e.ndim != 3 or e.shape[2] != 3 or e.shape != s.shape:
        raise ValueError(f"colour match: two uint8 [H, W, 3] images of one size, got {e.shape} {e.dtype} and {s.shape} {s.dtype}")
    if e.shape[0] * e.shape[1] < 1 or e.shape[0] * e.shape[1] > MAX_PIXELS:
        raise ValueError(f"colour match: {e.shape[0]} x {e.shape[1]} outside 1 .. 2^22 pixels")
    m = None
    if mask_l is not None:
        m = np.asarray(mask_l)
        if m.dtype != np.uint8 or m.shape != e.shape[:2]:
            raise ValueError(f"colour match: the mask must be uint8 {e.shape[:2]}, got {m.shape} {m.dtype}")
    return e, s, m


def stats_numpy(edit, source, mask_l=None):
    """The 26 statistics as Python ints: two sets {n, Se[3], Qe[3], Ss[3], Qs[3]}, set 0 over the pixels with L < 128 (every pixel without a
    mask), set 1 over those with L >= 128."""
    e, s, m = _images(edit, source, mask_l)
    inside = np.zeros(e.shape[:2], bool) if m is None else m >= 128
    out = []
    for sel in (~inside, inside):
        ev, sv = e[sel].astype(np.int64), s[sel].astype(np.int64)         # [n, 3]
        out += [int(sel.sum())] + [int(x) for x in ev.sum(0)] + [int(x) for x in (ev * ev).sum(0)]
        out += [int(x) for x in sv.sum(0)] + [int(x) for x in (sv * sv).sum(0)]
    return out


def gain_q10(n, se, qe, ss, qs):
    """The gain: 1024 for a flat edit, else the largest g in 512 .. 2048 with g^2 ve <= vs << 20 (512 if none)."""
    ve, vs = (n * qe - se * se) // n, (n * qs - ss * ss) // n
    if ve == 0:
        return GAIN_ONE
    g = GAIN_MIN
    for cand in range(GAIN_MIN, GAIN_MAX + 1):            # a plain loop: the definition, not the device's bisection
        if cand * cand * ve <= vs << 20:
            g = cand
    return g


def lut_numpy(edit, source, mask_l=None, a=256):
    """-> (LUT uint8 [3, 256], report): report = dict(region="background" / "image", gain=[g] * 3 (Q10 ints), shift=[LUT_c[128] - 128] * 3, n)."""
    if isinstance(a, bool) or not isinstance(a, int) or not 1 <= a <= 256:
        raise ValueError(f"colour match: a={a!r} outside 1 .. 256")
    e, _, m = _images(edit, source, mask_l)
    st = stats_numpy(edit, source, mask_l)
    hw = e.shape[0] * e.shape[1]
    bg = m is not None and st[0] * 16 >= hw               # at least ceil(hw / 16) pixels of L < 128
    word = (lambda k: st[k]) if bg else (lambda k: st[k] + st[13 + k])
    n = word(0)
    lut = np.empty((3, 256), np.uint8)
    gains = []
    for c in range(3):
        se, qe, ss, qs = word(1 + c), word(4 + c), word(7 + c), word(10 + c)
        g = gain_q10(n, se, qe, ss, qs)
        gains.append(g)
        for v in range(256):
            t = g * (v * n - se) + 1024 * ss
            mv = min(max((t + 512 * n) // (1024 * n), 0), 255)
            lut[c, v] = (v * (256 - a) + mv * a + 128) >> 8
    return lut, dict(region=REGIONS[int(bg)], gain=gains, shift=[int(lut[c, 128]) - 128 for c in range(3)], n=n)


def match_numpy(edit, source, mask_l=None, a=256):
    """The matched image E': every byte of `edit` through its channel's LUT, inside the mask too (uncomposited)."""
    lut, _ = lut_numpy(edit, source, mask_l, a)
    e = np.asarray(edit)
    return np.stack([lut[c][e[..., c]] for c in range(3)], axis=2)


def report_dict(words):
    """Eight report words {region, g[3], LUT_c[128] - 128, n} as the three metric keys: colour_gain, colour_shift, colour_region."""
    w = [int(x) for x in words[:8]]
    return dict(colour_gain=[w[1 + c] / GAIN_ONE for c in range(3)], colour_shift=[w[4 + c] for c in range(3)], colour_region=REGIONS[w[0]])
