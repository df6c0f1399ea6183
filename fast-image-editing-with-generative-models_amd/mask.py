"""Host side of mask-restricted edits: mask conversion, argument checks, the feather's Gaussian taps and the
PIE-Bench run-length code.  Device-free, so all of it runs (and is tested) on the CPU; the device side is csrc/mask.hip.

A mask marks the region to edit in white.  Accepted forms: a PIL image of any mode (taken through `.convert("L")`), or a uint8 / bool
[H, W] numpy array (bool True = 255)."""
import dataclasses
import math

import numpy as np
from PIL import Image

from . import header

# masked_content: the names and codes are include/fie.h's FIE_CONTENT_* defines, in code order
CONTENT_CODES = {n[len("CONTENT_"):].lower(): v for n, v in header.DEFINES.items() if n.startswith("CONTENT_")}
CONTENT_MODES = tuple(sorted(CONTENT_CODES, key=CONTENT_CODES.get))
MAX_BLUR = 21          # radius ceil(3 r) <= 64: the LDS bound of fie_mask_prep
BLEND_MODES = ("alpha", "multiband")      # blend: the paste-back as ever, or the one-sided multi-band blend
MAX_BLEND_LEVELS = 6                      # fie_multiband_blend_rgb_u8's bound
MAX_GROW = 64                             # mask_grow: fie_mask_grow_u8's radius bound, the halo a block stages
MAX_OUTPAINT = 4096                       # outpaint: fie_outpaint_canvas_rgb_u8's bound on each of the four margins
MASK_MODES = ("binary", "levels")         # mask_mode: the mask switches the edit, or its greys are per-pixel strengths
MAX_RAMP = 64                             # mask_ramp (section 21): fie_mask_ramp_u8's radius bound, the halo a block stages


def to_l_array(mask, size=None):
    """mask -> uint8 [H, W] numpy array (mode L).  `size` (width, height): the size the mask must have (the source image's)."""
    if isinstance(mask, Image.Image):
        a = np.asarray(mask.convert("L"))
    elif isinstance(mask, np.ndarray):
        if mask.ndim != 2:
            raise ValueError(f"mask array must be [H, W], got shape {mask.shape}")
        if mask.dtype == np.bool_:
            a = mask.astype(np.uint8) * 255
        elif mask.dtype == np.uint8:
            a = mask
        else:
            raise TypeError(f"mask array dtype {mask.dtype}: uint8 or bool")
    else:
        raise TypeError(f"mask of type {type(mask).__name__}: a PIL image or a uint8 / bool numpy array")
    if size is not None and (a.shape[1], a.shape[0]) != tuple(size):
        raise ValueError(f"mask size {(a.shape[1], a.shape[0])} differs from the image size {tuple(size)}")
    return np.array(a, dtype=np.uint8, order="C")             # a writable copy (PIL arrays are read-only)


def check_args(mask_blur, paste_back, have_mask=True):
    """The argument rules of a masked edit; returns mask_blur as a float."""
    try:
        r = float(mask_blur)
    except (TypeError, ValueError):
        raise ValueError(f"mask_blur={mask_blur!r}: a number") from None
    if not (0.0 <= r <= MAX_BLUR):
        raise ValueError(f"mask_blur={mask_blur!r}: must lie in [0, {MAX_BLUR}]")
    if r > 0 and not have_mask:
        raise ValueError("mask_blur needs a mask")
    if r > 0 and not paste_back:
        raise ValueError("mask_blur feathers the paste-back: it needs paste_back=True")
    return r


def check_content(masked_content, have_mask=True):
    """The argument rules of `masked_content` (what the model starts from inside the mask); returns the mode's name."""
    if not isinstance(masked_content, str) or masked_content not in CONTENT_MODES:
        raise ValueError(f"masked_content={masked_content!r}: one of {', '.join(repr(m) for m in CONTENT_MODES)}")
    if masked_content != "original" and not have_mask:
        raise ValueError(f"masked_content={masked_content!r} needs a mask")
    return masked_content


def check_blend(blend, blend_levels=4, have_mask=True, paste_back=True):
    """The argument rules of `blend` / `blend_levels` (how the paste-back meets the source); returns (name, levels)."""
    if not isinstance(blend, str) or blend not in BLEND_MODES:
        raise ValueError(f"blend={blend!r}: one of {', '.join(repr(m) for m in BLEND_MODES)}")
    if isinstance(blend_levels, bool) or not isinstance(blend_levels, (int, np.integer)) or not 1 <= blend_levels <= MAX_BLEND_LEVELS:
        raise ValueError(f"blend_levels={blend_levels!r}: an integer in 1..{MAX_BLEND_LEVELS}")
    if blend != "alpha" and not have_mask:
        raise ValueError(f"blend={blend!r} needs a mask")
    if blend != "alpha" and not paste_back:
        raise ValueError(f"blend={blend!r} is a paste-back: it needs paste_back=True")
    return blend, int(blend_levels)


def check_grow(mask_grow, have_mask=True):
    """The argument rules of `mask_grow` (the mask grown, or with a negative value shrunk, by an exact disk of that many pixels of the mask as
    passed, before anything else reads it); returns it as an int."""
    if isinstance(mask_grow, bool) or not isinstance(mask_grow, (int, np.integer)) or not -MAX_GROW <= mask_grow <= MAX_GROW:
        raise ValueError(f"mask_grow={mask_grow!r}: an integer in {-MAX_GROW}..{MAX_GROW}")
    if mask_grow != 0 and not have_mask:
        raise ValueError("mask_grow needs a mask")
    return int(mask_grow)


def check_levels(mask_mode="binary", mask_ramp=0, mask_grow=0, have_mask=True):
    """The argument rules of `mask_mode` / `mask_ramp` (soft masks: the mask's grey level as a per-pixel strength);
    returns (mask_mode, mask_ramp as an int).  Both need a mask (an outpaint counts as one).  "levels" reads the greys as passed, so neither
    `mask_ramp` nor `mask_grow` goes with it: both work on the binarised outline and would discard them.  `mask_ramp` with `mask_grow` is fine:
    grown first, ramped second."""
    if not isinstance(mask_mode, str) or mask_mode not in MASK_MODES:
        raise ValueError(f"mask_mode={mask_mode!r}: one of {', '.join(repr(m) for m in MASK_MODES)}")
    if isinstance(mask_ramp, (bool, np.bool_)) or not isinstance(mask_ramp, (int, np.integer)) or not 0 <= mask_ramp <= MAX_RAMP:
        raise ValueError(f"mask_ramp={mask_ramp!r}: an integer in 0..{MAX_RAMP}")
    if mask_mode != "binary" and not have_mask:
        raise ValueError(f"mask_mode={mask_mode!r} needs a mask")
    if mask_ramp != 0 and not have_mask:
        raise ValueError("mask_ramp needs a mask")
    if mask_mode == "levels" and mask_ramp != 0:
        raise ValueError("mask_mode='levels' with mask_ramp: the ramp is built from the mask's outline and would discard its greys")
    if mask_mode == "levels" and mask_grow != 0:
        raise ValueError("mask_mode='levels' with mask_grow: the grown mask is binary and would discard the greys")
    return mask_mode, int(mask_ramp)


@dataclasses.dataclass(frozen=True)
class MaskSpec:
    """The mask keywords of one call, normalised: what every entry point builds once, with check(), and hands inward in place of the keywords.
    A new mask keyword is a field here, its rule in check() and its public name in keywords()."""
    blur: float = 0.0
    paste_back: bool = True
    content: str = "original"
    blend: str = "alpha"
    blend_levels: int = 4
    grow: int = 0
    mode: str = "binary"
    ramp: int = 0
    paste_later: bool = False      # the caller composites behind the job, which counts as a paste-back for `blend`

    @classmethod
    def check(cls, mask_blur=0, paste_back=True, masked_content="original", blend="alpha", blend_levels=4, mask_grow=0, mask_mode="binary",
              mask_ramp=0, *, have_mask, paste_later=False):
        """The rule sets above in the one order every entry point runs them: args, content, blend, grow, levels."""
        blur = check_args(mask_blur, paste_back, have_mask)
        content = check_content(masked_content, have_mask)
        blend, blend_levels = check_blend(blend, blend_levels, have_mask, paste_back or paste_later)
        grow = check_grow(mask_grow, have_mask)
        mode, ramp = check_levels(mask_mode, mask_ramp, grow, have_mask)
        return cls(blur, bool(paste_back), content, blend, blend_levels, grow, mode, ramp, bool(paste_later))

    @property
    def soft(self):
        """A soft mask: its readers take a MaskLevels pair."""
        return self.mode != "binary" or self.ramp != 0

    def keywords(self):
        """The spec under the public keyword names, for re-entering a public method: check(**s.keywords(), have_mask=True) == s.  `paste_later`
        is the pipeline's alone (FastEditor's methods have no such keyword) and is named only where it is set."""
        return dict(mask_blur=self.blur, paste_back=self.paste_back, masked_content=self.content, blend=self.blend, blend_levels=self.blend_levels,
                    mask_grow=self.grow, mask_mode=self.mode, mask_ramp=self.ramp, **(dict(paste_later=True) if self.paste_later else {}))

    def unmasked(self):
        """What an image without a mask of its own runs with: as without the keywords."""
        return MaskSpec(paste_back=self.paste_back, paste_later=self.paste_later)

    def behind_fullres(self):
        """The job in front of the source-size back end (output_size="source"): feather and paste-back happen there, behind it."""
        return dataclasses.replace(self, blur=0.0, paste_back=False, paste_later=True)

    def prepared(self):
        """What goes with a mask that has been grown and ramped already: a soft one is a level map, read as it is."""
        return dataclasses.replace(self, grow=0, ramp=0, mode="levels" if self.soft else "binary")


def cli_keywords(args, masked, flag):
    """The command lines' mask flags behind the parser: `args` the parsed namespace (a flag its parser lacks counts as its default), `masked`
    whether the run has a mask, `flag` the option that gives one ("--use_mask" / "--mask").  Refuses what needs a mask without one, and "levels"
    with a ramp or a grow, as a ValueError; returns edit()'s keywords for the flags that differ from their defaults."""
    get = lambda name, default: getattr(args, name, default)
    out = {}
    if get("masked_content", "original") != "original":
        if not masked:
            raise ValueError(f"--masked_content needs {flag}")
        out.update(masked_content=args.masked_content)
    if get("blend", "alpha") != "alpha":
        if not masked or get("no_paste_back", False):
            raise ValueError(f"--blend multiband needs {flag}" + (" and the paste-back" if hasattr(args, "no_paste_back") else ""))
        out.update(blend=args.blend, blend_levels=get("blend_levels", 4))
    if get("mask_grow", 0):
        if not masked:
            raise ValueError(f"--mask_grow needs {flag}")
        out.update(mask_grow=args.mask_grow)
    if get("mask_mode", "binary") != "binary" or get("mask_ramp", 0):
        if not masked:
            raise ValueError(f"--mask_mode levels and --mask_ramp need {flag}")
        if get("mask_mode", "binary") == "levels" and (get("mask_ramp", 0) or get("mask_grow", 0)):
            raise ValueError("--mask_mode levels does not go with --mask_ramp or --mask_grow: both work on the outline and would discard the greys")
        out.update(mask_mode=get("mask_mode", "binary"), mask_ramp=get("mask_ramp", 0))
    return out


def level_steps(v, K):
    """n(v, K): how many of an edit's K steps a latent pixel of level v (0..255) is edited for -- the last n.  n(0) = 0, n(1) = 1, n(255) = K."""
    return (int(v) * int(K) + 254) // 255


def level_inside(v, K, j):
    """Whether a latent pixel of level v is inside the edit in the blend after step j of K (what fie_lcm_step_levels compares): the same
    statement as level_steps(v, K) >= K - j."""
    return int(v) * int(K) > 255 * (int(K) - 1 - int(j))


def support_numpy(levels):
    """S = 255 (V > 0): the binary mask every reader but the latent step takes in a level map's place (fie_mask_support_u8)."""
    return (np.asarray(levels) > 0).astype(np.uint8) * 255


def levels_lat_numpy(levels_e, mask_lat):
    """fie_mask_levels_u8 restated: levels_e uint8 [H, W] (the level map at the edit size), mask_lat [H/8, W/8] or flat (fie_mask_prep's, of
    the support) -> uint8 [H/8, W/8]: mask_lat ? max(levels_e[8y, 8x], 1) : 0."""
    v = np.asarray(levels_e)[::8, ::8]
    m = np.asarray(mask_lat).reshape(v.shape) != 0
    return np.where(m, np.maximum(v, 1), 0).astype(np.uint8)


def _isqrt(n):
    """floor(sqrt(n)) of a non-negative int64 array: the float root is a first guess, the integers decide."""
    n = np.asarray(n, np.int64)
    s = np.sqrt(n.astype(np.float64)).astype(np.int64)
    s = np.where(s * s > n, s - 1, s)
    return np.where((s + 1) * (s + 1) <= n, s + 1, s)


def ramp_numpy(mask_l, r):
    """fie_mask_ramp_u8 restated: uint8 [H, W] mask, r in 1..64 -> the level map.  m = mask_l >= 128; D2(p) the smallest
    squared distance from p to a pixel q of the image with !m(q); V = 0 where !m, 255 where no such q lies within distance < r (a mask of all
    ones: no q at all), else isqrt(65025 D2) // r.  Integers only: per row the distance to the row's nearest unset pixel (saturated at r), then
    D2 = min over dy in -(r-1) .. r-1 of dy^2 + that distance^2 in row y + dy; rows outside the image hold no unset pixel."""
    m = np.asarray(mask_l) >= 128
    r = int(r)
    if not 1 <= r <= MAX_RAMP:
        raise ValueError(f"ramp radius {r!r}: an integer in 1..{MAX_RAMP}")
    h, w = m.shape
    far = r * r
    if m.all():                                           # no unset pixel anywhere: nothing to measure a distance to
        return np.full((h, w), 255, np.uint8)
    idx = np.arange(w, dtype=np.int64)[None, :]
    left = idx - np.maximum.accumulate(np.where(~m, idx, -4 * MAX_RAMP), axis=1)                          # to the nearest unset pixel at or left of x
    right = np.minimum.accumulate(np.where(~m, idx, w + 4 * MAX_RAMP)[:, ::-1], axis=1)[:, ::-1] - idx    # at or right of x
    hx = np.full((h + 2 * r, w), r, np.int64)             # rows above and below the image: nothing unset
    hx[r:r + h] = np.minimum(np.minimum(left, right), r)
    d2 = np.full((h, w), far, np.int64)
    for dy in range(-r + 1, r):
        d2 = np.minimum(d2, dy * dy + hx[r + dy:r + dy + h] ** 2)
    v = np.where(d2 >= far, 255, np.minimum(255, _isqrt(65025 * d2) // r))
    return np.where(m, v, 0).astype(np.uint8)


def check_outpaint(outpaint):
    """The argument rules of `outpaint` (the canvas grown by four margins of new border, which becomes the mask): None, or a
    sequence (left, top, right, bottom) of integers in 0..4096 with at least one > 0.  Returns a tuple of ints, or None.  A mask is not needed:
    the border is the mask."""
    if outpaint is None:
        return None
    ok = isinstance(outpaint, (tuple, list, np.ndarray)) and len(outpaint) == 4 and all(
        not isinstance(m, (bool, np.bool_)) and isinstance(m, (int, np.integer)) and 0 <= m <= MAX_OUTPAINT for m in outpaint)
    if not ok or not any(outpaint):
        raise ValueError(f"outpaint={outpaint!r}: None or (left, top, right, bottom), integers in 0..{MAX_OUTPAINT}, at least one > 0")
    return tuple(int(m) for m in outpaint)


def parse_outpaint(text):
    """The command lines' `--outpaint L,T,R,B` -> check_outpaint()'s tuple; anything but four comma-separated integers in range is a ValueError."""
    parts = str(text).split(",")
    try:
        margins = tuple(int(p) for p in parts)
    except ValueError:
        raise ValueError(f"--outpaint {text!r}: four comma-separated integers LEFT,TOP,RIGHT,BOTTOM") from None
    if len(margins) != 4:
        raise ValueError(f"--outpaint {text!r}: four comma-separated integers LEFT,TOP,RIGHT,BOTTOM")
    return check_outpaint(margins)


def canvas_size(size, outpaint):
    """(width, height) of the canvas of a `size` = (width, height) image under check_outpaint()'s margins (None: the image's own)."""
    if outpaint is None:
        return tuple(size)
    return size[0] + outpaint[0] + outpaint[2], size[1] + outpaint[1] + outpaint[3]


def blur_radius(r):
    return int(math.ceil(3.0 * r)) if r > 0 else 0


def gaussian_taps(r):
    """f32 [2R + 1]: exp(-k^2 / (2 r^2)) for k = -R .. R, R = ceil(3 r), normalised to sum 1 (in float64, then rounded); [1.0] for r = 0."""
    R = blur_radius(r)
    if R == 0:
        return np.ones(1, np.float32)
    k = np.arange(-R, R + 1, dtype=np.float64)
    g = np.exp(-k * k / (2.0 * r * r))
    return (g / g.sum()).astype(np.float32)


def feather_numpy(binary, r):
    """The separable feather restated (f32, horizontal pass then vertical, taps summed in order, clamp-to-edge borders)."""
    taps = gaussian_taps(r)
    R = (len(taps) - 1) // 2
    m = np.asarray(binary, np.float32)
    if R == 0:
        return m.copy()
    h, w = m.shape
    p = np.pad(m, ((0, 0), (R, R)), mode="edge")
    acc = np.zeros((h, w), np.float32)
    for k in range(2 * R + 1):
        acc = acc + taps[k] * p[:, k:k + w]
    p = np.pad(acc, ((R, R), (0, 0)), mode="edge")
    out = np.zeros((h, w), np.float32)
    for k in range(2 * R + 1):
        out = out + taps[k] * p[k:k + h, :]
    return out


def rle_decode(encoded, shape=(512, 512)):
    """PIE-Bench `mask` field -> uint8 [H, W] (255 = edit).  The code is a flat list [start, length, start, length, ...] of runs of ones
    over the row-major array (0-based starts; a run is clipped at the array's end); as the benchmark's own decoder does, the 1-pixel
    border is then set to one."""
    enc = [int(v) for v in encoded]
    if len(enc) % 2:
        raise ValueError(f"run-length mask has an odd number of entries ({len(enc)})")
    h, w = shape
    n = h * w
    flat = np.zeros(n, np.uint8)
    for start, length in zip(enc[0::2], enc[1::2]):
        if start < 0 or length < 0 or start >= n:
            raise ValueError(f"run ({start}, {length}) outside the {h}x{w} mask")
        flat[start:start + min(length, n - start)] = 1
    m = flat.reshape(h, w)
    m[0, :] = m[-1, :] = 1
    m[:, 0] = m[:, -1] = 1
    return m * np.uint8(255)


def rle_encode(mask):
    """uint8 / bool [H, W] (non-zero = edit) -> the flat [start, length, ...] list rle_decode reads."""
    flat = (np.asarray(mask).reshape(-1) != 0).astype(np.int8)
    d = np.diff(np.concatenate([[0], flat, [0]]))
    starts = np.flatnonzero(d == 1)
    ends = np.flatnonzero(d == -1)
    out = []
    for s, e in zip(starts, ends):
        out += [int(s), int(e - s)]
    return out
