"""Control weights, host side: the ControlNet's residuals scaled per layer, kept or dropped per step, and weighed per latent
position by the mask -- the setting, its three definitions and the numpy restatements the device ops are pinned against bit for bit.

A ControlNet hands the UNet `n_out` residuals: one per skip tensor, finest first, and the mid block's last.  `layers` gives each a factor on top of
`controlnet_conditioning_scale`; `steps` is diffusers' control_guidance_start / control_guidance_end over the loop steps that run; `in_mask` scales
the residuals inside the mask relative to outside (fie_control_pyramid_u8 makes the weights, fie_control_add applies them)."""
import collections
import math
import numbers

import numpy as np

LAYER_MIN, LAYER_MAX = 0.0, 2.0
MAX_LEVELS = 3              # levels of the weight pyramid: block sides 8, 16, 32 edit-size pixels
MAX_SEGMENTS = 16           # residuals one fie_control_add launch takes
PROMPT_BASE = 0.825         # the front ends' soft weights ("My prompt is more important")

Setting = collections.namedtuple("Setting", "layers steps in_mask")       # check()'s result: (n_out floats | None, (start, end) | None, float | None)


def _number(x):
    return isinstance(x, numbers.Real) and not isinstance(x, bool) and math.isfinite(x)


def presets(n_out):
    """The named `layers`: "prompt" 0.825 ** (n_out - 1 - i), "guess" 10 ** (-1 + i / (n_out - 1)) (diffusers' logspace(-1, 0, n_out)); float64."""
    return {"prompt": tuple(float(np.float64(PROMPT_BASE) ** (n_out - 1 - i)) for i in range(n_out)),
            "guess": tuple(float(v) for v in np.logspace(-1.0, 0.0, n_out, dtype=np.float64))}


def check(layers, steps, in_mask, n_out):
    """The setting `control_weights` normalised: None when all three are neutral, else Setting(layers, steps, in_mask) with every neutral part None.
    layers: None, "balanced" (None), "prompt", "guess", or n_out numbers in [0, 2], mid last; steps: None or (start, end), 0 <= start <= end <= 1,
    (0, 1) is None; in_mask: None or a number in [0, 1], 1 is None.  Anything else is a ValueError that names the argument."""
    if isinstance(n_out, bool) or not isinstance(n_out, numbers.Integral) or not 2 <= n_out <= MAX_SEGMENTS:
        raise ValueError(f"control weights: n_out={n_out!r}: the ControlNet's residuals, 2 .. {MAX_SEGMENTS}")
    if layers is None or (isinstance(layers, str) and layers == "balanced"):
        lay = None
    elif isinstance(layers, str):
        if layers not in ("prompt", "guess"):
            raise ValueError(f"control weights: layers={layers!r}: None, 'balanced', 'prompt', 'guess', or {n_out} numbers in [0, 2]")
        lay = presets(n_out)[layers]
    else:
        try:
            lay = tuple(layers)
        except TypeError:
            raise ValueError(f"control weights: layers={layers!r}: None, 'balanced', 'prompt', 'guess', or {n_out} numbers in [0, 2]") from None
        if len(lay) != n_out or not all(_number(v) and LAYER_MIN <= v <= LAYER_MAX for v in lay):
            raise ValueError(f"control weights: layers={layers!r}: {n_out} numbers in [0, 2], one per residual of the ControlNet, the mid block's last")
        lay = tuple(float(v) for v in lay)
        if all(v == 1.0 for v in lay):
            lay = None
    if steps is None:
        win = None
    else:
        try:
            win = tuple(steps)
        except TypeError:
            win = ()
        if len(win) != 2 or not all(_number(v) for v in win) or not 0.0 <= win[0] <= win[1] <= 1.0:
            raise ValueError(f"control weights: steps={steps!r}: None, or (start, end) with 0 <= start <= end <= 1")
        win = (float(win[0]), float(win[1]))
        if win == (0.0, 1.0):
            win = None
    if in_mask is None:
        inm = None
    else:
        if not _number(in_mask) or not 0.0 <= in_mask <= 1.0:
            raise ValueError(f"control weights: in_mask={in_mask!r}: None, or a number in [0, 1]")
        inm = None if float(in_mask) == 1.0 else float(in_mask)
    if lay is None and win is None and inm is None:
        return None
    return Setting(lay, win, inm)


def parse_env(text):
    """The one text form of a setting, `layers=prompt;steps=0:0.5;in_mask=0` (FIE_CONTROL_WEIGHTS): any subset of the three, `layers` a preset's name
    or comma-separated numbers.  -> the keywords of check() / set_control_weights.  A malformed text is a ValueError that quotes it."""
    out = {}
    bad = ValueError(f"control weights: {text!r}: 'layers=<balanced|prompt|guess|n,n,...>;steps=<start>:<end>;in_mask=<number>', any subset")
    for part in filter(None, (p.strip() for p in text.split(";"))):
        key, eq, val = (s.strip() for s in part.partition("="))
        if not eq or key not in ("layers", "steps", "in_mask") or key in out or not val:
            raise bad
        try:
            if key == "layers":
                out[key] = val if val in ("balanced", "prompt", "guess") else [float(v) for v in val.split(",")]
            elif key == "steps":
                a, colon, b = val.partition(":")
                if not colon:
                    raise bad
                out[key] = (float(a), float(b))
            else:
                out[key] = float(val)
        except ValueError:
            raise bad from None
    if not out:
        raise bad
    return out


def layer_scales(cn_scale, layers, n_out=None):
    """s_i = float32(float64(cn_scale) * float64(layer_i)) as Python floats; `layers` None: n_out ones.  With every layer 1 this is cn_scale's f32."""
    lay = (1.0,) * n_out if layers is None else layers
    return tuple(float(np.float32(np.float64(cn_scale) * np.float64(v))) for v in lay)


def keep(n_steps, steps):
    """Which of the K loop steps of an edit keep the ControlNet: step k iff not (k / K < start or (k + 1) / K > end) -- diffusers' rule, over the
    steps that run after `strength`.  steps None: all."""
    if steps is None:
        return (True,) * n_steps
    start, end = steps
    return tuple(not (k / n_steps < start or (k + 1) / n_steps > end) for k in range(n_steps))


def mask_a(in_mask):
    """a = round(256 in_mask), halves up, capped at 255: the integer the weights are made from."""
    return min(255, int(math.floor(256.0 * in_mask + 0.5)))


def level_dims(h, w, levels=MAX_LEVELS):
    """The (h_l, w_l) of the pyramid of an H x W edit (multiples of 8): h_0 = H / 8, h_{l+1} = ceil(h_l / 2) -- a stride-2 3x3 conv's sizes."""
    if h < 8 or w < 8 or h % 8 or w % 8 or not 1 <= levels <= MAX_LEVELS:
        raise ValueError(f"control weights: an edit size of {w}x{h} (multiples of 8) and 1 .. {MAX_LEVELS} levels, got {levels}")
    dims = [(h // 8, w // 8)]
    for _ in range(levels - 1):
        dims.append(((dims[-1][0] + 1) // 2, (dims[-1][1] + 1) // 2))
    return dims


def edit_ness(mask_l):
    """e of a binary L mask: 255 where it is >= 128, else 0.  (A level map is its own e.)"""
    return np.where(np.asarray(mask_l) >= 128, 255, 0).astype(np.uint8)


def pyramid_numpy(e, dims):
    """e u8 [H, W], the edit-ness of every edit-size pixel; dims: level_dims(H, W, n).  -> per level the pair of int32 [h_l, w_l] (E, cnt): the sum
    of e over the pixels [y s, min((y + 1) s, H)) x [x s, min((x + 1) s, W)), s = 8 * 2^l, and their number."""
    e = np.asarray(e)
    if e.dtype != np.uint8 or e.ndim != 2:
        raise ValueError("pyramid_numpy: e is u8 [H, W]")
    h, w = e.shape
    if [tuple(d) for d in dims] != level_dims(h, w, len(dims)):
        raise ValueError(f"pyramid_numpy: dims {list(dims)} are not the levels of a {w}x{h} edit, {level_dims(h, w, len(dims))}")
    out = []
    for l, (hl, wl) in enumerate(dims):
        s = 8 << l
        pad = np.zeros((hl * s, wl * s), np.int64)
        pad[:h, :w] = e
        one = np.zeros((hl * s, wl * s), np.int64)
        one[:h, :w] = 1
        out.append((pad.reshape(hl, s, wl, s).sum((1, 3)).astype(np.int32), one.reshape(hl, s, wl, s).sum((1, 3)).astype(np.int32)))
    return out


def weights_numpy(pyr, a):
    """(E, cnt) per level -> f32 [P_tot], all levels concatenated, finest first: w = f32(255 cnt 256 - (256 - a) E) / f32(255 cnt 256), one IEEE
    f32 division of two int32 converted to f32 (the numerator stays <= 255 * 1024 * 256 < 2^31).  a = 0: 1 - E / (255 cnt), the share of the block
    outside the mask; a full block weighs a / 256."""
    if isinstance(a, bool) or not isinstance(a, numbers.Integral) or not 0 <= a <= 255:
        raise ValueError(f"weights_numpy: a={a!r}: an integer in 0 .. 255")
    out = []
    for big_e, cnt in pyr:
        den = (255 * 256) * cnt.astype(np.int64)
        num = den - (256 - int(a)) * big_e.astype(np.int64)
        assert (num >= 0).all() and (den < 2 ** 31).all()
        out.append((num.astype(np.int32).astype(np.float32) / den.astype(np.int32).astype(np.float32)).reshape(-1))
    return np.concatenate(out).astype(np.float32)


def add_numpy(u, t, s, w, rows_per_image):
    """fie_control_add on one residual, restated: u, t [B * P, C] float16 or float32 (B batch rows of P latent positions, image-major,
    rows_per_image batch rows per image), s the residual's scale, w f32 [images, P] the weights of its level.  out = u + (s * w[p]) * t, unfused:
    c = s * w in f32, q = c * t in f32, r = u + q in f32, and for float16 one round-to-nearest-even conversion.  Where c == 0 exactly, out is u's
    bits and t is not read (a NaN there does not leak)."""
    u, t, w = np.asarray(u), np.asarray(t), np.asarray(w, np.float32)
    if u.dtype not in (np.float16, np.float32) or t.dtype != u.dtype or u.shape != t.shape or u.ndim != 2 or w.ndim != 2:
        raise ValueError("add_numpy: u, t [B * P, C] of one dtype (float16 / float32), w f32 [images, P]")
    imgs, p = w.shape
    rows = u.shape[0]
    if rows_per_image < 1 or rows % p or rows // p > imgs * rows_per_image:
        raise ValueError(f"add_numpy: {rows} rows are not up to {imgs} x {rows_per_image} batch rows of {p} positions")
    r = np.arange(rows)
    c = (np.float32(s) * w[(r // p) // rows_per_image, r % p]).astype(np.float32)
    out = u.copy()
    on = np.flatnonzero(c != 0)
    if on.size:
        with np.errstate(over="ignore", invalid="ignore"):
            q = (c[on, None] * t[on].astype(np.float32)).astype(np.float32)
            out[on] = (u[on].astype(np.float32) + q).astype(u.dtype)
    return out
