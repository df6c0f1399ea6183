"""Host side of full-resolution edits: which box of the source a region edit crops, the argument rules of
`output_size` / `region`, and a numpy restatement of the device back end (csrc/fullres.hip).  Device-free, so all of it runs (and is
tested) on the CPU.

`output_size` (FastEditor.edit / edit_batch, the CLIs' --output_size):
  None / "edit"     the result at the size the edit ran at (the default without a region)
  "source"          the result at the source image's own (width, height), composited there against the source's own bytes
`region` (the CLIs' --region):
  None              the whole image is edited
  "mask"            the edit runs on a crop around the mask's selection (`mask_box`) and the output is the source with that crop edited
  (l, t, r, b)      the same with an explicit box in source pixels (PIL's crop convention: r and b are exclusive), used as given
A region implies output_size="source".

The box of region="mask" (`mask_box`), all in integers:
  1. the bounding box of `mask_l >= 128` (l, t inclusive; r, b exclusive); an empty selection is a ValueError;
  2. grown by `padding` pixels on each side and clipped to the image: sides bw, bh;
  3. (tw, th) = buckets.target_size(resolution, (bw, bh)): None is square, "auto" the bucket nearest the padded box;
  4. one axis grows so the box has the target's aspect: want_w = max(bw, ceil(bh * tw / th)), want_h = max(bh, ceil(bw * th / tw)),
     each capped at the image's side;
  5. the growth is centred: l -= (want_w - bw) // 2, t -= (want_h - bh) // 2, and the box is shifted back inside the image;
  6. sides below 16 pixels are a ValueError.
For example on a 400x300 image with padding 10 and a square target: a mask over x 100..180, y 120..160 gives (90, 90, 190, 190), one over
x 0..50, y 0..20 gives (0, 0, 60, 60), one over x 10..390, y 100..200 gives (0, 0, 400, 300)."""
import numpy as np

from . import buckets
from . import mask as hmask
from . import resize

MIN_SIDE = 16
OUTPUT_SIZES = (None, "edit", "source")


def check_output(output_size, region):
    """The argument rules of `output_size` and `region` -> True when the result is returned at the source's size.  None is the default and
    means "not asked for": the edit size without a region, the source's size with one.  "edit" asks for the edit size in so many words,
    which a region edit cannot return: a ValueError."""
    if not (output_size is None or isinstance(output_size, str)) or output_size not in OUTPUT_SIZES:
        raise ValueError(f"output_size={output_size!r}: None, 'edit' or 'source'")
    if region is None:
        return output_size == "source"
    if output_size == "edit":
        raise ValueError("output_size='edit' with a region: a region edit returns the source-size image (output_size='source')")
    return True


def check_box(box, size):
    """An explicit (l, t, r, b) in source pixels -> the same as a tuple of ints; ValueError when it is not inside the image or a side is
    below 16."""
    try:
        l, t, r, b = box
    except (TypeError, ValueError):
        raise ValueError(f"region {box!r}: None, 'mask' or a (left, top, right, bottom) box") from None
    if any(isinstance(v, bool) or int(v) != v for v in (l, t, r, b)):
        raise ValueError(f"region {box!r}: integer coordinates")
    l, t, r, b = int(l), int(t), int(r), int(b)
    w, h = size
    if not (0 <= l < r <= w and 0 <= t < b <= h):
        raise ValueError(f"region {(l, t, r, b)} does not lie inside the {w}x{h} image")
    if r - l < MIN_SIDE or b - t < MIN_SIDE:
        raise ValueError(f"region {(l, t, r, b)}: both sides must be at least {MIN_SIDE} pixels")
    return (l, t, r, b)


def mask_box(mask_l, padding=32, resolution=None):
    """uint8 [H, W] mode-L mask -> the (l, t, r, b) box region="mask" edits (the module docstring spells the rule out)."""
    m = np.asarray(mask_l)
    if m.ndim != 2:
        raise ValueError(f"mask array must be [H, W], got shape {m.shape}")
    if isinstance(padding, bool) or int(padding) != padding or padding < 0:
        raise ValueError(f"region_padding={padding!r}: a non-negative integer")
    padding = int(padding)
    h, w = m.shape
    sel = m >= 128
    ys, xs = np.flatnonzero(sel.any(axis=1)), np.flatnonzero(sel.any(axis=0))
    if len(ys) == 0:
        raise ValueError("region='mask': the mask selects nothing (no pixel >= 128)")
    l, t, r, b = int(xs[0]), int(ys[0]), int(xs[-1]) + 1, int(ys[-1]) + 1
    l, t, r, b = max(l - padding, 0), max(t - padding, 0), min(r + padding, w), min(b + padding, h)
    bw, bh = r - l, b - t
    tw, th = buckets.target_size(resolution, (bw, bh))
    want_w = min(max(bw, -(-bh * tw // th)), w)
    want_h = min(max(bh, -(-bw * th // tw)), h)
    l -= (want_w - bw) // 2
    t -= (want_h - bh) // 2
    l = min(max(l, 0), w - want_w)
    t = min(max(t, 0), h - want_h)
    if want_w < MIN_SIDE or want_h < MIN_SIDE:
        raise ValueError(f"region='mask': the box {(l, t, l + want_w, t + want_h)} has a side below {MIN_SIDE} pixels")
    return (l, t, l + want_w, t + want_h)


def resolve(region, size, mask_l=None, padding=32, resolution=None):
    """edit()'s `region` -> None or the checked (l, t, r, b) box.  `size`: the source's (width, height); `mask_l`: its uint8 [H, W] mask or None."""
    if region is None:
        return None
    if isinstance(region, str):
        if region != "mask":
            raise ValueError(f"region {region!r}: None, 'mask' or a (left, top, right, bottom) box")
        if mask_l is None:
            raise ValueError("region='mask' needs a mask")
        return mask_box(mask_l, padding, resolution)
    return check_box(region, size)


def paste(image, crop_out, box):
    """The host's last step of a region edit: a copy of the source converted to RGB with the composited crop pasted at the box's corner."""
    full = image.convert("RGB").copy()
    full.paste(crop_out, (box[0], box[1]))
    return full


def fullres_paste_numpy(res, source, mask_l=None, blur=0.0):
    """The device back end restated (CPU checker; the product path is csrc/fullres.hip).  res: uint8 [h, w, 3], the edit-size result; source:
    uint8 [H, W, 3]; mask_l: None or uint8 [H, W].  -> uint8 [H, W, 3]: up = Pillow's LANCZOS resize of res to the source's size
    (resize.resample_numpy); without a mask the output is up; with one, M = feather_numpy(mask_l >= 128, blur) and the output is the source
    where M <= 0, up where M >= 1 and rint(M up + (1 - M) source) in f32 between."""
    source = np.asarray(source, np.uint8)
    H, W, _ = source.shape
    up = resize.resample_numpy(np.asarray(res, np.uint8), H, W)
    if mask_l is None:
        return up
    m = hmask.feather_numpy(np.asarray(mask_l) >= 128, blur)[..., None]
    one = np.float32(1.0)
    mix = np.rint(m * up.astype(np.float32) + (one - m) * source.astype(np.float32))
    return np.where(m <= 0, source, np.where(m >= 1, up, mix.clip(0, 255).astype(np.uint8))).astype(np.uint8)
