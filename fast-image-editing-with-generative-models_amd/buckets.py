"""Output sizes of aspect-ratio edits: the SDXL resolution buckets, the choice of a bucket for a source image, and the
validation of explicit sizes.  Device-free, so all of it runs (and is tested) on the CPU.

`resolution` (FastEditor.edit / edit_batch, the CLIs' --resolution):
  None / "square"   1024x1024, the reference's size
  "auto"            the bucket whose aspect ratio is nearest the source's: smallest |log(w / h) - log(W / H)|, the larger area on a tie
  (w, h) / "WxH"    an explicit size: both sides multiples of 64, each in 512..2048, w * h <= 1024 * 1024
All sizes are (width, height), as PIL's."""
import math

SQUARE = (1024, 1024)
# the aspect-ratio buckets SDXL / SSD-1B were trained on at ~1024^2 pixels, (width, height)
BUCKETS = ((1024, 1024), (1152, 896), (896, 1152), (1216, 832), (832, 1216), (1344, 768), (768, 1344), (1536, 640), (640, 1536))
SIDE_STEP = 64
SIDE_MIN, SIDE_MAX = 512, 2048
MAX_PIXELS = 1024 * 1024
RULE = (f"both sides multiples of {SIDE_STEP}, each in {SIDE_MIN}..{SIDE_MAX}, and width * height <= {MAX_PIXELS} "
        f"(sizes above 1024^2 pixels are not supported)")


def nearest_bucket(size):
    """(width, height) of a source -> the bucket with the nearest aspect ratio (log distance); a tie goes to the larger area."""
    w, h = size
    if w <= 0 or h <= 0:
        raise ValueError(f"image size {size}: both sides must be positive")
    r = math.log(w / h)
    return min(BUCKETS, key=lambda b: (abs(r - math.log(b[0] / b[1])), -b[0] * b[1]))


def check_size(size):
    """An explicit (width, height) -> the same as a tuple of ints; ValueError names the rule when it breaks it."""
    try:
        w, h = size
    except (TypeError, ValueError):
        raise ValueError(f"resolution {size!r}: a (width, height) pair, 'square', 'auto' or 'WxH'") from None
    if isinstance(w, bool) or isinstance(h, bool) or int(w) != w or int(h) != h:
        raise ValueError(f"resolution {size!r}: integer sides; {RULE}")
    w, h = int(w), int(h)
    if w % SIDE_STEP or h % SIDE_STEP or not (SIDE_MIN <= w <= SIDE_MAX) or not (SIDE_MIN <= h <= SIDE_MAX) or w * h > MAX_PIXELS:
        raise ValueError(f"resolution {w}x{h}: {RULE}")
    return (w, h)


def parse(spec):
    """Command-line form -> "square", "auto" or a checked (width, height): "square", "auto" or "WxH" (e.g. "1152x896")."""
    s = str(spec).strip().lower()
    if s in ("square", "auto"):
        return s
    parts = s.split("x")
    if len(parts) != 2 or not all(p.strip().isdigit() for p in parts):
        raise ValueError(f"resolution {spec!r}: 'square', 'auto' or 'WxH' with {RULE}")
    return check_size((int(parts[0]), int(parts[1])))


def target_size(resolution, source_size):
    """edit()'s `resolution` and the source's (width, height) -> the (width, height) the edit runs at and returns."""
    if resolution is None:
        return SQUARE
    if isinstance(resolution, str):
        r = parse(resolution)
        if r == "square":
            return SQUARE
        if r == "auto":
            return nearest_bucket(source_size)
        return r
    return check_size(resolution)
