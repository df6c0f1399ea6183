"""Tiled edits: the plan that covers a W x H image with edit-size tiles, the split of the tiles into device jobs and
a numpy restatement of the device blend (csrc/tile_blend.hip).  Device-free and all in integers, so all of it runs (and is tested) on the CPU.

`tiles` (FastEditor.edit / edit_batch, the CLIs' --tiles):
  None              the feature is off
  "auto"            per axis the smallest legal tile side that still overlaps its neighbours by `tile_overlap`
  (tw, th) / "WxH"  an explicit tile size (buckets.check_size: multiples of 64, 512..2048, tw * th <= 1024^2)
`tile_overlap`: 0..256 pixels every pair of neighbouring tiles shares at least; `tile_batch`: 1..16 tiles per device job.

The plan of one axis -- S the image side, o the overlap, t the tile side, n tiles at p_0 .. p_(n-1):
  explicit t        S < t is a ValueError; S == t is the one tile [0]; else n = max(2, ceil((S - o) / (t - o)))
  "auto"            S < 512 is a ValueError; S <= 1024 and S % 64 == 0 is the one tile t = S; else n = max(2, ceil((S - o) / (1024 - o))) and
                    t = max(512, 64 * ceil(ceil((S + (n - 1) o) / n) / 64))
  positions         p_i = (i (S - t)) // (n - 1): the first tile at 0, the last one flush with the far border, the rest spread evenly
More than 32 tiles on an axis is a ValueError.  Tile j = iy * nx + ix (row-major) is the box (xs[ix], ys[iy], xs[ix] + tw, ys[iy] + th).

The blend: a tile's weight at its own pixel (v, u) is wy(v) * wx(u) with w(u) = min(t if first else u + 1, t if last else t - u) per axis -- the
distance to the tile's nearest INTERIOR edge, so the image border fades nothing -- and with S the sum of the weights of the tiles that cover
an output pixel, out = (sum_j W_j tile_j + (S >> 1)) // S: a linear crossfade over each overlap as wide as that overlap really is."""
import numpy as np

from . import buckets

MAX_OVERLAP = 256
MAX_BATCH = 16
MAX_AXIS_TILES = 32                       # fie_tile_blend_rgb_u8's bound on nx and ny
AUTO_MAX = 1024                           # the largest side "auto" picks: 1024 x 1024 = buckets.MAX_PIXELS


def _is_int(v):
    return not isinstance(v, (bool, np.bool_)) and isinstance(v, (int, np.integer))


def parse(text):
    """The command lines' `--tiles` -> "auto" or a checked (tw, th); anything else is a ValueError."""
    s = str(text).strip().lower()
    if s == "auto":
        return s
    parts = s.split("x")
    if len(parts) != 2 or not all(p.strip().isdigit() for p in parts):
        raise ValueError(f"tiles {text!r}: 'auto' or 'WxH' with {buckets.RULE}")
    return buckets.check_size((int(parts[0]), int(parts[1])))


def check(tiles, tile_overlap=128, tile_batch=4):
    """The argument rules of `tiles`, `tile_overlap` and `tile_batch` -> (None | "auto" | (tw, th), overlap, batch)."""
    if not _is_int(tile_overlap) or not 0 <= tile_overlap <= MAX_OVERLAP:
        raise ValueError(f"tile_overlap={tile_overlap!r}: an integer in 0..{MAX_OVERLAP}")
    if not _is_int(tile_batch) or not 1 <= tile_batch <= MAX_BATCH:
        raise ValueError(f"tile_batch={tile_batch!r}: an integer in 1..{MAX_BATCH}")
    if tiles is None:
        return None, int(tile_overlap), int(tile_batch)
    if isinstance(tiles, str):
        try:
            tiles = parse(tiles)
        except ValueError as e:
            raise ValueError(f"tiles={tiles!r}: None, 'auto', (tw, th) or 'WxH': {e}") from None
    else:
        try:
            tiles = buckets.check_size(tiles)
        except ValueError as e:
            raise ValueError(f"tiles={tiles!r}: None, 'auto', (tw, th) or 'WxH': {e}") from None
    return tiles, int(tile_overlap), int(tile_batch)


def _ceil_div(a, b):
    return -(-a // b)


def _axis(S, t, o, what):
    """One axis: image side S, tile side t (None: "auto") and overlap o -> (t, positions)."""
    if t is None:
        if S < buckets.SIDE_MIN:
            raise ValueError(f"tiles='auto': the image's {what} {S} is below the smallest tile side {buckets.SIDE_MIN}")
        if S <= AUTO_MAX and S % buckets.SIDE_STEP == 0:
            return S, [0]
        n = max(2, _ceil_div(S - o, AUTO_MAX - o))
        t = max(buckets.SIDE_MIN, buckets.SIDE_STEP * _ceil_div(_ceil_div(S + (n - 1) * o, n), buckets.SIDE_STEP))
    else:
        if S < t:
            raise ValueError(f"tiles: the image's {what} {S} is below the tile's {t}")
        if S == t:
            return t, [0]
        n = max(2, _ceil_div(S - o, t - o))
    if n > MAX_AXIS_TILES:
        raise ValueError(f"tiles: {n} tiles of {t} along the image's {what} {S}: at most {MAX_AXIS_TILES}")
    return t, [(i * (S - t)) // (n - 1) for i in range(n)]


def plan(size, tiles, overlap=128):
    """(width, height) of the image, check()'s `tiles` ("auto" or (tw, th)) and overlap -> (tw, th, xs, ys)."""
    tiles, overlap, _ = check(tiles, overlap)
    if tiles is None:
        raise ValueError("tiles=None has no plan")
    W, H = (int(v) for v in size)
    tw, th = (None, None) if tiles == "auto" else tiles
    tw, xs = _axis(W, tw, overlap, "width")
    th, ys = _axis(H, th, overlap, "height")
    return tw, th, xs, ys


def boxes(tw, th, xs, ys):
    """The (l, t, r, b) box of every tile, in tile order (row-major)."""
    return [(x, y, x + tw, y + th) for y in ys for x in xs]


def chunks(n, k):
    """range(n) in order as ceil(n / k) consecutive lists whose lengths differ by at most one (the longer ones first): the device jobs of n
    tiles at no more than k per job -- at most two distinct job shapes."""
    if not _is_int(n) or not _is_int(k) or n < 1 or k < 1:
        raise ValueError(f"chunks({n!r}, {k!r}): two integers >= 1")
    m = _ceil_div(n, k)
    base, extra = divmod(n, m)
    out, i = [], 0
    for c in range(m):
        size = base + (1 if c < extra else 0)
        out.append(list(range(i, i + size)))
        i += size
    return out


def axis_weight(t, i, n):
    """int64 [t]: the weight of tile i of n along one axis over its own pixels u = 0 .. t - 1."""
    u = np.arange(t, dtype=np.int64)
    head = np.full(t, t, np.int64) if i == 0 else u + 1
    tail = np.full(t, t, np.int64) if i == n - 1 else t - u
    return np.minimum(head, tail)


def check_positions(pos, t, S, what="positions"):
    """The rules of fie_tile_blend_rgb_u8 for one axis: 1..32 integers that start at 0, increase strictly, leave no gap and end at S - t."""
    try:
        pos = list(pos)
    except TypeError:
        pos = [None]
    if not all(_is_int(p) for p in pos):
        raise ValueError(f"tile_blend: {what}={pos!r}: a list of integers")
    pos = [int(p) for p in pos]
    ok =1 <= len(pos) <= MAX_AXIS_TILES and t >= 1 and S >= 1 and pos[0] == 0 and pos[-1] == S - t and all(
        a < b <= a + t for a, b in zip(pos, pos[1:]))
    if not ok:
        raise ValueError(f"tile_blend: {what}={pos!r} with tiles of {t} over {S}: 1..{MAX_AXIS_TILES} positions from 0 to {S - t}, strictly "
                         f"increasing, each at most {t} after the one before")
    return pos


def blend_numpy(tiles, xs, ys, H, W):
    """The device blend restated (CPU checker; the product path is csrc/tile_blend.hip).  tiles: uint8 [ny * nx, th, tw, 3] in tile order ->
    uint8 [H, W, 3]."""
    tiles = np.asarray(tiles)
    if tiles.ndim != 4 or tiles.shape[3] != 3 or tiles.dtype != np.uint8:
        raise ValueError(f"blend_numpy: uint8 [n, th, tw, 3] tiles, got {tiles.shape} {tiles.dtype}")
    n, th, tw, _ = tiles.shape
    xs, ys = check_positions(xs, tw, W, "xs"), check_positions(ys, th, H, "ys")
    nx, ny = len(xs), len(ys)
    if n != nx * ny:
        raise ValueError(f"blend_numpy: {n} tiles for a {nx} x {ny} grid")
    num = np.zeros((H, W, 3), np.int64)
    den = np.zeros((H, W, 1), np.int64)
    for iy, y in enumerate(ys):
        wy = axis_weight(th, iy, ny)
        for ix, x in enumerate(xs):
            w = (wy[:, None] * axis_weight(tw, ix, nx)[None, :])[:, :, None]
            num[y:y + th, x:x + tw] += w * tiles[iy * nx + ix].astype(np.int64)
            den[y:y + th, x:x + tw] += w
    return ((num + (den >> 1)) // den).astype(np.uint8)
