"""Coefficient tables of Pillow's 8-bit LANCZOS / BICUBIC resample, restated (host side of csrc/resize.hip).

Follows Pillow `src/libImaging/Resample.c`: `precompute_coeffs` (support 3 x max(scale, 1), bounds by truncating
`center -/+ support + 0.5`, weights normalised to sum 1) and `normalize_coeffs_8bpc` (22-bit fixed point, round half away from
zero).  The reference reaches it through `image.resize((1024, 1024), Image.LANCZOS)` (`src/pipeline.py:251`).  Pure Python / libm
doubles, as Pillow's C: the tables -- and therefore the device result -- are bit-exact with Pillow (tests/test_cabi_cpu.py).
`filter="bicubic"` is Pillow's `bicubic_filter` (a = -0.5, support 2): what `CLIPImageProcessor` resizes with; the
kernels are the same, taps and bounds come from the tables.  `nearest_indices` restates the index table of Pillow's NEAREST resize.
`aa_coefficients` restates the fp32 tables of torch's antialiased bilinear interpolation (host side of csrc/dino.hip)."""
import math

import numpy as np

PRECISION_BITS = 32 - 8 - 2
LANCZOS_SUPPORT = 3.0


def _sinc(x):
    if x == 0.0:
        return 1.0
    x *= math.pi
    return math.sin(x) / x


def _lanczos(x):
    return _sinc(x) * _sinc(x / 3) if -3.0 <= x < 3.0 else 0.0


def _bicubic(x):
    a = -0.5
    if x < 0.0:
        x = -x
    if x < 1.0:
        return ((a + 2.0) * x - (a + 3.0)) * x * x + 1
    if x < 2.0:
        return (((x - 5) * x + 8) * x - 4) * a
    return 0.0


FILTERS = {"lanczos": (_lanczos, LANCZOS_SUPPORT), "bicubic": (_bicubic, 2.0)}


def coefficients(in_size, out_size, filter="lanczos"):
    """-> (kk int32 [out_size, ksize], bounds int32 [out_size, 2] = (first input index, tap count), ksize)."""
    if filter not in FILTERS:
        raise ValueError(f"resample filter {filter!r}: one of {sorted(FILTERS)}")
    kernel, base_support = FILTERS[filter]
    scale = float(np.float32(in_size) - np.float32(0)) / out_size          # Pillow's box is float32
    filterscale = max(scale, 1.0)
    support = base_support * filterscale
    ksize = int(math.ceil(support)) * 2 + 1
    kk = np.zeros((out_size, ksize), dtype=np.int32)
    bounds = np.zeros((out_size, 2), dtype=np.int32)
    ss = 1.0 / filterscale
    for xx in range(out_size):
        center = 0.0 + (xx + 0.5) * scale
        xmin = max(int(center - support + 0.5), 0)                         # int(): truncation, as the C cast
        xmax = min(int(center + support + 0.5), in_size) - xmin
        w = [kernel((x + xmin - center + 0.5) * ss) for x in range(xmax)]
        ww = 0.0
        for v in w:
            ww += v
        for x, v in enumerate(w):
            k = v / ww if ww != 0.0 else v
            kk[xx, x] = int(-0.5 + k * (1 << PRECISION_BITS)) if k < 0 else int(0.5 + k * (1 << PRECISION_BITS))
        bounds[xx] = (xmin, xmax)
    return kk, bounds, ksize


def nearest_indices(in_size, out_size):
    """int32 [out_size]: the input index Pillow's `resize(..., Image.NEAREST)` reads for every output position (`ImagingScaleAffine`: the
    coordinate starts at scale / 2 and is ADVANCED by additions of scale, in doubles, then truncated)."""
    a = float(in_size) / out_size
    xo = a * 0.5
    out = np.empty(out_size, dtype=np.int32)
    for x in range(out_size):
        out[x] = min(int(xo), in_size - 1)
        xo += a
    return out


def resample_numpy(rgb, out_h, out_w, filter="lanczos"):
    """The two passes in numpy with the tables above (CPU checker of the tables; the product path is the HIP kernel)."""
    a = np.asarray(rgb, dtype=np.uint8)
    h, w, _ = a.shape

    def one_pass(img, axis_len, out_len):
        kk, bounds, _ = coefficients(axis_len, out_len, filter)
        out = np.empty((img.shape[0], out_len, 3), dtype=np.uint8)
        for o in range(out_len):
            x0, n = bounds[o]
            acc = (img[:, x0:x0 + n, :].astype(np.int64) * kk[o, :n, None].astype(np.int64)).sum(axis=1) + (1 << (PRECISION_BITS - 1))
            out[:, o, :] = np.clip(acc >> PRECISION_BITS, 0, 255).astype(np.uint8)
        return out

    if w != out_w:
        a = one_pass(a, w, out_w)
    if h != out_h:
        a = one_pass(a.transpose(1, 0, 2), h, out_h).transpose(1, 0, 2)
    return np.ascontiguousarray(a)


def aa_coefficients(in_size, out_size):
    """Tables of torch's `interpolate(mode="bilinear", antialias=True, align_corners=False)` on a float tensor, one axis (ATen
    UpSampleKernel.cpp: `_compute_indices_min_size_weights_aa` with the triangle filter, what torchvision's `Resize(antialias=True)` runs):
    scale = in / out in fp32, support = max(scale, 1), centre = scale (i + 0.5), first index = int(centre - support + 0.5) clipped at 0, count up to
    int(centre + support + 0.5) clipped at the input size, weight = max(1 - |(x - centre + 0.5) / max(scale, 1)|, 0), normalised per output pixel.
    The weights are fp32 and fp32 divisions, as ATen's (its mixed float / double expressions are restated as written there).
    -> (weights float32 [out_size, ksize], bounds int32 [out_size, 2] = (first input index, tap count), ksize).  Up-scaling (support 1, at most
    three taps) and the identity size (taps {1, 0}: exact) come from the same formula."""
    f32 = np.float32
    scale = f32(in_size) / f32(out_size)
    support = scale if scale >= 1.0 else f32(1.0)
    invscale = f32(1.0) / scale if scale >= 1.0 else f32(1.0)
    ksize = int(math.ceil(float(support))) * 2 + 1
    ww = np.zeros((out_size, ksize), dtype=np.float32)
    bounds = np.zeros((out_size, 2), dtype=np.int32)
    for i in range(out_size):
        center = f32(float(scale) * (i + 0.5))
        xmin = max(int(float(center) - float(support) + 0.5), 0)
        xsize = min(max(min(int(float(center) + float(support) + 0.5), in_size) - xmin, 0), ksize)
        total = f32(0.0)
        for j in range(xsize):
            x = abs(f32((float(f32(j + xmin) - center) + 0.5) * float(invscale)))
            w = f32(1.0) - x if x < 1.0 else f32(0.0)
            ww[i, j] = w
            total = f32(total + w)
        if total != 0.0:
            ww[i, :xsize] = ww[i, :xsize] / total
        bounds[i] = (xmin, xsize)
    return ww, bounds, ksize


def aa_resample_numpy(x, out_h, out_w):
    """float32 [h, w, c] -> float32 [out_h, out_w, c] with the tables above: the horizontal pass first, each output the fp32 sum of its taps in
    order (CPU checker of the tables; the product path is csrc/dino.hip)."""
    a = np.asarray(x, dtype=np.float32)

    def one_pass(img, out_len):                    # along axis 1
        ww, bounds, _ = aa_coefficients(img.shape[1], out_len)
        out = np.zeros((img.shape[0], out_len, img.shape[2]), dtype=np.float32)
        for o in range(out_len):
            x0, n = bounds[o]
            for j in range(n):
                t = img[:, x0 + j, :] * ww[o, j]
                out[:, o, :] = t if j == 0 else out[:, o, :] + t
        return out

    a = one_pass(a, out_w)
    a = one_pass(a.transpose(1, 0, 2), out_h).transpose(1, 0, 2)
    return np.ascontiguousarray(a)
