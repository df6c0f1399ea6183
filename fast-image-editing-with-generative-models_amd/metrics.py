"""Host side of the device metrics (the device side is csrc/metrics.hip): decoding of a result row of
`fie_metrics_pairs_u8` into SSIM / PSNR / MSE, and the preparation of the binary mask of the background variants.  Device-free, so all of it
runs (and is tested) on the CPU.

Metrics are taken at TARGET = 512 x 512 (LANCZOS, as the reference's evaluation does).  A row is four 8-byte fields
{uint64 sse, float64 ssim_sum, uint64 bg_sse, float64 bg_ssim_sum}: the integer sum of squared u8 differences and the sum of the SSIM map,
for the pair and for its background pair (both images zeroed inside the edited region -- PIE-Bench's `img * (1 - mask)` convention)."""
import math

import numpy as np
from PIL import Image

from . import mask as hmask

TARGET = (512, 512)
KEYS = ("ssim", "psnr", "mse")
BG_KEYS = ("bg_ssim", "bg_psnr", "bg_mse")


def from_sums(sse, ssim_sum, h, w, prefix=""):
    """(exact integer SSE, sum of the SSIM map) of an h x w RGB pair -> {ssim, psnr, mse} in float64: MSE = sse / (255^2 * 3hw) on [0, 1]
    pixels, PSNR = 10 log10(1 / MSE) (inf at 0), SSIM = ssim_sum / (3 (h - 10) (w - 10)): the mean of the map over the positions whose 11x11
    window lies inside the image, as oracle/metrics.py crops it."""
    mse = int(sse) / (65025.0 * 3 * int(h) * int(w))
    return {prefix + "ssim": float(ssim_sum) / (3 * (int(h) - 10) * (int(w) - 10)), prefix + "psnr": float("inf") if sse == 0 else 10.0 * math.log10(1.0 / mse),
            prefix + "mse": mse}


def rows_to_dicts(rows, h, w, bg=False):
    """int64 [n, 4] result rows (a host numpy array or tensor) -> one dict per pair; `bg` (a bool, or one per pair) adds the bg_* keys."""
    r = np.ascontiguousarray(np.asarray(rows), dtype=np.int64).reshape(-1, 4)
    sums = r.view(np.float64)
    bgs = [bool(bg)] * len(r) if isinstance(bg, (bool, np.bool_)) else [bool(v) for v in bg]
    out = []
    for i in range(len(r)):
        d = from_sums(int(r[i, 0]) & 0xFFFFFFFFFFFFFFFF, sums[i, 1], h, w)
        if bgs[i]:
            d.update(from_sums(int(r[i, 2]) & 0xFFFFFFFFFFFFFFFF, sums[i, 3], h, w, "bg_"))
        out.append(d)
    return out


def binary_mask(mask, size=None):
    """Whatever mask the caller has (a PIL image or a uint8 / bool [H, W] array, white = edited; `size` = (width, height) it must have) ->
    uint8 [512, 512] of 0 / 1: mode L, LANCZOS-resized to TARGET when it has another size, then L >= 128 (the binarisation rule of
    DESIGN.md section 8).  A PIE-Bench run-length mask is 512 x 512 already: binary_mask(mask.rle_decode(entry["mask"]))."""
    a = hmask.to_l_array(mask, size)
    if (a.shape[1], a.shape[0]) != TARGET:
        a = np.asarray(Image.fromarray(a, "L").resize(TARGET, Image.LANCZOS))
    return (a >= 128).astype(np.uint8)


def binary_mask_device(ctx, mask_l):
    """binary_mask() for a mode-L u8 [H, W] mask already on the device: the LANCZOS resize runs in fie_resize_l_u8 (bit-exact with Pillow)."""
    if (mask_l.shape[1], mask_l.shape[0]) != TARGET:
        mask_l = ctx.resize_lanczos(mask_l.contiguous(), TARGET[1], TARGET[0])
    return (mask_l >= 128).view(mask_l.dtype)
