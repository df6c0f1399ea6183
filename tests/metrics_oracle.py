"""Metrics oracle helpers (test infrastructure) for tests/test_metrics_cpu.py and tests/test_metrics_gpu.py.

    ssim64        the float64 restatement of SSIM that tests/test_oracle_cpu.py holds (separable float64 correlation with scipy.ndimage on the
                  un-padded image, the map kept only where the 11x11 window lies inside the image, Wang et al. 2004 eq. 13), restated here;
    ssim32        oracle.metrics.ssim(size=None): the reference definition in fp32 torch;
    sse           the exact integer sum of squared u8 differences (numpy int64);
    zeroed        the background pair: both images with the edited region (mask != 0) set to 0, then the plain metric on them;
    pair_set      the input pairs every device check runs on; d0(pairs) = max |ssim32 - ssim64| over them, the yardstick of the SSIM tolerance."""
import os
import sys

import numpy as np
from PIL import Image
from scipy.ndimage import correlate1d, gaussian_filter

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from oracle import metrics as ometrics  # noqa: E402


def ssim64(u8a, u8b):
    x, y = np.asarray(u8a).astype(np.float64) / 255.0, np.asarray(u8b).astype(np.float64) / 255.0
    d = np.arange(-5, 6, dtype=np.float64)
    g = np.exp(-(d / 1.5) ** 2 / 2)
    g /= g.sum()
    blur = lambda t: correlate1d(correlate1d(t, g, axis=0, mode="constant"), g, axis=1, mode="constant")[5:-5, 5:-5]
    c1, c2 = 0.01 ** 2, 0.03 ** 2
    vals = []
    for ch in range(3):
        mx, my = blur(x[..., ch]), blur(y[..., ch])
        sxx, syy, sxy = blur(x[..., ch] ** 2) - mx * mx, blur(y[..., ch] ** 2) - my * my, blur(x[..., ch] * y[..., ch]) - mx * my
        vals.append(((2 * mx * my + c1) * (2 * sxy + c2)) / ((mx * mx + my * my + c1) * (sxx + syy + c2)))
    return float(np.mean(vals))


def ssim32(u8a, u8b):
    return ometrics.ssim(Image.fromarray(np.asarray(u8a)), Image.fromarray(np.asarray(u8b)), size=None)


def sse(u8a, u8b):
    return int(((np.asarray(u8a).astype(np.int64) - np.asarray(u8b).astype(np.int64)) ** 2).sum())


def zeroed(u8a, u8b, mask):
    keep = (np.asarray(mask) == 0)[..., None].astype(np.uint8)
    return np.asarray(u8a) * keep, np.asarray(u8b) * keep


def textured(i, h=512, w=512):
    """Seeded picture of the synthetic PIE-Bench generator (bench.synth_item_image, what tools/make_synthetic_piebench.py writes), cut or
    resized to h x w."""
    from bench import synth_item_image
    im = synth_item_image(i)
    if (w, h) != im.size:
        im = im.resize((w, h), Image.LANCZOS)
    return np.asarray(im).copy()


def variants(a, seed):
    """(name, a, b) pairs of one image: its noisy, 3-pixel-shifted and blurred copies and itself."""
    rng = np.random.default_rng(seed)
    noisy = (a.astype(np.int64) + rng.integers(-20, 21, a.shape)).clip(0, 255).astype(np.uint8)
    shifted = np.roll(a, 3, axis=1)
    blurred = gaussian_filter(a.astype(np.float64), sigma=(2.0, 2.0, 0)).round().clip(0, 255).astype(np.uint8)
    return [("noisy", a, noisy), ("shifted", a, shifted), ("blurred", a, blurred), ("identical", a, a.copy())]


def pair_set():
    """Every input pair of the device checks: [(name, a u8 [H, W, 3], b)].  512x512 (the product size), 11x11 (the minimum) and 203x517 (no
    multiple of the kernel's tile): textured images against their noisy / shifted / blurred copies and themselves, black against white, two
    independent uniform-random images."""
    out = []
    for h, w in ((512, 512), (11, 11), (203, 517)):
        rng = np.random.default_rng(h * 1000 + w)
        a = textured(7 if h == 512 else 11, h, w)
        out += [(f"{n}_{h}x{w}", x, y) for n, x, y in variants(a, h + w)]
        out.append((f"black_white_{h}x{w}", np.zeros((h, w, 3), np.uint8), np.full((h, w, 3), 255, np.uint8)))
        out.append((f"random_{h}x{w}", rng.integers(0, 256, (h, w, 3), dtype=np.uint8), rng.integers(0, 256, (h, w, 3), dtype=np.uint8)))
    return out


def d0(pairs):
    """max |fp32 oracle - float64 restatement| over `pairs`: what the reference definition itself leaves undetermined in fp32."""
    return max(abs(ssim32(a, b) - ssim64(a, b)) for _, a, b in pairs)


def blob_mask(h, w, seed):
    """A seeded blob (a filled ellipse with a ragged edge) as uint8 0 / 255."""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    cy, cx = rng.uniform(0.3, 0.7) * h, rng.uniform(0.3, 0.7) * w
    ry, rx = rng.uniform(0.15, 0.3) * h, rng.uniform(0.15, 0.3) * w
    ang = np.arctan2(yy - cy, xx - cx)
    rag = 1.0 + 0.15 * np.sin(5 * ang + rng.uniform(0, 6)) + 0.08 * np.sin(11 * ang + rng.uniform(0, 6))
    return ((((yy - cy) / ry) ** 2 + ((xx - cx) / rx) ** 2) < rag ** 2).astype(np.uint8) * 255
