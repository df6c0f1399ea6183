"""CPU oracle of the LPIPS tests (tests/test_lpips_cpu.py, tests/test_lpips_gpu.py): SqueezeNet 1.1's `features` and the LPIPS head restated in plain
torch (`F.conv2d`, `F.max_pool2d(ceil_mode=True)`) from the public architecture, as DESIGN.md section 19 defines the number.  Everything can be
evaluated in float64 and float32: the GPU tests' bounds are 4 x the oracle's own fp32 error against its float64 self.

Weights are seeded, not trained: conv N(0, 2 / fan_in), biases 0.1 N, `lin` weights uniform in [0, 2 / C], all rounded to fp16 (exact in every
precision).  With them 44-53 % of every tap is positive on random bytes: no layer is dead.  `write_dir` writes a directory in either form
fie_amd.lpips.load reads.  Results are cached per (case, precision, variant): a reference is computed once and shared."""
import math
import os

import numpy as np
import torch
import torch.nn.functional as F

import dino_oracle as do

SHIFT, SCALE = (-0.030, -0.088, -0.188), (0.458, 0.448, 0.450)
FIRE = {3: (64, 16, 64, 64), 4: (128, 16, 64, 64), 6: (128, 32, 128, 128), 7: (256, 32, 128, 128), 9: (256, 48, 192, 192), 10: (384, 48, 192, 192),
        11: (384, 64, 256, 256), 12: (512, 64, 256, 256)}
POOLS = (2, 5, 8)
TAPS = (1, 4, 7, 9, 10, 11, 12)
CHANNELS = (64, 128, 256, 384, 384, 512, 512)
SEED = 19
DTYPES = {"f64": torch.float64, "f32": torch.float32}
PAIRS = ("ab", "ac", "ad")
CASES = {"small": (67, 45), "full": (512, 512)}          # (size of dino_oracle.images, rows kept): 45 x 67 and 512 x 512


def weights():
    """The seeded state dict under torchvision's names plus lin0 .. lin6 (fp32 tensors holding fp16-exact values), and some classifier keys a loader
    must ignore."""
    if "w" not in _cache:
        g = torch.Generator().manual_seed(SEED)
        sd = {}

        def conv(name, co, ci, k):
            sd[name + ".weight"] = (torch.randn((co, ci, k, k), generator=g) * math.sqrt(2.0 / (ci * k * k))).half().float()
            sd[name + ".bias"] = (0.1 * torch.randn((co,), generator=g)).half().float()
        conv("features.0", 64, 3, 3)
        for i, (cin, s, e1, e3) in FIRE.items():
            conv(f"features.{i}.squeeze", s, cin, 1)
            conv(f"features.{i}.expand1x1", e1, s, 1)
            conv(f"features.{i}.expand3x3", e3, s, 3)
        for k, c in enumerate(CHANNELS):
            sd[f"lin{k}.model.1.weight"] = (torch.rand((1, c, 1, 1), generator=g) * 2.0 / c).half().float()
        _cache["w"] = sd
    return _cache["w"]


def write_dir(path, form):
    """form "safetensors": model.safetensors with every key; "pth": the two original files, the backbone with classifier keys beside the features."""
    os.makedirs(str(path), exist_ok=True)
    sd = weights()
    if form == "safetensors":
        from safetensors.torch import save_file
        save_file({k: v.contiguous() for k, v in sd.items()}, os.path.join(str(path), "model.safetensors"))
    else:
        backbone = {k: v for k, v in sd.items() if k.startswith("features.")}
        backbone["classifier.1.weight"], backbone["classifier.1.bias"] = torch.zeros(10, 512, 1, 1), torch.zeros(10)
        torch.save(backbone, os.path.join(str(path), "squeezenet1_1-b8a52dc0.pth"))
        torch.save({k: v for k, v in sd.items() if k.startswith("lin")}, os.path.join(str(path), "squeeze.pth"))
    return str(path)


def images(case):
    size, rows = CASES[case]
    return {n: np.ascontiguousarray(v[:rows]) for n, v in do.images(size).items()}


def lut(dtype=torch.float32):
    """[3, 256]: byte -> the tower's input, the definition's operations in `dtype`."""
    x = torch.arange(256, dtype=dtype) / 255.0
    y = x * 2 - 1
    return (y[None] - torch.tensor(SHIFT, dtype=dtype)[:, None]) / torch.tensor(SCALE, dtype=dtype)[:, None]


def scaled(arr, dtype, mask=None, scaling=True):
    """u8 [h, w, 3] (mask: None or [h, w], non-zero = the pixel counts as black) -> [1, 3, h, w] tower input in `dtype`."""
    a = np.array(arr)
    if mask is not None:
        a[np.asarray(mask) != 0] = 0
    x = torch.from_numpy(a).permute(2, 0, 1)[None].to(dtype) / 255.0
    y = x * 2 - 1
    if not scaling:
        return y
    return (y - torch.tensor(SHIFT, dtype=dtype)[None, :, None, None]) / torch.tensor(SCALE, dtype=dtype)[None, :, None, None]


def tower(z, dtype, ceil=True):
    """[n, 3, h, w] -> the seven taps [n, C, H, W]."""
    sd = {k: v.to(dtype) for k, v in weights().items()}
    x = F.relu(F.conv2d(z, sd["features.0.weight"], sd["features.0.bias"], stride=2))
    taps = [x]
    for i in range(2, 13):
        if i in POOLS:
            x = F.max_pool2d(x, 3, 2, ceil_mode=ceil)
        else:
            p = f"features.{i}."
            s = F.relu(F.conv2d(x, sd[p + "squeeze.weight"], sd[p + "squeeze.bias"]))
            x = torch.cat([F.relu(F.conv2d(s, sd[p + "expand1x1.weight"], sd[p + "expand1x1.bias"])),
                           F.relu(F.conv2d(s, sd[p + "expand3x3.weight"], sd[p + "expand3x3.bias"], padding=1))], 1)
        if i in TAPS:
            taps.append(x)
    return taps


def layer_value(fa, fb, w):
    """[C, H, W] features of the two sides and the [C] lin weight -> the tap's value (a 0-d tensor in the features' dtype)."""
    na = fa / torch.sqrt(1e-8 + (fa * fa).sum(0, keepdim=True))
    nb = fb / torch.sqrt(1e-8 + (fb * fb).sum(0, keepdim=True))
    return (w.to(fa.dtype)[:, None, None] * (na - nb) ** 2).sum(0).mean()


def layers(ta, tb):
    """The seven layer values of one pair from its two tap lists ([1, C, H, W] each)."""
    sd = weights()
    return [layer_value(a[0], b[0], sd[f"lin{k}.model.1.weight"].reshape(-1)).item() for k, (a, b) in enumerate(zip(ta, tb))]


def total(values):
    s = 0.0
    for v in values:
        s += float(v)
    return s


_cache = {}


def taps_of(case, name, prec, mask=None, ceil=True, scaling=True, key=None):
    """The seven taps [1, C, H, W] of image `name` of `case` in DTYPES[prec]; `key` names the mask for the cache."""
    ck = ("taps", case, name, prec, key if mask is not None else None, ceil, scaling)
    if ck not in _cache:
        with torch.no_grad():
            _cache[ck] = tower(scaled(images(case)[name], DTYPES[prec], mask, scaling), DTYPES[prec], ceil)
    return _cache[ck]


def layers_of(case, pair, prec, mask=None, ceil=True, scaling=True, key=None):
    """The seven layer values of pair "ab" / "ac" / "ad" / "aa" of `case` at that precision."""
    ck = ("layers", case, pair, prec, key if mask is not None else None, ceil, scaling)
    if ck not in _cache:
        _cache[ck] = layers(taps_of(case, pair[0], prec, mask, ceil, scaling, key), taps_of(case, pair[1], prec, mask, ceil, scaling, key))
    return _cache[ck]


def score_of(case, pair, prec, **kw):
    return total(layers_of(case, pair, prec, **kw))


def score_error(case, **kw):
    """The oracle's own error: the largest |s_32 - s_64| / s_64 over the case's three pairs."""
    return max(abs(score_of(case, p, "f32", **kw) - score_of(case, p, "f64", **kw)) / score_of(case, p, "f64", **kw) for p in PAIRS)


def rel_err(a, b):
    """The project's parity measure: max |a - b| / max |b|."""
    return do.rel_err(a, b)


def tap_errors(case):
    """Per tap, the oracle's own fp32 relative max-abs error against float64, the largest over the four images."""
    return [max(rel_err(taps_of(case, n, "f32")[k], taps_of(case, n, "f64")[k]) for n in do.NAMES) for k in range(len(TAPS))]


def full_mask():
    """A 512 x 512 u8 mask (255 = edited) that does not coincide with image c's inverted rectangle: a band across its lower right part."""
    m = np.zeros((512, 512), np.uint8)
    m[200:420, 150:330] = 255
    return m
