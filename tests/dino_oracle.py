"""CPU oracle of the DINO structure distance tests (tests/test_dino_cpu.py, tests/test_dino_gpu.py): a seeded `transformers.ViTModel` without pooler,
written into a directory the product loads (`save_pretrained`), the keys of block `layer` captured by a forward hook on its key projection, the
preprocess as `F.interpolate(..., antialias=True)` and the distance formed as DESIGN.md section 12 defines it.  Everything can be evaluated in float64,
float32 and float16 on the CPU: the tests' bounds are 4 x the oracle's own error at the precision of the device context against its float64 self.

Weights are RE-DRAWN, not transformers' initialisation (std 0.02 would let every image produce nearly the same keys): matrices N(0, 4 / fan_in),
LayerNorm gains 1 + 0.2 N, biases 0.1 N, class token and position table 0.5 N, all rounded to fp16 so that the fp16 context loads exactly the oracle's
weights.  Results are cached per (config, precision): a reference is computed once and shared."""
import copy
import math

import numpy as np
import torch
import torch.nn.functional as F

MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)

CONFIGS = {
    # 2 layers, hidden 128 (2 heads of 64), 64 x 64 / patch 8: 65 tokens
    "tiny": dict(hidden_size=128, num_hidden_layers=2, num_attention_heads=2, intermediate_size=256, image_size=64, patch_size=8),
    # the shape of facebook/dino-vitb8: 785 tokens
    "b8": dict(hidden_size=768, num_hidden_layers=12, num_attention_heads=12, intermediate_size=3072, image_size=224, patch_size=8),
}
LAYER = {"tiny": 1, "b8": 11}
SOURCE = {"tiny": 203, "b8": 512}             # edge of the square test images
SEED = {"tiny": 5, "b8": 9}
DTYPES = {"f64": torch.float64, "f32": torch.float32, "f16": torch.float16}
NAMES = ("a", "b", "c", "d")


def images(size):
    """The four deterministic u8 [size, size, 3] test images: a smooth sinusoid / gradient, a + N(0, 12) noise, a with one rectangle inverted,
    uniform random bytes."""
    rng = np.random.default_rng(size)
    yy, xx = np.mgrid[0:size, 0:size].astype(np.float64) / size
    a = np.stack([128 + 90 * np.sin(2 * math.pi * (1.5 * xx + 0.5 * yy)), 40 + 170 * xx * (1 - 0.5 * yy),
                  128 + 60 * np.cos(2 * math.pi * (0.7 * xx - 2.2 * yy) + 1.0) + 40 * yy], axis=2)
    b = a + rng.normal(0, 12, a.shape)
    c = a.copy()
    y0, y1, x0, x1 = size // 5, size // 5 + size // 3, size // 3, size // 3 + size // 2
    c[y0:y1, x0:x1] = 255 - c[y0:y1, x0:x1]
    u8 = lambda v: np.clip(np.rint(v), 0, 255).astype(np.uint8)
    return {"a": u8(a), "b": u8(b), "c": u8(c), "d": rng.integers(0, 256, a.shape, dtype=np.uint8)}


def build_model(kind):
    """The seeded fp32 ViTModel (no pooler) of CONFIGS[kind] with re-drawn, fp16-rounded weights; layer_norm_eps 1e-12 as the hub file's."""
    from transformers import ViTConfig, ViTModel
    model = ViTModel(ViTConfig(**CONFIGS[kind], layer_norm_eps=1e-12, hidden_act="gelu"), add_pooling_layer=False).eval().float()
    g = torch.Generator().manual_seed(SEED[kind])
    with torch.no_grad():
        for name, p in model.named_parameters():
            n = lambda: torch.randn(p.shape, generator=g)
            if "cls_token" in name or "position_embeddings" in name:
                w = 0.5 * n()
            elif "layernorm" in name:
                w = 1.0 + 0.2 * n() if name.endswith("weight") else 0.1 * n()
            elif name.endswith("bias"):
                w = 0.1 * n()
            else:
                w = n() * 2.0 / math.sqrt(math.prod(p.shape[1:]))
            p.copy_(w.half().float())
    return model


def save(model, path):
    """A directory fie_amd.dino.load reads: save_pretrained (config.json + model.safetensors)."""
    model.save_pretrained(str(path))
    return str(path)


def block(model, i):
    """Block i of a ViTModel and its (query, key) projections, whatever this transformers version calls them."""
    if hasattr(model, "layers"):
        blk = model.layers[i]
    else:
        blk = model.encoder.layer[i]
    att = blk.attention
    if hasattr(att, "k_proj"):
        return blk, att.q_proj, att.k_proj
    return blk, att.attention.query, att.attention.key


def preprocess(arr, size, dtype=torch.float32):
    """u8 [h, w, 3] -> [3, size', size'']: /255, `Resize(size, antialias=True)` on the float tensor, (x - mean) / std -- all in `dtype`.  float16: the
    definition's fp32 preprocess, rounded once at the end (what the fp16 context's tower is fed)."""
    if dtype == torch.float16:
        return preprocess(arr, size, torch.float32).half()
    x = torch.from_numpy(np.ascontiguousarray(arr)).permute(2, 0, 1).to(dtype) / 255.0
    h, w = x.shape[1:]
    oh, ow = (int(size * h / w), size) if w <= h else (size, int(size * w / h))
    x = F.interpolate(x[None], size=(oh, ow), mode="bilinear", antialias=True, align_corners=False)[0]
    mean, std = torch.tensor(MEAN, dtype=dtype)[:, None, None], torch.tensor(STD, dtype=dtype)[:, None, None]
    return (x - mean) / std


def patch_rows(pixel_values, ps=8):
    """[3, S, S] -> [P, 3 ps ps] by `unfold`: the patch rows in the K order of the patch-embedding weight viewed as [C, 3 ps ps]."""
    return F.unfold(pixel_values[None].float(), kernel_size=ps, stride=ps)[0].T.contiguous()


def capture(model, pixel_values, layer, which="key"):
    """[n, 3, S, S] -> the output of the key (or query) projection of block `layer`, [n, T, C], by a forward hook."""
    got = []
    _, q, k = block(model, layer)
    handle = (k if which == "key" else q).register_forward_hook(lambda _m, _i, out: got.append(out.detach()))
    try:
        with torch.no_grad():
            model(pixel_values=pixel_values)
    finally:
        handle.remove()
    return got[0]


def selfsim(k):
    """[T, C] -> S = (K K^T) / max(|k_i| |k_j|, 1e-8): the PRODUCT of the norms is clamped."""
    norm = k.norm(dim=1, keepdim=True)
    return (k @ k.T) / torch.clamp(norm @ norm.T, min=1e-8)


def distance(k_src, k_edit):
    """Mean over all T^2 entries of (S_edited - S_source)^2, in the dtype of the keys."""
    return ((selfsim(k_edit) - selfsim(k_src)) ** 2).mean().item()


_cache = {}


def model_of(kind):
    if ("model", kind) not in _cache:
        _cache[("model", kind)] = build_model(kind)
    return _cache[("model", kind)]


def keys_of(kind, prec, layer=None, which="key"):
    """{image name: keys [T, C] in DTYPES[prec]} of the four test images of CONFIGS[kind], everything (resize, tower) evaluated in that precision."""
    layer = LAYER[kind] if layer is None else layer
    key = ("keys", kind, prec, layer, which)
    if key not in _cache:
        dt = DTYPES[prec]
        model = copy.deepcopy(model_of(kind)).to(dt)
        ims = images(SOURCE[kind])
        px = torch.stack([preprocess(ims[n], CONFIGS[kind]["image_size"], dt) for n in NAMES])
        k = capture(model, px, layer, which)
        _cache[key] = {n: k[i] for i, n in enumerate(NAMES)}
    return _cache[key]


def distances_of(kind, prec, layer=None, which="key"):
    """{"ab": d(a, b), "ac": ..., "ad": ..., "aa": ...} at that precision."""
    k = keys_of(kind, prec, layer, which)
    return {"a" + n: distance(k["a"], k[n]) for n in ("b", "c", "d", "a")}


def rel_err(a, b):
    """The project's parity measure: max |a - b| / max |b|."""
    a, b = torch.as_tensor(a).double().cpu(), torch.as_tensor(b).double().cpu()
    return ((a - b).abs().max() / b.abs().max().clamp_min(1e-300)).item()


def distance_errors(kind, prec):
    """e_p: the largest relative error |d_p - d_64| / d_64 of the oracle over the non-identical pairs."""
    d64, dp = distances_of(kind, "f64"), distances_of(kind, prec)
    return max(abs(dp[p] - d64[p]) / d64[p] for p in ("ab", "ac", "ad"))


def key_errors(kind, prec):
    """The oracle's own relative max-abs error of K at that precision against float64, the largest over the four images."""
    k64, kp = keys_of(kind, "f64"), keys_of(kind, prec)
    return max(rel_err(kp[n], k64[n]) for n in NAMES)
