"""DINO structure distance of an edit on the device (kernels: csrc/dino.hip).

The number is the reference's `DinoDistanceMetric` (reference src/metrics.py:24-147) on a source and an edited image: the MSE between the cosine
self-similarity matrices of the keys of block `layer` (11) of DINO ViT-B/8,
  image  -> float / 255 -> `Resize(R, antialias=True)` on the float tensor (torch's antialiased bilinear interpolation, fp32; R = the model's
            image_size) -> (x - mean) / std with the ImageNet constants;
  keys   -> `ViTModel` without pooler: patch conv WITH bias, class token + position table, no pre-LayerNorm, pre-LN blocks with q/k/v biases and the
            exact (erf) GELU; K = the key projection (bias included) of block `layer`, [T, C];
  S      =  K K^T / max(|k_i| |k_j|, 1e-8);  distance = mean over T x T of (S_edited - S_source)^2.
`load(dir, ctx)` reads a transformers `ViTModel` directory (facebook/dino-vitb8 is one); there is no scorer without one (a made-up number stays
forbidden).  Both images must resize to image_size x image_size, i.e. be square: any other shape needs interpolated position tables, and the
reference itself fails on such a pair.  The host-side arithmetic of this module is device-free and tested on the CPU."""
import json
import os

import torch

IMAGENET_MEAN = (0.485, 0.456, 0.406)
IMAGENET_STD = (0.229, 0.224, 0.225)
DIR_ENV = "FIE_DINO_DIR"
DEFAULT_LAYER = 11


def resolve_dir(dino_dir=None):
    """The ViTModel directory: the argument, else FIE_DINO_DIR, else <FIE_WEIGHTS_DIR>/dino when that exists, else None."""
    if dino_dir:
        return str(dino_dir)
    if os.environ.get(DIR_ENV):
        return os.environ[DIR_ENV]
    root = os.environ.get("FIE_WEIGHTS_DIR")
    if root and os.path.isdir(os.path.join(root, "dino")):
        return os.path.join(root, "dino")
    return None


def resized_size(h, w, short):
    """(height, width) after `Resize(short)`: the shorter edge becomes `short`, the other `int(short * long / short_edge)`."""
    if w <= h:
        return int(short * h / w), short
    return short, int(short * w / h)


def supported_size(h, w):
    """True when an h x w image resizes to image_size x image_size: square inputs only."""
    return h == w and h > 0


# safetensors names of one block: the file's (what `save_pretrained` and the hub checkpoint write) and the module names of transformers 5.x
_FILE = dict(q="attention.attention.query", k="attention.attention.key", v="attention.attention.value", o="attention.output.dense",
             fc1="intermediate.dense", fc2="output.dense", ln1="layernorm_before", ln2="layernorm_after")
_MODULE = dict(q="attention.q_proj", k="attention.k_proj", v="attention.v_proj", o="attention.o_proj", fc1="mlp.fc1", fc2="mlp.fc2",
               ln1="layernorm_before", ln2="layernorm_after")


def tower_tensors(sd, cfg):
    """The host tensors DinoVit needs, under fixed names, from a `ViTModel` state dict in either naming (optionally prefixed `vit.`): `patch.weight /
    .bias`, `cls`, `pos`, and per block i < layer `i.{q,k,v,o,fc1,fc2,ln1,ln2}.{weight,bias}`; for block `layer` only `ln1` and `k`.  Raises a
    KeyError that names the first missing file key."""
    pre = "vit." if any(k.startswith("vit.") for k in sd) else ""
    if f"{pre}encoder.layer.0.layernorm_before.weight" in sd:
        block, names = lambda i: f"{pre}encoder.layer.{i}.", _FILE
    else:
        block, names = lambda i: f"{pre}layers.{i}.", _MODULE

    def get(key):
        if key not in sd:
            raise KeyError(f"dino: the checkpoint has no tensor {key!r} (a transformers ViTModel state dict is needed)")
        return sd[key]

    out = {"patch.weight": get(pre + "embeddings.patch_embeddings.projection.weight"), "patch.bias": get(pre + "embeddings.patch_embeddings.projection.bias"),
           "cls": get(pre + "embeddings.cls_token").reshape(-1), "pos": get(pre + "embeddings.position_embeddings").reshape(-1, cfg["hidden"])}
    for i in range(cfg["layer"] + 1):
        for short in (("ln1", "k") if i == cfg["layer"] else tuple(names)):
            for part in ("weight", "bias"):
                out[f"{i}.{short}.{part}"] = get(f"{block(i)}{names[short]}.{part}")
    return out


class DinoVit:
    """`ViTModel` up to the key projection of block cfg["layer"]: the patch convolution (with bias) is a GEMM over the patch rows fie_dino_patches_u8_*
    wrote; class token and position table are added by fie_vit_embed_*; blocks 0 .. layer - 1 run in full (fused q/k/v GEMM, non-causal attention,
    exact GELU), block `layer` only its layernorm_before and a K-only GEMM; the final layernorm is never needed.  No torch kernel in the walk.  Runs in
    the fp16 and in the exact-fp32 context."""

    def __init__(self, ctx, cfg, sd):
        from . import hip
        from .nn import Linear, Norm
        self.ctx, self.cfg = ctx, cfg
        t = tower_tensors(sd, cfg)
        dev = lambda x: x.to(ctx.device, ctx.dtype).contiguous()
        self.patch = Linear(ctx, None, None, w=t["patch.weight"], b=t["patch.bias"])           # [C, 3, ps, ps] -> [C, 3 ps ps]
        self.cls, self.pos = dev(t["cls"]), dev(t["pos"])
        if self.pos.shape != (cfg["tokens"], cfg["hidden"]):
            raise ValueError(f"dino_vit: position table {tuple(self.pos.shape)} for {cfg['tokens']} tokens x {cfg['hidden']}")
        self.layers = []
        for i in range(cfg["layer"]):
            w = torch.cat([t[f"{i}.{n}.weight"] for n in "qkv"], 0)
            b = torch.cat([t[f"{i}.{n}.bias"] for n in "qkv"], 0)
            self.layers.append(dict(ln1=Norm(ctx, t, f"{i}.ln1"), qkv=Linear(ctx, None, None, w=w, b=b), out=Linear(ctx, t, f"{i}.o"),
                                    ln2=Norm(ctx, t, f"{i}.ln2"), fc1=Linear(ctx, t, f"{i}.fc1"), fc2=Linear(ctx, t, f"{i}.fc2")))
        last = cfg["layer"]
        self.last_ln, self.last_k = Norm(ctx, t, f"{last}.ln1"), Linear(ctx, t, f"{last}.k")
        self.act = hip.ACT_GELU

    def keys(self, patches, n):
        """patches: [n * P, 3 ps ps] (ctx.dino_patches).  Returns the keys of block `layer`, [n * T, C]."""
        ctx, cfg = self.ctx, self.cfg
        c, heads, t = cfg["hidden"], cfg["heads"], cfg["tokens"]
        x = ctx.vit_embed(self.patch(ctx, patches), self.cls, self.pos, n)
        for L in self.layers:
            y = ctx.layernorm(x, L["ln1"].g, L["ln1"].b, cfg["eps"])
            qkv = L["qkv"](ctx, y)
            a = ctx.attention(qkv[:, :c], qkv[:, c:2 * c], qkv[:, 2 * c:], heads, c // heads, t, t, n, causal=False)
            x = L["out"](ctx, a, residual=x)
            y = ctx.layernorm(x, L["ln2"].g, L["ln2"].b, cfg["eps"])
            x = L["fc2"](ctx, L["fc1"](ctx, y, act=self.act), residual=x)
        return self.last_k(ctx, ctx.layernorm(x, self.last_ln.g, self.last_ln.b, cfg["eps"]))


class DinoScorer:
    """The tower of one ViTModel on one context, plus the preprocess and the scorer op.  Every method queues work on torch's current stream and
    returns device tensors; nothing here synchronises."""

    def __init__(self, ctx, vit, mean=IMAGENET_MEAN, std=IMAGENET_STD):
        self.ctx, self.vit, self.mean, self.std = ctx, vit, tuple(mean), tuple(std)

    def check_size(self, h, w):
        if not supported_size(h, w):
            r = self.vit.cfg["image_size"]
            rh, rw = resized_size(h, w, r) if h > 0 and w > 0 else (0, 0)
            raise ValueError(f"dino_distance: a {w} x {h} image resizes to {rw} x {rh}, not to the tower's {r} x {r}: only square images are supported")

    def _group(self, images, what):
        h, w = images[0].shape[:2]
        self.check_size(h, w)
        ims = []
        for i, im in enumerate(images):
            if tuple(im.shape) != (h, w, 3) or im.dtype != torch.uint8:
                raise ValueError(f"dino_distance: {what} image {i} is {tuple(im.shape)} {im.dtype}, expected u8 {(h, w, 3)}")
            ims.append(im.contiguous())
        return ims[0][None] if len(ims) == 1 else torch.stack(ims)

    def patches(self, sources, editeds):
        """The patch rows of all 2 n images, sources first: [2 n P, 3 ps ps]."""
        cfg = self.vit.cfg
        r, ps, n = cfg["image_size"], cfg["patch_size"], len(sources)
        p = cfg["tokens"] - 1
        out = torch.empty((2 * n * p, 3 * ps * ps), device=self.ctx.device, dtype=self.ctx.dtype)
        for half, (ims, what) in enumerate(((sources, "source"), (editeds, "edited"))):
            self.ctx.dino_patches(self._group(ims, what), r, r, ps, self.mean, self.std, out=out[half * n * p:(half + 1) * n * p])
        return out

    def keys(self, sources, editeds):
        """[2 n T, C]: the keys of block `layer` of all sources, then of all editeds -- one batched pass of the tower."""
        return self.vit.keys(self.patches(sources, editeds), 2 * len(sources))

    def distances(self, sources, editeds, out=None):
        """sources, editeds: two lists of n u8 [h, w, 3] device tensors, each list of ONE square size (the two sizes may differ).  Returns f64 [n] on
        the device: one batched pass of the tower over all 2 n images, then the scorer op."""
        if len(sources) != len(editeds) or not sources:
            raise ValueError("dino_distance: sources and editeds must be non-empty lists of one length")
        n, t = len(sources), self.vit.cfg["tokens"]
        k = self.keys(sources, editeds)
        return self.ctx.selfsim_mse(k[:n * t], k[n * t:], n, out=out)


def load(dino_dir, ctx, layer=DEFAULT_LAYER):
    """A transformers `ViTModel` directory -> DinoScorer on `ctx`: config.json and model.safetensors.  Uses safetensors only."""
    from safetensors.torch import load_file
    from . import config as hconfig
    missing = [f for f in ("config.json", "model.safetensors") if not os.path.exists(os.path.join(dino_dir, f))]
    if missing:
        raise FileNotFoundError(f"dino: {dino_dir} lacks {missing} (a transformers ViTModel directory is needed)")
    with open(os.path.join(dino_dir, "config.json"), encoding="utf-8") as f:
        cfg = hconfig.dino_vit_cfg(json.load(f), layer=layer)
    sd = load_file(os.path.join(dino_dir, "model.safetensors"))
    with torch.cuda.device(ctx.device):
        ctx.sync_stream()
        return DinoScorer(ctx, DinoVit(ctx, cfg, sd))
