"""LPIPS (SqueezeNet) of an edit on the device (kernels: csrc/lpips.hip, csrc/f32.hip).

The number is torchmetrics' `LearnedPerceptualImagePatchSimilarity(net_type="squeeze")` with `normalize=False` on two 512 x 512 images in [-1, 1], as
the reference calls it (reference src/metrics.py:179-181, 241-269):
  input    u8 -> x = u8 / 255 -> y = x * 2 - 1 -> z = (y - SHIFT) / SCALE per channel, all fp32: 768 possible values, `input_lut()`;
  tower    torchvision `squeezenet1_1().features[0..12]`: conv 3 -> 64 k3 stride 2 without padding + ReLU, MaxPool(3, 2, ceil_mode=True) at indices
           2, 5, 8, Fire(in, squeeze, expand1x1, expand3x3) = cat(relu(conv1x1(s)), relu(conv3x3 pad 1 (s))) with s = relu(conv1x1(x)) elsewhere (FIRE);
  taps     the outputs after indices TAPS, TAP_CHANNELS wide;
  per tap  n = f / sqrt(1e-8 + sum_c f^2) per pixel, d = sum_c w_c (n_a - n_b)^2 with w the tap's 1x1 `lin` weight, value = mean of d over the map;
  LPIPS    the seven values added left to right in float64 (`total`).
Everything runs in fp32 whatever the context's dtype: one code path.  `load(dir, ctx)` reads a directory in either of two forms; there is no scorer
without one (a made-up number stays forbidden).  The host-side arithmetic of this module is device-free and tested on the CPU."""
import glob
import os

import torch

SHIFT = (-0.030, -0.088, -0.188)
SCALE = (0.458, 0.448, 0.450)
EPS = 1e-8                                   # inside the root: torchmetrics' form
DIR_ENV = "FIE_LPIPS_DIR"
POOLS = (2, 5, 8)                            # indices of `features` that are MaxPool2d(3, 2, ceil_mode=True)
FIRE = {3: (64, 16, 64, 64), 4: (128, 16, 64, 64), 6: (128, 32, 128, 128), 7: (256, 32, 128, 128), 9: (256, 48, 192, 192), 10: (384, 48, 192, 192),
        11: (384, 64, 256, 256), 12: (512, 64, 256, 256)}        # index -> (in, squeeze, expand1x1, expand3x3)
TAPS = (1, 4, 7, 9, 10, 11, 12)
TAP_CHANNELS = (64, 128, 256, 384, 384, 512, 512)
MIN_SIDE = 32
PASS_IMAGES = 16                             # images that go through the tower together


def resolve_dir(lpips_dir=None):
    """The weight directory: the argument, else FIE_LPIPS_DIR, else <FIE_WEIGHTS_DIR>/lpips when that exists, else None."""
    if lpips_dir:
        return str(lpips_dir)
    if os.environ.get(DIR_ENV):
        return os.environ[DIR_ENV]
    root = os.environ.get("FIE_WEIGHTS_DIR")
    if root and os.path.isdir(os.path.join(root, "lpips")):
        return os.path.join(root, "lpips")
    return None


def input_lut():
    """f32 [3, 256]: byte -> the tower's input per channel, by the definition's own fp32 operations in their order."""
    x = torch.arange(256, dtype=torch.float32) / 255.0
    y = x * 2 - 1
    return ((y[None] - torch.tensor(SHIFT, dtype=torch.float32)[:, None]) / torch.tensor(SCALE, dtype=torch.float32)[:, None]).contiguous()


def pooled(n):
    """Output edge of MaxPool2d(3, 2, ceil_mode=True) for an input edge n >= 3: ceil((n - 3) / 2) + 1 (the last window always starts inside)."""
    return (n - 2) // 2 + 1


def feature_sizes(h, w):
    """[(H, W)] of the seven taps for an h x w image."""
    if min(h, w) < MIN_SIDE:
        raise ValueError(f"lpips: a {w} x {h} image is below the {MIN_SIDE} x {MIN_SIDE} minimum")
    s = [((h - 3) // 2 + 1, (w - 3) // 2 + 1)]
    for _ in POOLS:
        s.append((pooled(s[-1][0]), pooled(s[-1][1])))
    return [s[0], s[1], s[2], s[3], s[3], s[3], s[3]]


def expected_shapes():
    """{key: shape} of every tensor the scorer needs, under torchvision's / the lpips package's names."""
    out = {"features.0.weight": (64, 3, 3, 3), "features.0.bias": (64,)}
    for i, (cin, s, e1, e3) in FIRE.items():
        out.update({f"features.{i}.squeeze.weight": (s, cin, 1, 1), f"features.{i}.squeeze.bias": (s,),
                    f"features.{i}.expand1x1.weight": (e1, s, 1, 1), f"features.{i}.expand1x1.bias": (e1,),
                    f"features.{i}.expand3x3.weight": (e3, s, 3, 3), f"features.{i}.expand3x3.bias": (e3,)})
    for k, c in enumerate(TAP_CHANNELS):
        out[f"lin{k}.model.1.weight"] = (1, c, 1, 1)
    return out


def check_tensors(sd):
    """{key: f32 host tensor} of expected_shapes() from a state dict that may hold more (classifier keys are ignored).  A missing key is a KeyError
    naming it, a wrong shape a ValueError naming key and shapes."""
    out = {}
    for key, shape in expected_shapes().items():
        if key not in sd:
            raise KeyError(f"lpips: the weights have no tensor {key!r}")
        if tuple(sd[key].shape) != shape:
            raise ValueError(f"lpips: tensor {key!r} has shape {tuple(sd[key].shape)}, expected {shape}")
        out[key] = sd[key].detach().to(torch.float32).contiguous()
    return out


def read_dir(lpips_dir):
    """The state dict of a weight directory: `model.safetensors` with all keys, or the two original files `squeezenet1_1*.pth` (torchvision's
    backbone) and `squeeze.pth` (the lpips package's linear layers)."""
    st = os.path.join(lpips_dir, "model.safetensors")
    if os.path.exists(st):
        from safetensors.torch import load_file
        return check_tensors(load_file(st))
    backbone = sorted(glob.glob(os.path.join(lpips_dir, "squeezenet1_1*.pth")))
    lin = os.path.join(lpips_dir, "squeeze.pth")
    if not backbone or not os.path.exists(lin):
        raise FileNotFoundError(f"lpips: {lpips_dir} holds neither model.safetensors nor squeezenet1_1*.pth + squeeze.pth")
    sd = dict(torch.load(backbone[0], weights_only=True, map_location="cpu"))
    sd.update(torch.load(lin, weights_only=True, map_location="cpu"))
    return check_tensors(sd)


def total(values):
    """The seven layer values -> LPIPS: added left to right in float64."""
    s = 0.0
    for v in values:
        s += float(v)
    return s


class LpipsScorer:
    """The tower and the `lin` weights on one context, as fp32 device tensors in the layouts the ops take.  Every method queues work on torch's current
    stream and returns device tensors; nothing here synchronises."""

    def __init__(self, ctx, tensors):
        self.ctx = ctx
        t = check_tensors(tensors)
        dev = lambda x: x.to(ctx.device, torch.float32).contiguous()
        self.lut = dev(input_lut())
        self.stem_w = dev(t["features.0.weight"].permute(2, 3, 1, 0).reshape(27, 64))             # [(ky, kx, ci), co]
        self.stem_b = dev(t["features.0.bias"])
        self.fire = {}
        for i, (cin, s, e1, e3) in FIRE.items():
            p = f"features.{i}."
            self.fire[i] = dict(sq_w=dev(t[p + "squeeze.weight"].reshape(s, cin)), sq_b=dev(t[p + "squeeze.bias"]),
                                e1_w=dev(t[p + "expand1x1.weight"].reshape(e1, s)), e1_b=dev(t[p + "expand1x1.bias"]),
                                e3_w=dev(t[p + "expand3x3.weight"].permute(0, 2, 3, 1).reshape(e3, 9 * s)), e3_b=dev(t[p + "expand3x3.bias"]))
        self.lin = [dev(t[f"lin{k}.model.1.weight"].reshape(-1)) for k in range(len(TAPS))]

    def _fire(self, i, x):
        """x f32 [m, H, W, in] -> [m, H, W, e1 + e3]: three launches, the two expand branches write the two channel halves of one tensor."""
        from . import hip
        ctx, f = self.ctx, self.fire[i]
        cin, s, e1, e3 = FIRE[i]
        m, h, w, _ = x.shape
        sq = ctx.gemm_f32(x.view(m * h * w, cin), f["sq_w"], s, bias=f["sq_b"], act=hip.ACT_RELU)
        out = ctx._alloc((m, h, w, e1 + e3), torch.float32)
        ctx.gemm_f32(sq, f["e1_w"], e1, out=out.view(m * h * w, e1 + e3)[:, :e1], bias=f["e1_b"], act=hip.ACT_RELU)
        ctx.conv3x3_f32(sq.view(m, h, w, s), f["e3_w"], e3, out[..., e1:], bias=f["e3_b"], act=hip.ACT_RELU)
        return out

    def taps(self, images, masks=None):
        """images u8 [m, h, w, 3] (masks: None or u8 [m, h, w], non-zero = black) -> a generator of the seven taps f32 [m, H, W, C], each
        computed when asked for: a consumer that drops a tap before asking for the next keeps at most two alive."""
        ctx = self.ctx
        x = ctx.lpips_stem(images, self.lut, self.stem_w, self.stem_b, mask=masks)
        yield x
        for i in range(2, 13):
            x = ctx.maxpool3s2(x) if i in POOLS else self._fire(i, x)
            if i in TAPS:
                yield x

    def _pass(self, a, b, chunk, res):
        """One pass of the tower over the 2 k images of k items (image index, mask or None), then the layer op per tap and run of items."""
        ctx = self.ctx
        k = len(chunk)
        ims = torch.stack([a[i] for i, _ in chunk] + [b[i] for i, _ in chunk])
        mk = None
        if any(m is not None for _, m in chunk):
            zero = torch.zeros(a[0].shape[:2], device=ctx.device, dtype=torch.uint8)
            half = [zero if m is None else m for _, m in chunk]
            mk = torch.stack(half + half)
        # runs of items whose rows are consecutive in one column block of `res`
        runs, r0 = [], 0
        for r in range(1, k + 1):
            if r == k or chunk[r][0] != chunk[r - 1][0] + 1 or (chunk[r][1] is None) != (chunk[r - 1][1] is None):
                runs.append((r0, r))
                r0 = r
        for t, f in enumerate(self.taps(ims, mk)):
            f = f.view(2 * k, -1, f.shape[3])
            for r0, r1 in runs:
                i0, col = chunk[r0][0], t if chunk[r0][1] is None else 7 + t
                ctx.lpips_layer(f[r0:r1], f[k + r0:k + r1], self.lin[t], out=res[i0:i0 + (r1 - r0), col])
            del f

    def scores(self, a, b, masks=None, out=None):
        """a, b: two lists of n u8 [h, w, 3] device tensors of ONE size, sides >= 32.  Returns f64 [n, 7] on the device: the seven layer values of
        every pair (`total` of a row is its LPIPS).  With `masks` (a list of n: None, or a u8 [h, w] tensor whose non-zero pixels count as black in
        both images) the result is [n, 14], the background variant second (NaN where no mask was given).  All images go through the tower in
        passes of at most PASS_IMAGES; a pair's bits depend neither on n nor on its position."""
        n = len(a)
        if n == 0 or len(b) != n or (masks is not None and len(masks) != n):
            raise ValueError("lpips: a, b and masks must be non-empty lists of one length")
        h, w = a[0].shape[:2]
        if min(h, w) < MIN_SIDE:
            raise ValueError(f"lpips: a {w} x {h} image is below the {MIN_SIDE} x {MIN_SIDE} minimum")
        for what, ims in (("a", a), ("b", b)):
            for i, im in enumerate(ims):
                if tuple(im.shape) != (h, w, 3) or im.dtype != torch.uint8:
                    raise ValueError(f"lpips: image {what}[{i}] is {tuple(im.shape)} {im.dtype}, expected u8 {(h, w, 3)}")
        for i, m in enumerate(masks or ()):
            if m is not None and (tuple(m.shape) != (h, w) or m.dtype != torch.uint8):
                raise ValueError(f"lpips: mask {i} is {tuple(m.shape)} {m.dtype}, expected u8 {(h, w)}")
        cols = 7 if masks is None else 14
        if out is None:
            out = torch.empty((n, cols), device=self.ctx.device, dtype=torch.float64)
        elif tuple(out.shape) != (n, cols) or out.dtype != torch.float64:
            raise ValueError(f"lpips: out must be a f64 {(n, cols)} tensor, got {tuple(out.shape)} {out.dtype}")
        items = [(i, None) for i in range(n)]
        if masks is not None:
            items += [(i, m) for i, m in enumerate(masks) if m is not None]
            if len(items) < 2 * n:
                out[:, 7:] = float("nan")
        per = PASS_IMAGES // 2
        for j in range(0, len(items), per):
            self._pass(a, b, items[j:j + per], out)
        return out


def load(lpips_dir, ctx):
    """A weight directory (read_dir's two forms) -> LpipsScorer on `ctx`."""
    sd = read_dir(lpips_dir)
    with torch.cuda.device(ctx.device):
        ctx.sync_stream()
        return LpipsScorer(ctx, sd)
