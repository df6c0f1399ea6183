"""Prompt emphasis, what the CPU and the GPU tests share: the inputs and weights of the one-evaluation test, the unchanged
oracle with `oracle.nets._lin` wrapped so that every `*attn2.to_v` output row is multiplied by its weight, and the caches of a net's blocks."""
import contextlib

import numpy as np
import torch

from fie_amd import emphasis

T = 77


def rel_err(a, b):
    a, b = a.float().cpu(), b.float().cpu()
    return ((a - b).abs().max() / b.abs().max().clamp_min(1e-9)).item()


def eval_weights():
    """The weights of the evaluation test, [2, 77], rows [negative, positive]."""
    w = np.ones((2, T), np.float32)
    w[1, 2:5] = 4.0
    w[1, 7] = 0.0
    w[0, 3] = 0.5
    return w


def eval_inputs(cfgs):
    """tests/test_pipeline_gpu.py::test_unet_controlnet_eval_parity's inputs: seed 5, 16 x 16 latents, CFG batch 2."""
    g = torch.Generator().manual_seed(5)
    lh = lw = 16
    lat = torch.randn(2, 4, lh, lw, generator=g).half().float()
    cond = (torch.rand(2, 3, lh * 8, lw * 8, generator=g) > 0.9).float()
    xd = cfgs["unet"]["cross_attention_dim"]
    text = torch.randn(2, T, xd, generator=g).half().float()
    pdim = cfgs["unet"]["projection_class_embeddings_input_dim"] - 6 * cfgs["unet"]["addition_time_embed_dim"]
    pooled = torch.randn(2, pdim, generator=g).half().float()
    tid = torch.tensor([[128., 128., 0, 0, 128., 128.]]).repeat(2, 1)
    return dict(lat=lat, cond=cond, text=text, pooled=pooled, tid=tid, t=499, lh=lh, lw=lw, xd=xd)


@contextlib.contextmanager
def weighted_to_v(weights):
    """Inside: `oracle.nets._lin` multiplies the output rows of every `*attn2.to_v` by `weights` ([B, 77]).  Nothing under oracle/ changes."""
    from oracle import nets
    plain = nets._lin
    w = torch.from_numpy(np.asarray(weights, np.float32))
    seen = []

    def lin(sd, p, x):
        y = plain(sd, p, x)
        if p.endswith("attn2.to_v"):
            assert y.shape[:2] == w.shape, (p, tuple(y.shape))
            seen.append(p)
            y = y * w[:, :, None]
        return y
    nets._lin = lin
    try:
        yield seen
    finally:
        nets._lin = plain


def oracle_eval(sds32, cfgs, x, weights=None):
    """One ControlNet + UNet evaluation of the oracle on `x` (eval_inputs); `weights`: None, or the emphasis weights [2, 77]."""
    from oracle import nets
    with weighted_to_v(weights) if weights is not None else contextlib.nullcontext([]) as seen:
        down, mid = nets.controlnet_forward(sds32["controlnet"], cfgs["controlnet"], x["lat"], x["t"], x["text"], x["cond"], 0.5, x["pooled"], x["tid"])
        ref = nets.unet_forward(sds32["unet"], cfgs["unet"], x["lat"], x["t"], x["text"], x["pooled"], x["tid"], down, mid)
    assert weights is None or len(seen) > 2
    return ref


def hip_eval(pipe, ctx, x, emph=None):
    """The same evaluation through the nets of `pipe`, in the context's dtype; `emph`: None, or f32 [2 * 77] on the device.  -> eps as [2, 4, H, W]."""
    dev, dt, lh, lw = ctx.device, ctx.dtype, x["lh"], x["lw"]
    model_in = torch.zeros(2, lh, lw, 8, dtype=dt, device=dev)
    model_in[..., :4] = x["lat"].permute(0, 2, 3, 1).to(dev, dt)
    cond8 = torch.zeros(2, lh * 8, lw * 8, 8, dtype=dt, device=dev)
    cond8[..., :3] = x["cond"].permute(0, 2, 3, 1).to(dev, dt)
    text_d = x["text"].reshape(2 * T, x["xd"]).to(dev, dt)
    pipe.unet.begin_image(x["pooled"].to(dev, dt), x["tid"].to(dev), emph=emph)
    pipe.controlnet.begin_image(x["pooled"].to(dev, dt), x["tid"].to(dev), emph=emph)
    cemb = pipe.controlnet.cond_embedding(cond8)
    t_dev = torch.full((2, 1), float(x["t"]), device=dev)
    tb_u, tb_c = pipe.unet.time_rowbias(t_dev), pipe.controlnet.time_rowbias(t_dev)
    skips, m = pipe.unet.encode(pipe.unet.conv_in(ctx, model_in), tb_u, text_d, T)
    c_skips, c_mid = pipe.controlnet.encode_cond(model_in, cemb, tb_c, text_d, T)
    skips2, m2 = pipe.controlnet.add_residuals(c_skips, c_mid, 0.5, skips, m)
    eps = pipe.unet.decode(m2, skips2, tb_u, text_d, T)
    return eps[..., :4].permute(0, 3, 1, 2)


def blocks(net):
    return [b for t in net.transformers() for b in t.blocks]


def caches(pipe):
    """The text K | V cache of every transformer block of the UNet and the ControlNet, as numpy copies: [(c, [rows, 2 c])]."""
    out = []
    for net in (pipe.unet, pipe.controlnet):
        for b in blocks(net):
            assert b.kv_cache is not None, "a block's cache was not filled"
            out.append((b.c, b.kv_cache.detach().cpu().numpy().copy()))
    return out


def expected_caches(plain, w):
    """The restatement applied to the plain caches: K columns as they are, V columns through kv_emphasis_numpy with the rows' weights `w`."""
    w = np.asarray(w, np.float32).reshape(-1)
    return [(c, emphasis.kv_emphasis_numpy(kv, w, emphasis.v_flags([c]))) for c, kv in plain]


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    view = {2: np.uint16, 4: np.uint32}[a.dtype.itemsize]
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(view), b.view(view))
