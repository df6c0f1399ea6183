"""Control weights, what the CPU and the GPU tests share: the plain-loop restatement of the weight pyramid, the maps of the op
tests, the hole and the weights of the one-evaluation test, the unchanged oracle with its ControlNet residuals weighed on the host, and the same
evaluation through the nets of a pipeline."""
import numpy as np
import torch

import emphasis_oracle as eo
from fie_amd import control

HOLE = (20, 100, 36, 128)                   # rows 20 .. 99, columns 36 .. 127 of the 128 x 128 edit: aligned to 8 px on no side but the right
LEVELS = [0, 0, 0, 1, 1, 1, 2, 2, 2, 2]     # the pyramid level of the ten residuals of SDXL / SSD-1B and the tiny stacks, the mid block's last
SIZES = [(8, 8), (24, 40), (128, 128), (320, 512)]      # (H, W): one position per level; odd latent sizes, so every level clips; the evaluation's; a bucket


def hole_map(h=128, w=128):
    e = np.zeros((h, w), np.uint8)
    e[HOLE[0]:HOLE[1], HOLE[2]:HOLE[3]] = 255
    return e


def maps(h, w, seed=0):
    """The inputs of the pyramid tests: a random binary map, a grey level map, all 0, all 255."""
    rng = np.random.default_rng(seed + h * 4096 + w)
    return {"binary": np.where(rng.random((h, w)) > 0.6, 255, 0).astype(np.uint8), "grey": rng.integers(0, 256, (h, w)).astype(np.uint8),
            "zeros": np.zeros((h, w), np.uint8), "full": np.full((h, w), 255, np.uint8)}


def pyramid_loop(e, levels=3):
    """pyramid_numpy as a plain Python loop over positions and pixels: [(E, cnt)] per level, lists of lists of ints."""
    h, w = e.shape
    rows = [[int(v) for v in r] for r in e]
    out, hl, wl = [], h // 8, w // 8
    for l in range(levels):
        s = 8 << l
        big_e, cnt = [], []
        for y in range(hl):
            big_e.append([])
            cnt.append([])
            for x in range(wl):
                ys, xs = range(y * s, min((y + 1) * s, h)), range(x * s, min((x + 1) * s, w))
                big_e[-1].append(sum(rows[yy][xx] for yy in ys for xx in xs))
                cnt[-1].append(len(ys) * len(xs))
        out.append((big_e, cnt))
        hl, wl = (hl + 1) // 2, (wl + 1) // 2
    return out


def weights_loop(pyr, a):
    """weights_numpy on pyramid_loop's lists, one position at a time."""
    out = []
    for big_e, cnt in pyr:
        for er, cr in zip(big_e, cnt):
            for ev, cv in zip(er, cr):
                out.append(np.float32(255 * cv * 256 - (256 - a) * ev) / np.float32(255 * cv * 256))
    return np.asarray(out, np.float32)


def eval_weights(in_mask):
    """The weights of the evaluation test: the hole on the 128 x 128 edit of eval_inputs (16 x 16 latents), three levels; f32 [336]."""
    e = hole_map()
    return control.weights_numpy(control.pyramid_numpy(e, control.level_dims(128, 128)), control.mask_a(in_mask))


def level_maps(w, lh=16, lw=16):
    """The weight vector of one image as a [1, 1, h_l, w_l] tensor per level."""
    out, off = [], 0
    for hl, wl in control.level_dims(lh * 8, lw * 8):
        out.append(torch.from_numpy(np.asarray(w[off:off + hl * wl], np.float32).reshape(1, 1, hl, wl)))
        off += hl * wl
    return out


def oracle_eval(sds32, cfgs, x, scales=None, w=None):
    """One ControlNet + UNet evaluation of the unchanged oracle on `x` (emphasis_oracle.eval_inputs) with the residuals of its ControlNet, taken at
    scale 1, weighed on the host: residual i times scales[i] (None: 0.5 each, the plain evaluation) times the weight of its latent position (w: None,
    or the f32 vector of one image -- both CFG rows are the one image).  scales of all 0: the UNet alone."""
    from oracle import nets
    scales = [0.5] * 10 if scales is None else list(scales)
    down, mid = nets.controlnet_forward(sds32["controlnet"], cfgs["controlnet"], x["lat"], x["t"], x["text"], x["cond"], 1.0, x["pooled"], x["tid"])
    res = down + [mid]
    assert len(res) == len(scales) == len(LEVELS)
    wm = level_maps(w, x["lh"], x["lw"]) if w is not None else None
    res = [r * float(s) * (wm[l] if wm is not None else 1.0) for r, s, l in zip(res, scales, LEVELS)]
    return nets.unet_forward(sds32["unet"], cfgs["unet"], x["lat"], x["t"], x["text"], x["pooled"], x["tid"], res[:-1], res[-1])


def hip_eval(pipe, ctx, x, scales=None, w=None):
    """The same evaluation through the nets of `pipe`, in the context's dtype.  scales None: the parent's path, add_residuals at 0.5; else
    add_residuals_weighted with them and `w` (None: the scalar path; f32 [1, P_tot] on the device: the map path).  -> eps as [2, 4, H, W]."""
    dev, dt, lh, lw = ctx.device, ctx.dtype, x["lh"], x["lw"]
    model_in = torch.zeros(2, lh, lw, 8, dtype=dt, device=dev)
    model_in[..., :4] = x["lat"].permute(0, 2, 3, 1).to(dev, dt)
    cond8 = torch.zeros(2, lh * 8, lw * 8, 8, dtype=dt, device=dev)
    cond8[..., :3] = x["cond"].permute(0, 2, 3, 1).to(dev, dt)
    text_d = x["text"].reshape(2 * eo.T, x["xd"]).to(dev, dt)
    pipe.unet.begin_image(x["pooled"].to(dev, dt), x["tid"].to(dev))
    pipe.controlnet.begin_image(x["pooled"].to(dev, dt), x["tid"].to(dev))
    cemb = pipe.controlnet.cond_embedding(cond8)
    t_dev = torch.full((2, 1), float(x["t"]), device=dev)
    tb_u, tb_c = pipe.unet.time_rowbias(t_dev), pipe.controlnet.time_rowbias(t_dev)
    skips, m = pipe.unet.encode(pipe.unet.conv_in(ctx, model_in), tb_u, text_d, eo.T)
    c_skips, c_mid = pipe.controlnet.encode_cond(model_in, cemb, tb_c, text_d, eo.T)
    if scales is None:
        skips2, m2 = pipe.controlnet.add_residuals(c_skips, c_mid, 0.5, skips, m)
    else:
        skips2, m2 = pipe.controlnet.add_residuals_weighted(c_skips, c_mid, scales, skips, m, w=w, rows_per_image=2)
    eps = pipe.unet.decode(m2, skips2, tb_u, text_d, eo.T)
    return eps[..., :4].permute(0, 3, 1, 2)
