"""Soft-mask oracle (test infrastructure): the ramp's definition word for word, and `masked_oracle.run_masked` with the
release schedule, composed from `oracle.nets`, `oracle.lcm.LCMOracle` and `oracle.pipeline` the way tests/masked_oracle.py is.  CPU fp32.

    1. V: the level map, mode-L u8 at the edit size; its support S = 255 (V > 0) stands where run_masked reads the mask;
    2. m_lat[y, x] = (S[8y, 8x] >= 128); lvl_lat = m_lat ? max(V[8y, 8x], 1) : 0;
    3. the edit runs K steps j = 0 .. K-1; after step j: lat = (lvl_lat K > 255 (K-1-j)) ? lat : (add_noise(z0, n_init, next t), or z0 after the last);
    4. output: run_masked's, over the support."""
import math

import numpy as np
import torch

import masked_oracle
from oracle import nets
from oracle.lcm import LCMOracle
from oracle.pipeline import encode_prompt, float_to_u8, pil_to_float


def ramp_literal(mask_l, r):
    """The definition by brute force: for every set pixel the smallest squared distance to ANY unset pixel of the image, python integers."""
    m = np.asarray(mask_l) >= 128
    h, w = m.shape
    out = np.zeros((h, w), np.uint8)
    uy, ux = np.nonzero(~m)
    for y, x in zip(*np.nonzero(m)):
        if uy.size == 0:                                  # a mask of all ones: no unset pixel within any distance
            out[y, x] = 255
            continue
        d2 = int(((uy - y) ** 2 + (ux - x) ** 2).min())
        out[y, x] = 255 if d2 >= r * r else min(255, math.isqrt(65025 * d2) // r)
    return out


def lat_levels(levels):
    """-> (support u8 [H, W], lvl_lat int64 [H/8, W/8]) of a level map at the edit size."""
    v = np.asarray(levels)
    s = (v > 0).astype(np.uint8) * 255
    m_lat = s[::8, ::8] >= 128
    return s, np.where(m_lat, np.maximum(v[::8, ::8], 1), 0).astype(np.int64)


@torch.no_grad()
def run_levels(sds, cfgs, image, control_image, ids, neg_ids, levels, mask_blur=0, paste_back=True, strength=0.8, num_inference_steps=4,
               guidance_scale=1.5, controlnet_conditioning_scale=0.5, generator=None, sched_cfg=None, trace=None):
    """masked_oracle.run_masked with a level map (levels: uint8 [H, W] at the image's size).  Returns uint8 HxWx3."""
    do_cfg = guidance_scale > 1.0
    pe, pooled = encode_prompt(sds, cfgs, *ids)
    if do_cfg:
        npe, npooled = encode_prompt(sds, cfgs, *neg_ids)
        pe, pooled = torch.cat([npe, pe]), torch.cat([npooled, pooled])
    x_img = pil_to_float(image, True)
    cond = pil_to_float(control_image, False)
    if do_cfg:
        cond = torch.cat([cond, cond])
    h, w = x_img.shape[-2:]
    support, lvl = lat_levels(levels)
    _, _, m_paste = masked_oracle.masks(support, mask_blur)
    lvl = torch.from_numpy(lvl)[None, None]                # [1, 1, h/8, w/8]

    sch = LCMOracle(**(sched_cfg or {}))
    sch.set_timesteps(num_inference_steps)
    timesteps, _ = sch.get_timesteps(num_inference_steps, strength)
    K = len(timesteps)

    vae_cfg = cfgs["vae"]
    mean, logvar = nets.vae_encode_moments(sds["vae"], vae_cfg, x_img)
    std = torch.exp(0.5 * logvar)
    z0 = (mean + std * torch.randn(mean.shape, generator=generator, dtype=torch.float32)) * vae_cfg["scaling_factor"]
    noise = torch.randn(z0.shape, generator=generator, dtype=torch.float32)
    lat = sch.add_noise(z0, noise, timesteps[0]) if K else z0

    tid = torch.tensor([[h, w, 0, 0, h, w]], dtype=torch.float32).repeat(pe.shape[0], 1)
    for j, t in enumerate(timesteps):
        x_in = torch.cat([lat, lat]) if do_cfg else lat
        down, mid = nets.controlnet_forward(sds["controlnet"], cfgs["controlnet"], x_in, t, pe, cond,
                                            controlnet_conditioning_scale, pooled, tid)
        eps = nets.unet_forward(sds["unet"], cfgs["unet"], x_in, t, pe, pooled, tid, down, mid)
        if do_cfg:
            eu, ec = eps.chunk(2)
            eps = eu + guidance_scale * (ec - eu)
        last = sch.step_index == sch.num_inference_steps - 1
        z = None if last else torch.randn(eps.shape, generator=generator, dtype=torch.float32)
        lat, _ = sch.step(eps, t, lat, z)
        proper = z0 if last else sch.add_noise(z0, noise, sch.timesteps[sch.step_index])
        lat = torch.where(lvl * K > 255 * (K - 1 - j), lat, proper)
    if trace is not None:
        trace.update(z0=z0, latents=lat)
    dec = nets.vae_decode(sds["vae"], vae_cfg, lat / vae_cfg["scaling_factor"])
    if not paste_back:
        return float_to_u8(dec)[0]
    return masked_oracle.composite(dec, np.asarray(image), m_paste)
