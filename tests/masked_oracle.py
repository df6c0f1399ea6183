"""Masked-edit oracle (test infrastructure): `oracle.pipeline.run` plus the mask semantics of DESIGN.md section 8, composed from
`oracle.nets`, `oracle.lcm.LCMOracle` and `oracle.pipeline.pil_to_float` / `float_to_u8`.  CPU fp32.

    1. mask: mode-L u8 at the edit size, binarised m_px = L >= 128;
    2. m_lat[y, x] = m_px[8y, 8x];
    3. after every LCM step: lat = m_lat ? lat : (add_noise(z0, n_init, next t), or z0 after the last step);
    4. output: the decoded bytes, or with paste_back the source where m == 0, the decoded byte where m == 1, rint(m d + (1 - m) src)
       between (m = m_px, or its Gaussian feather with mask_blur > 0)."""
import numpy as np
import torch

from oracle import nets
from oracle.lcm import LCMOracle
from oracle.pipeline import encode_prompt, float_to_u8, pil_to_float


def masks(mask_l, mask_blur=0):
    """-> (m_px float32 0/1 [H, W], m_lat bool [H/8, W/8], paste-back weights float32 [H, W])."""
    import fie_amd  # noqa: F401
    from fie_amd import mask as hmask
    m_px = (np.asarray(mask_l) >= 128).astype(np.float32)
    return m_px, m_px[::8, ::8] > 0, hmask.feather_numpy(m_px, mask_blur)


def composite(dec, src_u8, m):
    """dec: decoded NCHW fp32 [1, 3, H, W]; src_u8 [H, W, 3]; m float32 [H, W] -> u8 [H, W, 3]."""
    d_f = (np.clip(dec[0].permute(1, 2, 0).float().numpy() * np.float32(0.5) + np.float32(0.5), 0, 1) * np.float32(255)).astype(np.float32)
    s = np.asarray(src_u8).astype(np.float32)
    mm = m[..., None].astype(np.float32)
    mid = np.rint(mm * d_f + (np.float32(1) - mm) * s)
    out = np.where(mm <= 0, s, np.where(mm >= 1, np.rint(d_f), mid))
    return out.astype(np.uint8)


@torch.no_grad()
def run_masked(sds, cfgs, image, control_image, ids, neg_ids, mask_l, mask_blur=0, paste_back=True, strength=0.8, num_inference_steps=4,
               guidance_scale=1.5, controlnet_conditioning_scale=0.5, generator=None, sched_cfg=None, trace=None):
    """oracle.pipeline.run with a mask (mask_l: uint8 [H, W] at the image's size, white = edit).  Returns uint8 HxWx3."""
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
    m_px, m_lat, m_paste = masks(mask_l, mask_blur)
    keep = torch.from_numpy(m_lat)[None, None]             # [1, 1, h/8, w/8]: True = edit

    sch = LCMOracle(**(sched_cfg or {}))
    sch.set_timesteps(num_inference_steps)
    timesteps, _ = sch.get_timesteps(num_inference_steps, strength)

    vae_cfg = cfgs["vae"]
    mean, logvar = nets.vae_encode_moments(sds["vae"], vae_cfg, x_img)
    std = torch.exp(0.5 * logvar)
    z0 = (mean + std * torch.randn(mean.shape, generator=generator, dtype=torch.float32)) * vae_cfg["scaling_factor"]
    noise = torch.randn(z0.shape, generator=generator, dtype=torch.float32)
    lat = sch.add_noise(z0, noise, timesteps[0]) if timesteps else z0

    tid = torch.tensor([[h, w, 0, 0, h, w]], dtype=torch.float32).repeat(pe.shape[0], 1)
    for t in timesteps:
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
        lat = torch.where(keep, lat, proper)
    if trace is not None:
        trace.update(z0=z0, latents=lat)
    dec = nets.vae_decode(sds["vae"], vae_cfg, lat / vae_cfg["scaling_factor"])
    if not paste_back:
        return float_to_u8(dec)[0]
    return composite(dec, np.asarray(image), m_paste)
