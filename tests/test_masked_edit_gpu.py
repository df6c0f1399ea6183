"""Mask-restricted edits on the device: the new kernels against closed forms (masked LCM step, mask prep,
composite), a masked edit against the masked oracle, and the product surfaces (graph replay, batches, the C-ABI edit, run_batch
--use_mask, FastEditor.edit at full size)."""
import json
import pprint

import numpy as np
import pytest
import torch
from PIL import Image

import masked_oracle

pytestmark = pytest.mark.gpu

KW = dict(strength=0.8, num_inference_steps=4, guidance_scale=1.5, controlnet_conditioning_scale=0.5)


def synth_image(seed, size):
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:size, 0:size].astype(np.float32) / size
    img = np.stack([0.5 + 0.4 * np.sin(6.0 * xx + rng.uniform(0, 6)) * np.cos(4.0 * yy + rng.uniform(0, 6)) for _ in range(3)], axis=2)
    for _ in range(6):
        cx, cy, r = rng.uniform(0.1, 0.9), rng.uniform(0.1, 0.9), rng.uniform(0.05, 0.2)
        img[((xx - cx) ** 2 + (yy - cy) ** 2) < r * r] = rng.uniform(0, 1, 3)
    return Image.fromarray((img.clip(0, 1) * 255).astype(np.uint8))


def box_mask(size, x0, y0, x1, y1, value=255):
    m = np.zeros((size, size), np.uint8)
    m[y0:y1, x0:x1] = value
    return m


@pytest.fixture(scope="module", params=["tiny", "tiny-nomid"])
def rig(request, fie):
    from fie_amd import stack
    from fie_amd.pipe import HipImg2ImgPipeline
    cfgs, sds = stack.synthetic_stack(request.param, True, device="cpu", dtype=torch.float16)
    sds32 = {k: {n: v.float() for n, v in sd.items()} for k, sd in sds.items()}
    pipe = HipImg2ImgPipeline(fie, cfgs, sds, noise_dtype=torch.float32)
    return cfgs, sds32, pipe


def _ids(pipe, texts):
    return pipe.tok_l(texts), pipe.tok_g(texts)


def _ctrl(img):
    from oracle import canny
    return Image.fromarray(canny.canny_rgb(np.asarray(img)))


def _edit(pipe, img, seed, **kw):
    args = dict(KW)
    args.update(kw)
    return np.asarray(pipe(prompt="a [red] circle", negative_prompt="", image=img, control_image=_ctrl(img),
                           generator=torch.Generator("cpu").manual_seed(seed), **args).images[0])


# ------------------------------------------------------------------------------------------------------------------------ kernels
@pytest.mark.parametrize("dtype", [torch.float16, torch.float32])
@pytest.mark.parametrize("nb", [1, 2])
@pytest.mark.parametrize("last", [False, True])
def test_lcm_step_masked_closed_form(fie, dtype, nb, last):
    from fie_amd import hip
    ctx = hip.context(0, dtype)
    g = torch.Generator("cpu").manual_seed(nb * 10 + int(last))
    lh, lw = 16, 24
    hw = lh * lw
    dev = ctx.device
    eps = torch.randn((nb, lh, lw, 8), generator=g).to(dtype).to(dev)
    lat0 = torch.randn((hw, 4), generator=g).to(dev)
    noise = None if last else torch.randn((4, hw), generator=g).to(dev)
    z0 = torch.randn((hw, 4), generator=g).to(dev)
    n_init = torch.randn((4, hw), generator=g).to(dev)
    m_lat = (torch.rand(hw, generator=g) < 0.5).to(torch.uint8).to(dev)
    sc = dict(sab_t=0.35, s1mab_t=0.937, c_skip=0.002, c_out=0.998, sab_p=0.62, s1mab_p=0.785)
    outs = {}
    for masked in (False, True):
        lat = lat0.clone()
        model_in = torch.zeros((nb, lh, lw, 8), device=dev, dtype=dtype)
        dec = torch.zeros((1, lh, lw, 8), device=dev, dtype=dtype)
        args = (eps, nb, 1.7, lat, noise, hw, sc["sab_t"], sc["s1mab_t"], sc["c_skip"], sc["c_out"], sc["sab_p"], sc["s1mab_p"], model_in, 0.13, dec)
        if masked:
            ctx.lcm_step_masked(*args, m_lat, z0, n_init)
        else:
            ctx.lcm_step(*args)
        torch.cuda.synchronize()
        outs[masked] = (lat.cpu(), model_in.cpu(), dec.cpu())
    inside = m_lat.cpu().bool()
    # inside the mask: exactly what the unmasked step writes
    assert torch.equal(outs[True][0][inside], outs[False][0][inside])
    # the numpy closed form of the whole step
    e = eps.float().cpu().numpy().reshape(nb, hw, 8)[..., :4].astype(np.float64)
    if nb == 2:
        e = e[0] + 1.7 * (e[1] - e[0])
    else:
        e = e[0]
    x = lat0.cpu().numpy().astype(np.float64)
    den = sc["c_out"] * (x - sc["s1mab_t"] * e) / sc["sab_t"] + sc["c_skip"] * x
    z = z0.cpu().numpy().astype(np.float64)
    if not last:
        den = sc["sab_p"] * den + sc["s1mab_p"] * noise.cpu().numpy().T
        proper = sc["sab_p"] * z + sc["s1mab_p"] * n_init.cpu().numpy().T
    else:
        proper = z
    want = np.where(inside.numpy()[:, None], den, proper)
    lat, model_in, dec = outs[True]
    assert np.allclose(lat.numpy(), want, rtol=1e-5, atol=1e-5)
    mi = model_in.float().numpy().reshape(nb, hw, 8)
    for k in range(nb):
        assert np.array_equal(mi[k, :, :4], lat.numpy().astype(np.float16 if dtype == torch.float16 else np.float32).astype(np.float32))
        assert not mi[k, :, 4:].any()
    assert np.allclose(dec.float().numpy().reshape(hw, 8)[:, :4], lat.numpy() * 0.13, rtol=2e-3 if dtype == torch.float16 else 1e-6, atol=1e-6)


def test_mask_prep_resize_binarise_downsample_feather(fie):
    from fie_amd import mask as hmask
    rng = np.random.default_rng(4)
    src = (rng.integers(0, 2, (50, 70)) * 255).astype(np.uint8)
    src[10:30, 20:50] = rng.integers(90, 170, (20, 30))             # grey levels around the threshold
    pil = Image.fromarray(src, "L")
    for ow, oh in ((96, 80), (128, 128), (70, 48)):
        dev = fie.resize_lanczos(torch.from_numpy(src).cuda(), oh, ow)
        want = np.asarray(pil.resize((ow, oh), Image.LANCZOS))
        assert np.array_equal(dev.cpu().numpy(), want), (ow, oh)
    lm = np.asarray(pil.resize((96, 80), Image.LANCZOS))
    binary = (lm >= 128).astype(np.float32)
    for r in (0, 1.0, 2.5):
        m_px, m_lat = fie.mask_prep(torch.from_numpy(np.array(lm)).cuda(), r)
        torch.cuda.synchronize()
        assert np.array_equal(m_lat.cpu().numpy().reshape(10, 12), binary[::8, ::8].astype(np.uint8))
        if r == 0:
            assert np.array_equal(m_px.cpu().numpy(), binary)
        else:
            assert np.abs(m_px.cpu().numpy() - hmask.feather_numpy(binary, r)).max() <= 1e-5


@pytest.mark.parametrize("dtype", [torch.float16, torch.float32])
def test_pixels_out_composite(fie, dtype):
    from fie_amd import hip
    ctx = hip.context(0, dtype)
    g = torch.Generator("cpu").manual_seed(5)
    h, w = 40, 56
    dec = (torch.randn((1, h, w, 8), generator=g) * 1.2).to(dtype)
    src = torch.randint(0, 256, (h, w, 3), generator=g, dtype=torch.uint8)
    m = torch.rand((h, w), generator=g)
    m[:, :16] = 0
    m[:, 16:32] = 1
    got = ctx.pixels_out_composite(dec.cuda(), src.cuda(), m.cuda()).cpu().numpy()
    plain = ctx.pixels_out(dec.cuda()).cpu().numpy()
    want = masked_oracle.composite(dec[..., :3].float().permute(0, 3, 1, 2), src.numpy(), m.numpy())
    mm = m.numpy()
    hard = (mm == 0) | (mm == 1)
    assert np.array_equal(got[:, :16], src.numpy()[:, :16])
    assert np.array_equal(got[:, 16:32], plain[:, 16:32])
    assert np.array_equal(got[hard], want[hard])
    assert np.abs(got.astype(int) - want.astype(int)).max() <= 1


# ------------------------------------------------------------------------------------------------------------------------ edits
@pytest.mark.parametrize("guidance,strength", [(1.5, 0.8), (1.0, 0.5), (2.0, 1.0)])
def test_masked_edit_vs_masked_oracle(rig, guidance, strength):
    from oracle import metrics
    cfgs, sds32, pipe = rig
    img = synth_image(11, 128)
    mask = box_mask(128, 24, 40, 96, 104)
    kw = dict(strength=strength, num_inference_steps=4, guidance_scale=guidance, controlnet_conditioning_scale=0.5)
    out = _edit(pipe, img, 42, mask_image=mask, mask_blur=1.5, **kw)
    ref = masked_oracle.run_masked(sds32, cfgs, img, _ctrl(img), _ids(pipe, ["a [red] circle"]), _ids(pipe, [""]), mask, mask_blur=1.5,
                                   generator=torch.Generator("cpu").manual_seed(42), **kw)
    s = metrics.ssim(Image.fromarray(out), ref, size=None)
    print(f"masked edit vs masked oracle: ssim={s:.5f}")
    assert s >= 0.99
    outside = hmask_feather(mask, 1.5) == 0
    assert np.array_equal(out[outside], np.asarray(img)[outside])


def hmask_feather(mask, r):
    from fie_amd import mask as hmask
    return hmask.feather_numpy((mask >= 128).astype(np.float32), r)


def test_all_ones_mask_is_the_unmasked_edit(rig):
    _, _, pipe = rig
    img = synth_image(12, 128)
    ones = np.full((128, 128), 255, np.uint8)
    for graph in (False, True):
        pipe.use_graph = graph
        base = _edit(pipe, img, 7)
        for paste_back in (True, False):
            assert np.array_equal(_edit(pipe, img, 7, mask_image=ones, paste_back=paste_back), base), (graph, paste_back)
    pipe.use_graph = True


def test_paste_back_keeps_the_source(rig):
    _, _, pipe = rig
    img = synth_image(13, 128)
    src = np.asarray(img)
    mask = box_mask(128, 40, 32, 88, 80)
    for r in (0, 3.0):
        out = _edit(pipe, img, 9, mask_image=Image.fromarray(mask), mask_blur=r)
        outside = hmask_feather(mask, r) == 0
        assert outside.sum() > 5000 and np.array_equal(out[outside], src[outside]), r
        assert not np.array_equal(out[mask > 0], src[mask > 0])
    # all-zeros mask without the paste-back decodes z0: the VAE round trip of the source, close to it but not equal
    zero = _edit(pipe, img, 9, mask_image=np.zeros((128, 128), np.uint8), paste_back=False)
    assert not np.array_equal(zero, src)
    lat = pipe(prompt="a [red] circle", negative_prompt="", image=img, control_image=_ctrl(img), output_type="latent",
               mask_image=np.zeros((128, 128), bool), paste_back=False, generator=torch.Generator("cpu").manual_seed(9), **KW).images[0]
    assert lat.shape == (16, 16, 4)


def test_masked_graph_replay_matches_eager_and_takes_the_new_mask(rig):
    _, _, pipe = rig
    img = synth_image(14, 128)
    masks = [box_mask(128, 0, 0, 64, 128), box_mask(128, 48, 16, 128, 80)]
    eager, graph = [], []
    pipe.use_graph = False
    for m in masks:
        eager.append(_edit(pipe, img, 3, mask_image=m, mask_blur=2.0))
    pipe.use_graph = True
    n_graphs = len(pipe._graphs)
    for m in masks:
        graph.append(_edit(pipe, img, 3, mask_image=m, mask_blur=2.0))
    assert len(pipe._graphs) == n_graphs + 1                       # one masked graph, replayed with the second mask
    assert not np.array_equal(eager[0], eager[1])
    for a, b in zip(eager, graph):
        assert np.array_equal(a, b)


def test_cabi_run_edit_masked_matches_product_path(rig):
    from fie_amd import cabi
    _, _, pipe = rig
    img = synth_image(15, 128)
    mask = box_mask(128, 16, 16, 80, 112)
    cabi.register_pipeline(pipe)
    job = pipe.prepare("a [red] circle", "", img, _ctrl(img), generator=torch.Generator("cpu").manual_seed(4), mask_image=mask, **KW)
    out = cabi.run_edit(pipe, job).cpu().numpy()
    pipe.use_graph = False
    prod = _edit(pipe, img, 4, mask_image=mask)
    pipe.use_graph = True
    assert np.abs(out.astype(int) - prod.astype(int)).max() <= 3
    outside = mask == 0
    assert np.array_equal(out[outside], np.asarray(img)[outside])


# ------------------------------------------------------------------------------------------------------------------------ the prepared jobs
def prepared_jobs(pipe):
    """Six prepare*() calls at 64 x 64 that between them set every mask keyword -> {name: job}.  Nothing runs on the jobs."""
    img, img2 = synth_image(21, 64), synth_image(22, 64)
    ctrl, ctrl2 = _ctrl(img), _ctrl(img2)
    m = box_mask(64, 12, 8, 52, 44)
    gen = lambda seed: torch.Generator("cpu").manual_seed(seed)
    one = lambda **kw: pipe.prepare("a [red] circle", "", img, ctrl, generator=gen(1), **KW, **kw)
    return dict(unmasked=one(), blur=one(mask_image=m, mask_blur=2),
                content_blend_grow=one(mask_image=m, masked_content="fill", blend="multiband", blend_levels=3, mask_grow=4),
                ramp=one(mask_image=m, mask_ramp=8),
                batch=pipe.prepare_batch(["a [red] circle", "a dog"], None, [img, img2], [ctrl, ctrl2], generators=[gen(1), gen(2)],
                                         mask_image=[m, None], masked_content="latent_noise", **KW),
                sweep=pipe.prepare_sweep("a [red] circle", "", img, ctrl, strengths="all", generator=gen(1), mask_image=m,
                                         **{k: v for k, v in KW.items() if k != "strength"}))


def describe_job(job, base):
    """What of a prepared job the graph key and the C ABI read, as plain Python values: its keys, the mask entries that are not tensors, the
    shape and dtype of every tensor (and of every list of tensors), and the graph key's `base`."""
    plain = lambda v: tuple(plain(x) for x in v) if isinstance(v, (tuple, list)) else v.item() if isinstance(v, np.generic) else v
    shape = lambda t: (tuple(t.shape), str(t.dtype).replace("torch.", ""))
    return dict(keys=sorted(job), mask_cfg=job.get("mask_cfg"), content=job.get("content"), blend=job.get("blend"), sweep=job.get("sweep"),
                tensors={k: shape(v) for k, v in sorted(job.items()) if torch.is_tensor(v)},
                lists={k: [shape(t) for t in v] for k, v in sorted(job.items()) if isinstance(v, list) and v and torch.is_tensor(v[0])},
                base=plain(base))


# recorded by running prepared_jobs() / describe_job() on the commit before MaskSpec, with `base` as run_device_graphed computed it inline
PREPARED_JOBS = {'batch': {'base': ((64, 64), 2, (759, 499, 259), 1.5, 0.5, 0, 2, (True, 0.0, True, 'latent_noise')),
           'blend': None,
           'content': 'latent_noise',
           'keys': ['cn_scale', 'content', 'content_lat', 'ctl_u8', 'eos_rows', 'guidance', 'hw', 'ids_g', 'ids_l', 'img_u8', 'mask_cfg', 'mask_l', 'mask_lat',
                    'mask_px', 'n', 'nb', 'noises', 'steps', 't_dev', 'time_ids'],
           'lists': {'noises': [((1, 4, 8, 8), 'float32'), ((1, 4, 8, 8), 'float32'), ((1, 4, 8, 8), 'float32'), ((1, 4, 8, 8), 'float32'),
                                ((1, 4, 8, 8), 'float32'), ((1, 4, 8, 8), 'float32'), ((1, 4, 8, 8), 'float32'), ((1, 4, 8, 8), 'float32')],
                     't_dev': [((4, 1), 'float32'), ((4, 1), 'float32'), ((4, 1), 'float32')]},
           'mask_cfg': (0.0, True),
           'sweep': None,
           'tensors': {'content_lat': ((2, 64), 'uint8'),
                       'ctl_u8': ((2, 64, 64, 3), 'uint8'),
                       'eos_rows': ((4,), 'int32'),
                       'ids_g': ((4, 77), 'int32'),
                       'ids_l': ((4, 77), 'int32'),
                       'img_u8': ((2, 64, 64, 3), 'uint8'),
                       'mask_l': ((2, 64, 64), 'uint8'),
                       'mask_lat': ((2, 64), 'uint8'),
                       'mask_px': ((2, 64, 64), 'float32'),
                       'time_ids': ((4, 6), 'float32')}},
 'blur': {'base': ((64, 64), 2, (759, 499, 259), 1.5, 0.5, 0, 1, (True, 2.0, True)),
          'blend': None,
          'content': None,
          'keys': ['cn_scale', 'ctl_u8', 'eos_rows', 'guidance', 'hw', 'ids_g', 'ids_l', 'img_u8', 'mask_cfg', 'mask_lat', 'mask_px', 'nb', 'noises', 'steps',
                   't_dev', 'time_ids'],
          'lists': {'noises': [((1, 4, 8, 8), 'float32'), ((1, 4, 8, 8), 'float32'), ((1, 4, 8, 8), 'float32'), ((1, 4, 8, 8), 'float32')],
                    't_dev': [((2, 1), 'float32'), ((2, 1), 'float32'), ((2, 1), 'float32')]},
          'mask_cfg': (2.0, True),
          'sweep': None,
          'tensors': {'ctl_u8': ((64, 64, 3), 'uint8'),
                      'eos_rows': ((2,), 'int32'),
                      'ids_g': ((2, 77), 'int32'),
                      'ids_l': ((2, 77), 'int32'),
                      'img_u8': ((64, 64, 3), 'uint8'),
                      'mask_lat': ((1, 64), 'uint8'),
                      'mask_px': ((1, 64, 64), 'float32'),
                      'time_ids': ((2, 6), 'float32')}},
 'content_blend_grow': {'base': ((64, 64), 2, (759, 499, 259), 1.5, 0.5, 0, 1, (True, 0.0, True, 'fill', ('multiband', 3))),
                        'blend': ('multiband', 3),
                        'content': 'fill',
                        'keys': ['blend', 'blend_l', 'cn_scale', 'content', 'ctl_u8', 'eos_rows', 'guidance', 'hw', 'ids_g', 'ids_l', 'img_u8', 'mask_cfg', 'mask_l',
                                 'mask_lat', 'mask_px', 'nb', 'noises', 'steps', 't_dev', 'time_ids'],
                        'lists': {'noises': [((1, 4, 8, 8), 'float32'), ((1, 4, 8, 8), 'float32'), ((1, 4, 8, 8), 'float32'), ((1, 4, 8, 8), 'float32')],
                                  't_dev': [((2, 1), 'float32'), ((2, 1), 'float32'), ((2, 1), 'float32')]},
                        'mask_cfg': (0.0, True),
                        'sweep': None,
                        'tensors': {'blend_l': ((1, 64, 64), 'uint8'),
                                    'ctl_u8': ((64, 64, 3), 'uint8'),
                                    'eos_rows': ((2,), 'int32'),
                                    'ids_g': ((2, 77), 'int32'),
                                    'ids_l': ((2, 77), 'int32'),
                                    'img_u8': ((64, 64, 3), 'uint8'),
                                    'mask_l': ((1, 64, 64), 'uint8'),
                                    'mask_lat': ((1, 64), 'uint8'),
                                    'mask_px': ((1, 64, 64), 'float32'),
                                    'time_ids': ((2, 6), 'float32')}},
 'ramp': {'base': ((64, 64), 2, (759, 499, 259), 1.5, 0.5, 0, 1, (True, 0.0, True, 'levels')),
          'blend': None,
          'content': None,
          'keys': ['cn_scale', 'ctl_u8', 'eos_rows', 'guidance', 'hw', 'ids_g', 'ids_l', 'img_u8', 'lvl_lat', 'mask_cfg', 'mask_lat', 'mask_px', 'nb', 'noises',
                   'steps', 't_dev', 'time_ids'],
          'lists': {'noises': [((1, 4, 8, 8), 'float32'), ((1, 4, 8, 8), 'float32'), ((1, 4, 8, 8), 'float32'), ((1, 4, 8, 8), 'float32')],
                    't_dev': [((2, 1), 'float32'), ((2, 1), 'float32'), ((2, 1), 'float32')]},
          'mask_cfg': (0.0, True),
          'sweep': None,
          'tensors': {'ctl_u8': ((64, 64, 3), 'uint8'),
                      'eos_rows': ((2,), 'int32'),
                      'ids_g': ((2, 77), 'int32'),
                      'ids_l': ((2, 77), 'int32'),
                      'img_u8': ((64, 64, 3), 'uint8'),
                      'lvl_lat': ((1, 64), 'uint8'),
                      'mask_lat': ((1, 64), 'uint8'),
                      'mask_px': ((1, 64, 64), 'float32'),
                      'time_ids': ((2, 6), 'float32')}},
 'sweep': {'base': ((64, 64), 2, (999, 759, 499, 259), 1.5, 0.5, 0, 1, (True, 0.0, True), ('sweep', (4, 3, 2, 1))),
           'blend': None,
           'content': None,
           'keys': ['cn_scale', 'ctl_u8', 'eos_rows', 'guidance', 'hw', 'ids_g', 'ids_l', 'img_u8', 'mask_cfg', 'mask_lat', 'mask_px', 'nb', 'noises', 'plans',
                    'sched', 'steps', 'sweep', 't_dev', 'time_ids'],
           'lists': {'noises': [((1, 4, 8, 8), 'float32'), ((1, 4, 8, 8), 'float32'), ((1, 4, 8, 8), 'float32'), ((1, 4, 8, 8), 'float32'),
                                ((1, 4, 8, 8), 'float32')],
                     't_dev': [((2, 1), 'float32'), ((4, 1), 'float32'), ((6, 1), 'float32'), ((8, 1), 'float32')]},
           'mask_cfg': (0.0, True),
           'sweep': (4, 3, 2, 1),
           'tensors': {'ctl_u8': ((64, 64, 3), 'uint8'),
                       'eos_rows': ((2,), 'int32'),
                       'ids_g': ((2, 77), 'int32'),
                       'ids_l': ((2, 77), 'int32'),
                       'img_u8': ((64, 64, 3), 'uint8'),
                       'mask_lat': ((1, 64), 'uint8'),
                       'mask_px': ((1, 64, 64), 'float32'),
                       'time_ids': ((2, 6), 'float32')}},
 'unmasked': {'base': ((64, 64), 2, (759, 499, 259), 1.5, 0.5, 0, 1),
              'blend': None,
              'content': None,
              'keys': ['cn_scale', 'ctl_u8', 'eos_rows', 'guidance', 'hw', 'ids_g', 'ids_l', 'img_u8', 'mask_cfg', 'mask_lat', 'mask_px', 'nb', 'noises', 'steps',
                       't_dev', 'time_ids'],
              'lists': {'noises': [((1, 4, 8, 8), 'float32'), ((1, 4, 8, 8), 'float32'), ((1, 4, 8, 8), 'float32'), ((1, 4, 8, 8), 'float32')],
                        't_dev': [((2, 1), 'float32'), ((2, 1), 'float32'), ((2, 1), 'float32')]},
              'mask_cfg': None,
              'sweep': None,
              'tensors': {'ctl_u8': ((64, 64, 3), 'uint8'),
                          'eos_rows': ((2,), 'int32'),
                          'ids_g': ((2, 77), 'int32'),
                          'ids_l': ((2, 77), 'int32'),
                          'img_u8': ((64, 64, 3), 'uint8'),
                          'time_ids': ((2, 6), 'float32')}}}


def test_prepared_jobs_are_what_they_were_before_the_spec(rig):
    """The prepare family behind MaskSpec builds the jobs it built from the loose keywords: same keys, same mask_cfg / content / blend / sweep
    values, same tensor shapes and dtypes, and the same graph key."""
    _, _, pipe = rig
    jobs = prepared_jobs(pipe)
    assert set(jobs) == set(PREPARED_JOBS)
    for name, job in jobs.items():
        got = describe_job(job, pipe._graph_base(job, 0))
        assert got == PREPARED_JOBS[name], name
        assert pprint.pformat(got) == pprint.pformat(PREPARED_JOBS[name]), name              # and of the same types: 0.0 is not 0, True is not 1


# ------------------------------------------------------------------------------------------------------------------------ product surfaces
@pytest.fixture(scope="module")
def editor(fie):
    from src.pipeline import FastEditor
    return FastEditor(model_name="tiny", enable_cpu_offload=False)


def test_edit_batch_with_masks_matches_serial(editor):
    imgs = [synth_image(60 + i, 96) for i in range(3)]
    prompts = [f"a [toy] number {i}" for i in range(3)]
    masks = [box_mask(96, 10, 10, 60, 70), None, Image.fromarray(box_mask(96, 30, 0, 96, 50))]
    serial = [np.asarray(editor.edit(im, p, seed=11, strength=0.5, mask=m)) for im, p, m in zip(imgs, prompts, masks)]
    batch = [np.asarray(o) for o in editor.edit_batch(imgs, prompts, seed=11, strength=0.5, masks=masks)]
    for a, b in zip(serial, batch):
        assert a.shape == b.shape == (1024, 1024, 3)
        assert np.abs(a.astype(int) - b.astype(int)).max() <= 2
    src0 = np.asarray(imgs[0].resize((1024, 1024), Image.LANCZOS))
    m0 = np.asarray(Image.fromarray(masks[0]).resize((1024, 1024), Image.LANCZOS)) < 128
    assert np.array_equal(batch[0][m0], src0[m0])


def test_full_size_edit_with_a_512_mask(editor):
    img = synth_image(70, 512)
    mask = box_mask(512, 100, 150, 300, 400)
    out = np.asarray(editor.edit(img, "a [blue] ball", seed=5, strength=0.5, mask=Image.fromarray(mask), mask_blur=2.0))
    src = np.asarray(img.resize((1024, 1024), Image.LANCZOS))
    m_l = np.asarray(Image.fromarray(mask).convert("L").resize((1024, 1024), Image.LANCZOS))
    outside = hmask_feather(m_l, 2.0) == 0
    assert out.shape == (1024, 1024, 3) and outside.mean() > 0.5
    assert np.array_equal(out[outside], src[outside])
    assert not np.array_equal(out[m_l >= 128], src[m_l >= 128])


def test_run_batch_use_mask_end_to_end(editor, tmp_path):
    import run_batch
    from fie_amd import mask as hmask
    from tools import make_synthetic_piebench as msp
    data = tmp_path / "pie"
    msp.main(["--out", str(data), "--num", "2", "--with_masks"])
    mapping = json.load(open(data / "mapping_file.json"))
    nomask = dict(next(iter(mapping.values())))
    nomask.pop("mask")
    mapping["nomask"] = nomask
    entries = [(i, k, e) for i, (k, e) in enumerate(mapping.items())]
    out = tmp_path / "out"
    args = run_batch.add_mask_args(run_batch.build_parser()).parse_args(
        ["--source_dir", str(data / "annotation_images"), "--output_dir", str(out), "--seed", "42", "--strength", "0.5", "--use_mask"])
    r = run_batch.process_shard(editor, entries, args, str(out / "e"), str(out / "c"))
    assert (r["processed"], r["skipped"], r["failed"]) == (2, 0, 1)
    for k, e in list(mapping.items())[:2]:
        got = np.asarray(Image.open(out / "e" / e["image_path"]).convert("RGB")).astype(int)
        src = Image.open(data / "annotation_images" / e["image_path"]).convert("RGB")
        m = hmask.rle_decode(e["mask"])
        want = np.asarray(editor.edit(src, e["editing_prompt"], seed=42, strength=0.5, mask=m)).astype(int)
        assert got.shape == (1024, 1024, 3) and np.abs(got - want).mean() < 4.0       # a JPEG round trip apart
        outside = np.asarray(Image.fromarray(m).resize((1024, 1024), Image.LANCZOS)) < 128
        src_u8 = np.asarray(src.resize((1024, 1024), Image.LANCZOS)).astype(int)
        assert np.array_equal(want[outside], src_u8[outside])
