"""Masked-content modes on the device: the hole-fill op and the edge-map clear bit for bit against the numpy restatement
(tests/masked_content_oracle.py), the latent-prep twin against fie_latent_prep_src's own bits, the modes in the pipeline on the tiny stack at
64x64 (every comparison a bit equality except the batch, which keeps the bound of the masked batch test in tests/test_masked_edit_gpu.py), and
one FastEditor call at the product surface."""
import numpy as np
import pytest
import torch
from PIL import Image

import masked_content_oracle as mco

pytestmark = pytest.mark.gpu

MODES = ("original", "fill", "latent_noise", "latent_nothing")
NEW = MODES[1:]
KW = dict(strength=0.8, num_inference_steps=4, guidance_scale=1.5, controlnet_conditioning_scale=0.5)


def _dev(fie, a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(fie.device)


# ------------------------------------------------------------------------------------------------------------------------ the fill op
# 72x88: levels 9, 5, 3 have odd sides (ceil-halving, the clamped neighbour) and level 1 (1584 cells) goes through the per-level kernels;
# 200x136: two per-level pushes and resolves; 8x8, 24x40: level 1 already belongs to the one-block kernel; 1x1: no pyramid at all
@pytest.mark.parametrize("h,w", [(8, 8), (24, 40), (72, 88), (200, 136), (1, 1)])
def test_fill_and_edge_clear_match_the_restatement(fie, h, w):
    src = mco.case_image(h, w, h * 100 + w)
    ctl = (np.random.default_rng(w).integers(0, 2, (h, w, 1), dtype=np.uint8) * 255).repeat(3, 2)
    for name, mask in mco.case_masks(h, w, w).items():
        filled, cleared = fie.mask_fill(_dev(fie, src), _dev(fie, mask), _dev(fie, ctl))
        assert np.array_equal(filled.cpu().numpy(), mco.fill(src, mask)), name
        assert np.array_equal(cleared.cpu().numpy(), mco.clear_edges(ctl, mask)), name
        only, none = fie.mask_fill(_dev(fie, src), _dev(fie, mask))          # the control pair is optional
        assert none is None and np.array_equal(only.cpu().numpy(), mco.fill(src, mask)), name


def test_clear_only_form_writes_no_image(fie):
    """out == NULL: one launch that clears the edge map; neither the source nor a workspace is touched (both may be NULL)."""
    from fie_amd import hip
    h, w = 72, 88
    src = mco.case_image(h, w, 1)
    ctl = mco.case_image(h, w, 2)
    mask = mco.case_masks(h, w, 3)["threshold"]
    none, cleared = fie.mask_fill(_dev(fie, src), _dev(fie, mask), _dev(fie, ctl), fill=False)
    assert none is None and np.array_equal(cleared.cpu().numpy(), mco.clear_edges(ctl, mask))
    lib, p = hip.lib(), hip._p
    fie.sync_stream()
    nbytes = lib.fie_mask_fill_workspace_bytes(h, w)
    ws = torch.full((nbytes,), 0xA5, dtype=torch.uint8, device=fie.device)
    s_dev, m_dev, c_dev = _dev(fie, src), _dev(fie, mask), _dev(fie, ctl)
    for s_arg, ws_arg in ((s_dev, ws), (None, None)):
        out = torch.full((h, w, 3), 0x5A, dtype=torch.uint8, device=fie.device)
        hip._chk(lib.fie_mask_fill_rgb_u8(fie.h, p(s_arg), p(m_dev), h, w, p(ws_arg), None, p(c_dev), p(out)))
        assert np.array_equal(out.cpu().numpy(), mco.clear_edges(ctl, mask))
    assert (ws.cpu().numpy() == 0xA5).all() and np.array_equal(s_dev.cpu().numpy(), src)
    # in place: out may be src, ctl_out may be ctl_in
    hip._chk(lib.fie_mask_fill_rgb_u8(fie.h, p(s_dev), p(m_dev), h, w, p(ws), p(s_dev), p(c_dev), p(c_dev)))
    assert np.array_equal(s_dev.cpu().numpy(), mco.fill(src, mask)) and np.array_equal(c_dev.cpu().numpy(), mco.clear_edges(ctl, mask))
    with pytest.raises(hip.FieError):
        hip._chk(lib.fie_mask_fill_rgb_u8(fie.h, p(s_dev), p(m_dev), h, w, p(ws), None, None, None))


# ------------------------------------------------------------------------------------------------------------------------ the latent-prep twin
@pytest.mark.parametrize("dtype", [torch.float16, torch.float32])
def test_latent_prep_twin(fie, dtype):
    from fie_amd import hip
    ctx = hip.context(0, dtype)
    g = torch.Generator("cpu").manual_seed(21)
    lh, lw, nb = 16, 24, 2
    hw = lh * lw
    dev = ctx.device
    moments = torch.randn((1, lh, lw, 8), generator=g).to(dtype).to(dev)
    eps_post = torch.randn((1, 4, lh, lw), generator=g).to(dev)
    n_init = torch.randn((1, 4, lh, lw), generator=g).to(dev)
    m_lat = (torch.rand(hw, generator=g) < 0.5).to(torch.uint8)
    sf, sab, s1mab = 0.13025, 0.35, 0.937

    def run(mode):
        lat = torch.full((hw, 4), 7.0, device=dev)
        z0 = torch.full((hw, 4), 7.0, device=dev)
        model_in = torch.full((nb, lh, lw, 8), 7.0, device=dev, dtype=dtype)
        if mode is None:
            ctx.latent_prep_src(moments, eps_post, n_init, hw, sf, sab, s1mab, lat, model_in, z0)
        else:
            ctx.latent_prep_src_content(moments, eps_post, n_init, hw, sf, sab, s1mab, lat, model_in, z0, m_lat.to(dev), mode)
        torch.cuda.synchronize()
        return lat.cpu().numpy(), model_in.float().cpu().numpy().reshape(nb, hw, 8), z0.cpu().numpy()

    lat0, mi0, z00 = run(None)
    inside = m_lat.numpy().astype(bool)
    assert 0 < inside.sum() < hw
    noise = n_init.cpu().numpy().reshape(4, hw)
    npdt = np.float16 if dtype == torch.float16 else np.float32
    for mode in MODES:
        lat, mi, z0 = run(mode)
        assert np.array_equal(z0.view(np.uint32), z00.view(np.uint32)), mode                     # z0: the original op's everywhere
        want = mco.initial_latents(mode, lat0, noise, inside, s1mab)
        assert np.array_equal(lat.view(np.uint32), want.view(np.uint32)), mode
        assert np.array_equal(lat[~inside].view(np.uint32), lat0[~inside].view(np.uint32)), mode
        assert np.array_equal(mi[:, ~inside], mi0[:, ~inside]), mode
        for k in range(nb):                                                                      # model_in: cast from the selected value
            assert np.array_equal(mi[k, :, :4], want.astype(npdt).astype(np.float32)), mode
            assert not mi[k, :, 4:].any()
    assert np.array_equal(run("latent_noise")[0][inside], noise.T[inside])
    assert np.array_equal(run("latent_nothing")[0][inside], (np.float32(s1mab) * noise.T)[inside])


# ------------------------------------------------------------------------------------------------------------------------ the pipeline, 64x64
SIZE = 64


def synth_image(seed, size=SIZE):
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:size, 0:size].astype(np.float32) / size
    img = np.stack([0.5 + 0.4 * np.sin(6.0 * xx + rng.uniform(0, 6)) * np.cos(4.0 * yy + rng.uniform(0, 6)) for _ in range(3)], axis=2)
    for _ in range(4):
        cx, cy, r = rng.uniform(0.1, 0.9), rng.uniform(0.1, 0.9), rng.uniform(0.1, 0.25)
        img[((xx - cx) ** 2 + (yy - cy) ** 2) < r * r] = rng.uniform(0, 1, 3)
    return Image.fromarray((img.clip(0, 1) * 255).astype(np.uint8))


def box_mask(x0, y0, x1, y1, size=SIZE):
    m = np.zeros((size, size), np.uint8)
    m[y0:y1, x0:x1] = 255
    return m


@pytest.fixture(scope="module")
def pipe(fie):
    from fie_amd import stack
    from fie_amd.pipe import HipImg2ImgPipeline
    cfgs, sds = stack.synthetic_stack("tiny", True, device="cpu", dtype=torch.float16)
    return HipImg2ImgPipeline(fie, cfgs, sds, noise_dtype=torch.float32)


def _ctrl(img):
    from oracle import canny
    return Image.fromarray(canny.canny_rgb(np.asarray(img)))


def _edit(pipe, img, seed, graph=False, ctl=None, **kw):
    pipe.use_graph = graph
    try:
        return np.asarray(pipe(prompt="a [red] circle", negative_prompt="", image=img, control_image=ctl if ctl is not None else _ctrl(img),
                               generator=torch.Generator("cpu").manual_seed(seed), **dict(KW, **kw)).images[0])
    finally:
        pipe.use_graph = True


IMG = synth_image(31)
MASK = box_mask(8, 16, 40, 48)                     # latent cells 1..4 x 2..5 of the 8 x 8 latent
MASK2 = box_mask(24, 0, 64, 40)


@pytest.fixture(scope="module")
def original(pipe):
    """The masked edit as it was before the modes existed, computed once: (paste-back on, paste-back off)."""
    return _edit(pipe, IMG, 5, mask_image=MASK), _edit(pipe, IMG, 5, mask_image=MASK, paste_back=False)


def test_explicit_original_is_the_default(pipe, original):
    assert np.array_equal(_edit(pipe, IMG, 5, mask_image=MASK, masked_content="original"), original[0])
    keys = set(pipe.prepare("p", "", IMG, _ctrl(IMG), mask_image=MASK, masked_content="original"))
    assert keys == set(pipe.prepare("p", "", IMG, _ctrl(IMG), mask_image=MASK)) and not {"content", "mask_l", "content_lat"} & keys
    with pytest.raises(ValueError, match="needs a mask"):
        pipe.prepare("p", "", IMG, _ctrl(IMG), masked_content="fill")
    with pytest.raises(ValueError, match="latent_nothing"):
        pipe.prepare("p", "", IMG, _ctrl(IMG), mask_image=MASK, masked_content="noise")


@pytest.mark.parametrize("mode", NEW)
def test_all_zeros_mask_is_the_original_masked_edit(pipe, mode):
    zeros = np.zeros((SIZE, SIZE), np.uint8)
    for paste_back in (True, False):
        want = _edit(pipe, IMG, 6, mask_image=zeros, paste_back=paste_back)
        assert np.array_equal(_edit(pipe, IMG, 6, mask_image=zeros, paste_back=paste_back, masked_content=mode), want), paste_back


def test_fill_is_the_original_edit_of_the_filled_source(pipe, original):
    src, ctl = np.asarray(IMG), np.asarray(_ctrl(IMG))
    got = _edit(pipe, IMG, 5, mask_image=MASK, paste_back=False, masked_content="fill")
    want = _edit(pipe, Image.fromarray(mco.fill(src, MASK)), 5, ctl=Image.fromarray(mco.clear_edges(ctl, MASK)), mask_image=MASK, paste_back=False)
    assert np.array_equal(got, want)
    assert not np.array_equal(got, original[1])
    # with the paste-back the composite still blends against the ORIGINAL source: outside the mask the caller's bytes, not the filled image's
    pasted = _edit(pipe, IMG, 5, mask_image=MASK, masked_content="fill")
    assert np.array_equal(pasted[MASK == 0], src[MASK == 0]) and np.array_equal(pasted[MASK > 0], got[MASK > 0])


@pytest.mark.parametrize("mode", ["latent_noise", "latent_nothing"])
def test_latent_modes_change_the_inside_and_keep_the_outside(pipe, original, mode):
    src = np.asarray(IMG)
    out = _edit(pipe, IMG, 5, mask_image=MASK, masked_content=mode)
    assert not np.array_equal(out[MASK > 0], original[0][MASK > 0])
    assert np.array_equal(out[MASK == 0], src[MASK == 0])


@pytest.mark.parametrize("mode", NEW)
def test_graph_replay_matches_eager_and_takes_the_new_mask(pipe, mode):
    eager = [_edit(pipe, IMG, 3, mask_image=m, mask_blur=1.0, masked_content=mode) for m in (MASK, MASK2)]
    n_graphs = len(pipe._graphs)
    graph = [_edit(pipe, IMG, 3, graph=True, mask_image=m, mask_blur=1.0, masked_content=mode) for m in (MASK, MASK2)]
    assert len(pipe._graphs) == n_graphs + 1                       # one graph per mode, replayed with the second mask
    assert any(isinstance(k[0][-1], tuple) and k[0][-1][-1] == mode for k in pipe._graphs) and not np.array_equal(eager[0], eager[1])
    for a, b in zip(eager, graph):
        assert np.array_equal(a, b)


def test_original_graph_key_is_unchanged(pipe):
    _edit(pipe, IMG, 3, graph=True, mask_image=MASK, masked_content="original")
    masked = [k[0][-1] for k in pipe._graphs if isinstance(k[0][-1], tuple) and k[0][-1][0] is True]
    assert (True, 0.0, True) in masked                              # (masked, mask_blur, paste_back): no mode in an "original" key


@pytest.mark.parametrize("mode", NEW)
def test_batch_with_a_masked_and_an_unmasked_image_matches_serial(pipe, mode):
    imgs = [IMG, synth_image(32)]
    ctls = [_ctrl(im) for im in imgs]
    prompts = ["a [red] circle", "a [toy] boat"]
    gens = lambda: [torch.Generator("cpu").manual_seed(11) for _ in imgs]
    pipe.use_graph = False
    try:
        serial = [np.asarray(pipe(prompt=p, negative_prompt="", image=im, control_image=c, generator=g, mask_image=m,
                                  **dict(KW, **({"masked_content": mode} if m is not None else {}))).images[0])
                  for p, im, c, g, m in zip(prompts, imgs, ctls, gens(), [MASK, None])]
        batch = pipe(prompt=prompts, negative_prompt=["", ""], image=imgs, control_image=ctls, generator=gens(), mask_image=[MASK, None],
                     masked_content=mode, **KW).images
    finally:
        pipe.use_graph = True
    for a, b in zip(serial, batch):
        diff = np.abs(a.astype(int) - np.asarray(b).astype(int)).max()
        print(f"[masked_content batch] {mode}: max diff {diff}")
        assert diff <= 2                                            # the bound of test_masked_edit_gpu.py::test_edit_batch_with_masks_matches_serial
    assert np.array_equal(np.asarray(batch[0])[MASK == 0], np.asarray(IMG)[MASK == 0])


# ------------------------------------------------------------------------------------------------------------------------ the product surface
RES = (512, 512)


@pytest.fixture(scope="module")
def editor(fie):
    from src.pipeline import FastEditor
    return FastEditor(model_name="tiny", enable_cpu_offload=False)


def test_region_fill_edit_with_metrics(editor):
    from fie_amd import region as hregion
    img = synth_image(41, 96).crop((0, 0, 96, 80))                  # 96 x 80
    mask = np.zeros((80, 96), np.uint8)
    mask[30:52, 40:66] = 255
    kw = dict(seed=8, strength=0.6, resolution=RES, mask_blur=1.0, masked_content="fill")
    out, scores = editor.edit(img, "an [empty] table", mask=mask, region="mask", region_padding=8, metrics=True, **kw)
    box = hregion.resolve("mask", img.size, mask, 8, RES)
    l, t, r, b = box
    src, got = np.asarray(img), np.asarray(out)
    outside = np.ones((80, 96), bool)
    outside[t:b, l:r] = False
    assert out.size == img.size and outside.any() and np.array_equal(got[outside], src[outside])
    assert {"ssim", "psnr", "mse", "bg_ssim", "bg_psnr", "bg_mse"} <= set(scores)
    crop = editor.edit(img.crop(box), "an [empty] table", mask=Image.fromarray(mask).crop(box), output_size="source", **kw)
    want = src.copy()
    want[t:b, l:r] = np.asarray(crop)
    assert np.array_equal(got, want)
    assert not np.array_equal(got[mask >= 128], src[mask >= 128])
    plain = editor.edit(img, "an [empty] table", mask=mask, region="mask", region_padding=8, **dict(kw, masked_content="original"))
    assert not np.array_equal(np.asarray(plain), got)
    with pytest.raises(ValueError, match="needs a mask"):
        editor.edit(img, "p", masked_content="fill")
    with pytest.raises(ValueError, match="latent_noise"):
        editor.edit(img, "p", mask=mask, masked_content="blur")


def test_edit_batch_leaves_the_unmasked_image_as_it_was(editor):
    imgs = [synth_image(42, 96), synth_image(43, 96)]
    prompts = ["a [toy] number 0", "a [toy] number 1"]
    mask = box_mask(20, 10, 70, 60, 96)
    kw = dict(seed=11, strength=0.5, resolution=RES)
    serial = [np.asarray(editor.edit(imgs[0], prompts[0], mask=mask, masked_content="latent_noise", **kw)),
              np.asarray(editor.edit(imgs[1], prompts[1], **kw))]
    batch = [np.asarray(o) for o in editor.edit_batch(imgs, prompts, masks=[mask, None], masked_content="latent_noise", **kw)]
    for a, b in zip(serial, batch):
        assert a.shape == b.shape == (512, 512, 3)
        assert np.abs(a.astype(int) - b.astype(int)).max() <= 2
    with pytest.raises(ValueError, match="needs a mask"):
        editor.edit_batch(imgs, prompts, masked_content="fill", **kw)
