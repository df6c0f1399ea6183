"""The one-sided multi-band paste-back on the device: the op bit for bit against the numpy restatement
(tests/multiband_oracle.py), the blend in the pipeline on the tiny stack at 64x64 (every comparison a bit equality; the batch is compared with
the restatement applied to the batch's own decoded bytes, and its decoded bytes with the serial ones under the bound of the masked batch test in
tests/test_masked_edit_gpu.py), and FastEditor at the product surface."""
import numpy as np
import pytest
import torch
from PIL import Image

import multiband_oracle as mbo

pytestmark = pytest.mark.gpu

KW = dict(strength=0.8, num_inference_steps=4, guidance_scale=1.5, controlnet_conditioning_scale=0.5)
MB = dict(blend="multiband")


def _dev(fie, a):
    return torch.from_numpy(np.array(a, order="C")).to(fie.device)                 # a writable copy (PIL arrays are read-only)


# ------------------------------------------------------------------------------------------------------------------------ the op
def _feathered(fie, mask, radius=3):
    """A feathered mask_px from fie_mask_prep at the image's size.  The entry takes sides that are multiples of 8, so the mask is edge-padded up to
    one, feathered there and cropped: to the blend, alpha is an operand like any other (the restatement composites with the same array)."""
    h, w = mask.shape
    padded = np.pad(mask, ((0, -h % 8), (0, -w % 8)), mode="edge")
    m_px, _ = fie.mask_prep(_dev(fie, padded), radius / 3.0)
    alpha = m_px[:h, :w].contiguous()
    a = alpha.cpu().numpy()
    if h * w > 64:
        assert ((a > 0) & (a < 1)).any()                                 # there is a ramp to blend over
    return alpha, a


# 1x1: every level is one cell; 5x7: odd sides below one tile, every tap clamped; 24x40: several tiles at level 0, one above; 72x88: partial
# tiles on both axes, odd sides at levels 3 .. 5; 33x130: an odd side that crosses a tile and its halo, 9 tiles across; 200x136: 13 x 9 tiles,
# more than one tile at levels 1 .. 3
@pytest.mark.parametrize("h,w", [(1, 1), (5, 7), (24, 40), (72, 88), (33, 130), (200, 136)])
def test_op_matches_the_restatement(fie, h, w):
    from fie_amd import hip
    A, S = mbo.case_images(h, w, 100 * h + w)
    full, zero = np.full((h, w, 3), 255, np.uint8), np.zeros((h, w, 3), np.uint8)
    blob = mbo.blob_mask(h, w, w)
    coin = np.random.default_rng(h).integers(0, 2, (h, w), dtype=np.uint8) * 255
    cases = {"random": (A, S, blob), "extreme": (full, zero, coin), "extreme-": (zero, full, coin)}
    alpha_dev, alpha = _feathered(fie, blob)
    for name, (a, s, mask) in cases.items():
        a_dev, s_dev, m_dev = _dev(fie, a), _dev(fie, s), _dev(fie, mask)
        for L in (1, 3, 6):
            want = mbo.multiband(a, s, mask, L)
            want_alpha = mbo.multiband(a, s, mask, L, alpha=alpha)
            # a poisoned workspace of exactly the size the entry asks for and a poisoned output of its own: no stale level is read, every byte is written
            nbytes = hip.lib().fie_multiband_workspace_bytes(h, w, L)
            for al_dev, ref in ((None, want), (alpha_dev, want_alpha)):
                ws = torch.full((nbytes,), 0xA5, dtype=torch.uint8, device=fie.device)
                out = torch.full((h, w, 3), 0x5A, dtype=torch.uint8, device=fie.device)
                got = fie.multiband_blend(a_dev, s_dev, m_dev, alpha=al_dev, levels=L, out=out, workspace=ws)
                assert got is out
                bad = np.argwhere(got.cpu().numpy() != ref)
                assert bad.size == 0, (name, L, al_dev is not None, len(bad), bad[:4].tolist())
            assert np.array_equal(fie.multiband_blend(a_dev, s_dev, m_dev, levels=L).cpu().numpy(), want), (name, L)     # its own workspace and output
        assert np.array_equal(a_dev.cpu().numpy(), a) and np.array_equal(s_dev.cpu().numpy(), s) and np.array_equal(m_dev.cpu().numpy(), mask)


def test_op_refuses_bad_arguments(fie):
    from fie_amd import hip
    A, S = mbo.case_images(24, 40, 1)
    mask = mbo.blob_mask(24, 40, 2)
    a, s, m = _dev(fie, A), _dev(fie, S), _dev(fie, mask)
    for L in (0, 7):
        with pytest.raises(hip.FieError):
            fie.multiband_blend(a, s, m, levels=L)
    with pytest.raises(ValueError):
        fie.multiband_blend(a, s, m[:, :39].contiguous())
    with pytest.raises(ValueError):
        fie.multiband_blend(a, s, m, out=a)                              # out is no operand
    with pytest.raises(ValueError):
        fie.multiband_blend(a, s, m, alpha=torch.zeros((24, 40), dtype=torch.float16, device=fie.device))
    with pytest.raises(ValueError):
        fie.multiband_blend(a, s, m, levels=4, workspace=torch.empty(16, dtype=torch.uint8, device=fie.device))


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


def _edit(pipe, img, seed, graph=False, **kw):
    pipe.use_graph = graph
    try:
        return np.asarray(pipe(prompt="a [red] circle", negative_prompt="", image=img, control_image=_ctrl(img),
                               generator=torch.Generator("cpu").manual_seed(seed), **dict(KW, **kw)).images[0])
    finally:
        pipe.use_graph = True


IMG = synth_image(31)
SRC = np.asarray(IMG)
MASK = box_mask(8, 16, 40, 48)
MASK2 = box_mask(24, 0, 64, 40)


@pytest.fixture(scope="module")
def decoded(pipe):
    """The masked edit's decoded bytes (paste-back off) and its alpha paste-back, computed once."""
    return _edit(pipe, IMG, 5, mask_image=MASK, paste_back=False), _edit(pipe, IMG, 5, mask_image=MASK)


def test_all_ones_mask_is_the_unmasked_edit(pipe):
    ones = np.full((SIZE, SIZE), 255, np.uint8)
    assert np.array_equal(_edit(pipe, IMG, 6, mask_image=ones, **MB), _edit(pipe, IMG, 6))


def test_all_zeros_mask_returns_the_source(pipe):
    assert np.array_equal(_edit(pipe, IMG, 6, mask_image=np.zeros((SIZE, SIZE), np.uint8), **MB), SRC)


@pytest.mark.parametrize("levels", [4, 2])
def test_masked_edit_is_the_restatement_of_the_decoded_bytes(pipe, decoded, levels):
    out = _edit(pipe, IMG, 5, mask_image=MASK, blend_levels=levels, **MB)
    B = mbo.multiband(decoded[0], SRC, MASK, levels)
    assert np.array_equal(out[MASK == 0], SRC[MASK == 0])
    assert np.array_equal(out[MASK > 0], B[MASK > 0])
    assert not np.array_equal(out[MASK > 0], decoded[1][MASK > 0])       # it is not the alpha paste-back
    # feathered: blend_u8 over the job's mask_px with B where the decoded value stood; where the feather is 0 the source's bytes
    from fie_amd import mask as hmask
    soft = _edit(pipe, IMG, 5, mask_image=MASK, mask_blur=1.0, blend_levels=levels, **MB)
    alpha = pipe.ctx.mask_prep(_dev(pipe.ctx, MASK), 1.0)[0].cpu().numpy()
    assert np.array_equal(soft, mbo.multiband(decoded[0], SRC, MASK, levels, alpha=alpha))
    outside = hmask.feather_numpy(MASK >= 128, 1.0) == 0
    assert outside.any() and np.array_equal(alpha == 0, outside) and np.array_equal(soft[outside], SRC[outside])


def test_argument_rules_at_the_pipeline(pipe, decoded):
    ctl = _ctrl(IMG)
    with pytest.raises(ValueError, match="needs a mask"):
        pipe.prepare("p", "", IMG, ctl, **MB)
    with pytest.raises(ValueError, match="paste_back=True"):
        pipe.prepare("p", "", IMG, ctl, mask_image=MASK, paste_back=False, **MB)
    with pytest.raises(ValueError, match="'multiband'"):
        pipe.prepare("p", "", IMG, ctl, mask_image=MASK, blend="poisson")
    with pytest.raises(ValueError, match="blend_levels"):
        pipe.prepare("p", "", IMG, ctl, mask_image=MASK, blend_levels=7, **MB)
    # "alpha" spelled out is the default: the same job entries, the same bytes
    keys = set(pipe.prepare("p", "", IMG, ctl, mask_image=MASK, blend="alpha", blend_levels=2))
    assert keys == set(pipe.prepare("p", "", IMG, ctl, mask_image=MASK)) and not {"blend", "blend_l"} & keys
    assert np.array_equal(_edit(pipe, IMG, 5, mask_image=MASK, blend="alpha"), decoded[1])
    # the source-size path's job: paste-back off, the caller composites later -- B itself, uncomposited
    raw = _edit(pipe, IMG, 5, mask_image=MASK, paste_back=False, paste_later=True, **MB)
    assert np.array_equal(raw, mbo.multiband(decoded[0], SRC, MASK, 4))
    from fie_amd import cabi
    with pytest.raises(NotImplementedError, match="multiband"):
        cabi.run_edit(pipe, pipe.prepare("p", "", IMG, ctl, mask_image=MASK, **MB))


def test_graph_replay_matches_eager_and_takes_the_new_mask(pipe):
    eager = [_edit(pipe, IMG, 3, mask_image=m, mask_blur=1.0, **MB) for m in (MASK, MASK2)]
    n_graphs = len(pipe._graphs)
    graph = [_edit(pipe, IMG, 3, graph=True, mask_image=m, mask_blur=1.0, **MB) for m in (MASK, MASK2)]
    assert len(pipe._graphs) == n_graphs + 1                            # one graph, replayed with the second mask
    assert any(isinstance(k[0][-1], tuple) and k[0][-1] == (True, 1.0, True, ("multiband", 4)) for k in pipe._graphs)
    assert not np.array_equal(eager[0], eager[1])
    for a, b in zip(eager, graph):
        assert np.array_equal(a, b)
    _edit(pipe, IMG, 3, graph=True, mask_image=MASK, mask_blur=1.0, blend_levels=3, **MB)
    assert len(pipe._graphs) == n_graphs + 2                            # the level count is part of the key


def test_alpha_graph_key_is_unchanged(pipe):
    _edit(pipe, IMG, 3, graph=True, mask_image=MASK, blend="alpha")
    masked = [k[0][-1] for k in pipe._graphs if isinstance(k[0][-1], tuple) and k[0][-1][0] is True]
    assert (True, 0.0, True) in masked                                  # (masked, mask_blur, paste_back): no blend in an "alpha" key


def test_batch_with_a_masked_and_an_unmasked_image(pipe):
    """Image 0 of the batch is the restatement applied to the batch's own decoded bytes and image 1 is its decoded bytes, bit for bit; the batch's
    decoded bytes are the serial ones up to the fp16 tiling effects of the batched UNet (<= 2 levels, the bound of
    test_masked_edit_gpu.py::test_edit_batch_with_masks_matches_serial), which is all that separates the batch from the serial edits."""
    imgs = [IMG, synth_image(32)]
    ctls = [_ctrl(im) for im in imgs]
    prompts = ["a [red] circle", "a [toy] boat"]
    gens = lambda: [torch.Generator("cpu").manual_seed(11) for _ in imgs]
    run = lambda **kw: [np.asarray(o) for o in pipe(prompt=prompts, negative_prompt=["", ""], image=imgs, control_image=ctls, generator=gens(),
                                                    mask_image=[MASK, None], **dict(KW, **kw)).images]
    pipe.use_graph = False
    try:
        raw = run(paste_back=False)
        batch = run(**MB)
        serial_raw = [np.asarray(pipe(prompt=p, negative_prompt="", image=im, control_image=c, generator=g, mask_image=m, paste_back=False,
                                      **KW).images[0]) for p, im, c, g, m in zip(prompts, imgs, ctls, gens(), [MASK, None])]
        serial = [np.asarray(pipe(prompt=p, negative_prompt="", image=im, control_image=c, generator=g, mask_image=m,
                                  **dict(KW, **(MB if m is not None else {}))).images[0])
                  for p, im, c, g, m in zip(prompts, imgs, ctls, gens(), [MASK, None])]
    finally:
        pipe.use_graph = True
    B = mbo.multiband(raw[0], SRC, MASK, 4)
    assert np.array_equal(batch[0], np.where((MASK > 0)[..., None], B, SRC))
    assert np.array_equal(batch[1], raw[1])                             # no mask of its own: as without the keyword
    assert np.array_equal(serial[0], np.where((MASK > 0)[..., None], mbo.multiband(serial_raw[0], SRC, MASK, 4), SRC))
    assert np.array_equal(serial[1], serial_raw[1])
    for a, b in zip(serial_raw, raw):
        diff = np.abs(a.astype(int) - b.astype(int)).max()
        print(f"[multiband batch] decoded bytes, serial vs batch: max diff {diff}")
        assert diff <= 2


# ------------------------------------------------------------------------------------------------------------------------ the product surface
RES = (512, 512)


@pytest.fixture(scope="module")
def editor(fie):
    from src.pipeline import FastEditor
    return FastEditor(model_name="tiny", enable_cpu_offload=False)


def test_edit_at_the_sources_size(editor, fie):
    """output_size="source": the edit-size job returns B, and the existing full-resolution rule composites up(B) against the source as uploaded."""
    img = synth_image(51, 200).crop((0, 0, 200, 150))                   # 200 x 150
    mask = np.zeros((150, 200), np.uint8)
    mask[40:110, 60:140] = 255
    kw = dict(seed=9, strength=0.6, resolution=RES)
    out = editor.edit(img, "a [red] kite", mask=mask, mask_blur=2, output_size="source", blend="multiband", blend_levels=3, **kw)
    assert out.size == img.size
    d = np.asarray(editor.edit(img, "a [red] kite", mask=mask, paste_back=False, **kw))                 # the decoded bytes at the edit size
    S = np.asarray(img.resize(RES, Image.LANCZOS))
    mask_e = np.asarray(Image.fromarray(mask).resize(RES, Image.LANCZOS))
    B = mbo.multiband(d, S, mask_e, 3)
    want = fie.fullres_paste(_dev(fie, B), _dev(fie, np.asarray(img)), _dev(fie, mask), 2.0).cpu().numpy()
    assert np.array_equal(np.asarray(out), want)
    alpha_out = editor.edit(img, "a [red] kite", mask=mask, mask_blur=2, output_size="source", **kw)
    assert not np.array_equal(np.asarray(alpha_out), np.asarray(out))
    # at the edit size: the paste-back of B with the job's feathered mask
    edit_size = editor.edit(img, "a [red] kite", mask=mask, mask_blur=2, blend="multiband", blend_levels=3, **kw)
    alpha = fie.mask_prep(_dev(fie, mask_e), 2.0)[0].cpu().numpy()
    assert np.array_equal(np.asarray(edit_size), mbo.multiband(d, S, mask_e, 3, alpha=alpha))


def test_region_edit_with_metrics(editor):
    from fie_amd import region as hregion
    img = synth_image(41, 96).crop((0, 0, 96, 80))                      # 96 x 80
    mask = np.zeros((80, 96), np.uint8)
    mask[30:52, 40:66] = 255
    kw = dict(seed=8, strength=0.6, resolution=RES, mask_blur=1.0)
    out, scores = editor.edit(img, "an [empty] table", mask=mask, region="mask", region_padding=8, metrics=True, blend="multiband", **kw)
    l, t, r, b = hregion.resolve("mask", img.size, mask, 8, RES)
    src, got = np.asarray(img), np.asarray(out)
    outside = np.ones((80, 96), bool)
    outside[t:b, l:r] = False
    assert out.size == img.size and outside.any() and np.array_equal(got[outside], src[outside])
    assert {"ssim", "psnr", "mse", "bg_ssim", "bg_psnr", "bg_mse"} <= set(scores)
    assert not np.array_equal(got[mask >= 128], src[mask >= 128])
    plain = editor.edit(img, "an [empty] table", mask=mask, region="mask", region_padding=8, **kw)
    assert not np.array_equal(np.asarray(plain), got)


def test_edit_batch_leaves_the_unmasked_image_as_it_was(editor):
    imgs = [synth_image(42, 96), synth_image(43, 96)]
    prompts = ["a [toy] number 0", "a [toy] number 1"]
    mask = box_mask(20, 10, 70, 60, 96)
    kw = dict(seed=11, strength=0.5, resolution=RES)
    plain = [np.asarray(o) for o in editor.edit_batch(imgs, prompts, masks=[mask, None], **kw)]
    batch = [np.asarray(o) for o in editor.edit_batch(imgs, prompts, masks=[mask, None], blend="multiband", **kw)]
    assert np.array_equal(batch[1], plain[1])                           # same batch, same kernels: the unmasked image's bytes do not move
    mask_e = np.asarray(Image.fromarray(mask).resize(RES, Image.LANCZOS)) >= 128
    assert np.array_equal(batch[0][~mask_e], plain[0][~mask_e]) and not np.array_equal(batch[0][mask_e], plain[0][mask_e])
