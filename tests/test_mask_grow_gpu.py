"""`mask_grow` on the device: fie_mask_grow_u8 byte for byte against the numpy restatement (tests/mask_grow_oracle.py), and
the one identity every layer above it is held to -- a call with `mask_grow=r` returns exactly what the call with the grown mask passed in
returns -- on the pipeline object (tiny stack, 64x64) and on FastEditor (every comparison a bit equality)."""
import numpy as np
import pytest
import torch
from PIL import Image

import mask_grow_oracle as mgo
from isolation import flat, isolated
from multiband_oracle import blob_mask

pytestmark = pytest.mark.gpu

KW = dict(strength=0.8, num_inference_steps=4, guidance_scale=1.5, controlnet_conditioning_scale=0.5)
# 1: the plus shape; 5: lattice points exactly on the circle; 64: the halo bound, larger than several of the images
RADII = (1, -1, 2, -2, 3, -3, 5, -5, 16, -16, 64, -64)


def _dev(fie, a):
    return torch.from_numpy(np.array(a, order="C")).to(fie.device)                 # a writable copy (PIL arrays are read-only)


def _masks(h, w):
    return {"empty": np.zeros((h, w), np.uint8), "full": np.full((h, w), 255, np.uint8), "points": mgo.points_mask(h, w),
            "sparse": mgo.random_mask(h, w, 0.002, 7 * h + w),           # isolated disks that straddle tile seams
            "dense": mgo.random_mask(h, w, 0.998, 11 * h + w),           # the same for erosion
            "blob": blob_mask(h, w, w), "ramp": mgo.grey_ramp(h, w)}


# ------------------------------------------------------------------------------------------------------------------------ the op
# 1x1: one pixel, the tile almost all outside; 5x7: odd sides below one tile; 33x130: an odd side across three tiles; 72x88 and 200x136:
# partial tiles on both axes, 2 x 2 and 4 x 3 tiles; 70x333: six tiles and their halos in a row, two rows of tiles
@pytest.mark.parametrize("h,w", [(1, 1), (5, 7), (33, 130), (72, 88), (200, 136), (70, 333)])
def test_op_matches_the_restatement(fie, h, w):
    for name, mask in _masks(h, w).items():
        m_dev = _dev(fie, mask)
        for r in RADII:
            out = torch.full((h, w), 0x5A, dtype=torch.uint8, device=fie.device)
            got = fie.mask_grow(m_dev, r, out=out)
            assert got is out
            bad = np.argwhere(got.cpu().numpy() != mgo.grow(mask, r))
            assert bad.size == 0, (name, r, len(bad), bad[:4].tolist())
        assert np.array_equal(fie.mask_grow(m_dev, 5).cpu().numpy(), mgo.grow(mask, 5)), name          # an output of its own
        assert np.array_equal(fie.mask_grow(m_dev, 0).cpu().numpy(), (mask >= 128).astype(np.uint8) * 255), name        # the entry at 0: binarised
        assert np.array_equal(m_dev.cpu().numpy(), mask), name                                         # the operand is unchanged


@pytest.mark.parametrize("h,w", [(33, 130), (70, 333)])
def test_op_stays_inside_its_operands(fie, h, w):
    """Both tensors inside guard bands (tests/isolation.py): the mask's moat is 0xff -- set -- in one run and 0 in the other, so a read one byte
    outside it changes the result, and a store outside the output is found in its arena."""
    masks = _masks(h, w)
    for name in ("sparse", "dense", "blob"):
        for r in (3, -3, 64, -64):
            got = isolated(lambda i, o: fie.mask_grow(i["m"], r, out=o), {"m": flat(_dev(fie, masks[name]))},
                           dict(shape=(h, w), dtype=torch.uint8, flat=True))
            assert np.array_equal(got.cpu().numpy(), mgo.grow(masks[name], r)), (name, r)


def test_op_refuses_bad_arguments(fie):
    from fie_amd import hip
    m = _dev(fie, blob_mask(24, 40, 2))
    for r in (65, -65):
        with pytest.raises(hip.FieError):
            fie.mask_grow(m, r)
    with pytest.raises(ValueError):
        fie.mask_grow(m, 2, out=m)                                       # in place would race the halo reads
    with pytest.raises(ValueError):
        fie.mask_grow(m, 2, out=torch.empty((24, 39), dtype=torch.uint8, device=fie.device))
    with pytest.raises(ValueError):
        fie.mask_grow(m.float(), 2)
    with pytest.raises(ValueError):
        fie.mask_grow(m[:, :39], 2)                                      # not contiguous
    with pytest.raises(ValueError):
        fie.mask_grow(m, 1.5)
    flat2 = torch.zeros(2 * 24 * 40 - 8, dtype=torch.uint8, device=fie.device)
    with pytest.raises(hip.FieError):                                    # a partial overlap is refused by the entry itself
        fie.mask_grow(flat2[:960].view(24, 40), 2, out=flat2[952:1912].view(24, 40))


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
MASK = box_mask(12, 20, 36, 44)
MASK[22:30, 36:41] = 200                                                   # not a rectangle, not only 0 / 255
MASK2 = box_mask(24, 4, 60, 36)


@pytest.mark.parametrize("r", [3, -3])
def test_pipeline_call_is_the_call_with_the_grown_mask(pipe, r):
    grown = mgo.grow(MASK, r)
    assert not np.array_equal(grown, (MASK >= 128) * 255)
    want = _edit(pipe, IMG, 5, mask_image=grown)
    assert not np.array_equal(want, _edit(pipe, IMG, 5, mask_image=MASK))
    assert np.array_equal(_edit(pipe, IMG, 5, mask_image=MASK, mask_grow=r), want)                     # eager
    assert np.array_equal(_edit(pipe, IMG, 5, graph=True, mask_image=MASK, mask_grow=r), want)         # capture + replay
    assert np.array_equal(_edit(pipe, IMG, 5, graph=True, mask_image=_dev(pipe.ctx, MASK), mask_grow=r), want)       # a device tensor


def test_replay_takes_another_radius_and_another_mask_under_the_same_key(pipe):
    _edit(pipe, IMG, 3, graph=True, mask_image=MASK)
    keys = set(pipe._graphs)
    masked = [k[0][-1] for k in keys if isinstance(k[0][-1], tuple) and k[0][-1][0] is True]
    assert (True, 0.0, True) in masked                                  # (masked, mask_blur, paste_back): what it was
    for m, r in ((MASK, 2), (MASK, -4), (MASK2, 5), (MASK2, 2)):
        assert np.array_equal(_edit(pipe, IMG, 3, graph=True, mask_image=m, mask_grow=r), _edit(pipe, IMG, 3, mask_image=mgo.grow(m, r))), r
    assert set(pipe._graphs) == keys                                    # the grow runs in front of the graph: no new key, no new capture


def test_grow_0_launches_nothing_and_passes_greys_on(pipe, monkeypatch):
    grey = MASK.copy()
    grey[20:44, 12:20] = 130
    grey[0:8, 0:8] = 120
    want = _edit(pipe, IMG, 5, mask_image=grey, mask_blur=1.0)

    def boom(*a, **k):
        raise AssertionError("mask_grow=0 must not reach the op")
    monkeypatch.setattr(type(pipe.ctx), "mask_grow", boom)
    assert np.array_equal(_edit(pipe, IMG, 5, mask_image=grey, mask_blur=1.0, mask_grow=0), want)
    job = pipe.prepare("p", "", IMG, _ctrl(IMG), mask_image=grey, masked_content="fill", mask_grow=0)
    assert np.array_equal(job["mask_l"][0].cpu().numpy(), grey)         # untouched, greys included
    with pytest.raises(AssertionError, match="must not reach"):
        pipe.prepare("p", "", IMG, _ctrl(IMG), mask_image=grey, mask_grow=1)


def test_argument_rules_at_the_pipeline(pipe):
    ctl = _ctrl(IMG)
    with pytest.raises(ValueError, match="needs a mask"):
        pipe.prepare("p", "", IMG, ctl, mask_grow=2)
    for bad in (65, -65, 2.0, True):
        with pytest.raises(ValueError, match="mask_grow"):
            pipe.prepare("p", "", IMG, ctl, mask_image=MASK, mask_grow=bad)
    with pytest.raises(ValueError, match="needs a mask"):
        pipe.prepare_batch(["p", "q"], None, [IMG, IMG], [ctl, ctl], mask_image=[None, None], mask_grow=2)
    job = pipe.prepare("p", "", IMG, ctl, mask_image=MASK, masked_content="fill", blend="multiband", mask_grow=4)
    grown = mgo.grow(MASK, 4)
    assert np.array_equal(job["mask_l"][0].cpu().numpy(), grown) and np.array_equal(job["blend_l"][0].cpu().numpy(), grown)
    assert np.array_equal(job["mask_px"][0].cpu().numpy(), (grown > 0).astype(np.float32))
    assert np.array_equal(job["mask_lat"][0].cpu().numpy().reshape(8, 8), grown[::8, ::8] // 255)


@pytest.mark.parametrize("kw", [dict(masked_content="fill"), dict(blend="multiband", mask_blur=1.0)], ids=["fill", "multiband"])
def test_fill_and_multiband_see_the_grown_mask(pipe, kw):
    want = _edit(pipe, IMG, 5, mask_image=mgo.grow(MASK, 4), **kw)
    assert not np.array_equal(want, _edit(pipe, IMG, 5, mask_image=MASK, **kw))
    assert np.array_equal(_edit(pipe, IMG, 5, mask_image=MASK, mask_grow=4, **kw), want)


def test_batch_with_a_masked_and_an_unmasked_image(pipe):
    imgs = [IMG, synth_image(32)]
    ctls = [_ctrl(im) for im in imgs]
    gens = lambda: [torch.Generator("cpu").manual_seed(11) for _ in imgs]
    run = lambda masks, **kw: [np.asarray(o) for o in pipe(prompt=["a [red] circle", "a [toy] boat"], negative_prompt=["", ""], image=imgs,
                                                           control_image=ctls, generator=gens(), mask_image=masks, **dict(KW, **kw)).images]
    pipe.use_graph = False
    try:
        plain = run([MASK, None])
        got = run([MASK, None], mask_grow=-3)
        want = run([mgo.grow(MASK, -3), None])
    finally:
        pipe.use_graph = True
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    assert np.array_equal(got[1], plain[1]) and not np.array_equal(got[0], plain[0])                   # no mask of its own: untouched


# ------------------------------------------------------------------------------------------------------------------------ the product surface
RES = (512, 512)


@pytest.fixture(scope="module")
def editor(fie):
    from src.pipeline import FastEditor
    return FastEditor(model_name="tiny", enable_cpu_offload=False)


def test_edit_at_the_sources_size(editor):
    img = synth_image(51, 200).crop((0, 0, 200, 150))                   # 200 x 150
    mask = np.zeros((150, 200), np.uint8)
    mask[40:110, 60:140] = 255
    mask[60:70, 140:150] = 255
    kw = dict(seed=9, strength=0.6, resolution=RES, output_size="source", mask_blur=2)
    got = editor.edit(img, "a [red] kite", mask=mask, mask_grow=4, **kw)
    want = editor.edit(img, "a [red] kite", mask=mgo.grow(mask, 4), **kw)
    assert got.size == img.size and np.array_equal(np.asarray(got), np.asarray(want))
    assert not np.array_equal(np.asarray(got), np.asarray(editor.edit(img, "a [red] kite", mask=mask, **kw)))


def test_region_mask_takes_its_box_from_the_grown_mask(editor):
    from fie_amd import region as hregion
    img = synth_image(41, 96).crop((0, 0, 96, 80))                      # 96 x 80
    mask = np.zeros((80, 96), np.uint8)
    mask[30:52, 40:66] = 255
    grown = mgo.grow(mask, 6)
    kw = dict(seed=8, strength=0.6, resolution=RES, mask_blur=1.0, region="mask", region_padding=8, metrics=True)
    got, scores = editor.edit(img, "an [empty] table", mask=mask, mask_grow=6, **kw)
    want, want_scores = editor.edit(img, "an [empty] table", mask=grown, **kw)
    assert np.array_equal(np.asarray(got), np.asarray(want)) and scores == want_scores
    assert {"ssim", "psnr", "mse", "bg_ssim", "bg_psnr", "bg_mse"} <= set(scores)
    box = hregion.resolve("mask", img.size, grown, 8, RES)
    assert box != hregion.resolve("mask", img.size, mask, 8, RES)
    l, t, r, b = box
    outside = np.ones((80, 96), bool)
    outside[t:b, l:r] = False
    assert outside.any() and np.array_equal(np.asarray(got)[outside], np.asarray(img)[outside])
    assert not np.array_equal(np.asarray(got)[grown > 0], np.asarray(img)[grown > 0])


def test_an_explicit_region_is_cropped_after_the_mask_has_grown(editor):
    img = synth_image(44, 96).crop((0, 0, 96, 80))
    box = (30, 20, 70, 60)
    mask = np.zeros((80, 96), np.uint8)
    mask[30:50, 44:60] = 255                                             # inside the box
    mask[38:48, 27:30] = 255                                             # a strip 1 .. 3 pixels outside its left edge
    cut = lambda a: a[box[1]:box[3], box[0]:box[2]]
    grown = mgo.grow(mask, 5)
    assert not np.array_equal(cut(grown), mgo.grow(cut(mask), 5))        # crop-then-grow would miss what reaches in from outside
    kw = dict(seed=4, strength=0.6, resolution=RES, region=box)
    got = np.asarray(editor.edit(img, "a [blue] door", mask=mask, mask_grow=5, **kw))
    assert np.array_equal(got, np.asarray(editor.edit(img, "a [blue] door", mask=grown, **kw)))
    assert not np.array_equal(got, np.asarray(editor.edit(img, "a [blue] door", mask=mask, **kw)))
    reached = grown > 0
    reached[:, 35:] = False
    reached[:, :30] = False                                              # columns 30 .. 34 of the box: selected only through the strip
    assert reached.any() and not np.array_equal(got[reached], np.asarray(img)[reached])


def test_edit_batch_with_regions_and_an_unmasked_image(editor):
    imgs = [synth_image(42, 96), synth_image(43, 96)]
    prompts = ["a [toy] number 0", "a [toy] number 1"]
    mask = box_mask(30, 20, 60, 52, 96)
    kw = dict(seed=11, strength=0.5, resolution=RES, region=["mask", None], region_padding=8)
    got = [np.asarray(o) for o in editor.edit_batch(imgs, prompts, masks=[mask, None], mask_grow=7, **kw)]
    want = [np.asarray(o) for o in editor.edit_batch(imgs, prompts, masks=[mgo.grow(mask, 7), None], **kw)]
    plain = [np.asarray(o) for o in editor.edit_batch(imgs, prompts, masks=[mask, None], **kw)]
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    assert not np.array_equal(got[0], plain[0])
    # without regions: one device job, the unmasked image's bytes do not move
    kw = dict(seed=11, strength=0.5, resolution=RES)
    got = [np.asarray(o) for o in editor.edit_batch(imgs, prompts, masks=[mask, None], mask_grow=7, **kw)]
    want = [np.asarray(o) for o in editor.edit_batch(imgs, prompts, masks=[mgo.grow(mask, 7), None], **kw)]
    plain = [np.asarray(o) for o in editor.edit_batch(imgs, prompts, masks=[mask, None], **kw)]
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]) and np.array_equal(got[1], plain[1])
    assert not np.array_equal(got[0], plain[0])


def test_a_mask_eroded_to_nothing_returns_the_source(editor):
    img = synth_image(45, 512)
    mask = box_mask(200, 240, 230, 270, 512)                            # 30 x 30
    assert not mgo.grow(mask, -20).any()
    out = editor.edit(img, "a [green] leaf", mask=mask, mask_grow=-20, seed=3, strength=0.6, resolution=RES)
    assert np.array_equal(np.asarray(out), np.asarray(img))
