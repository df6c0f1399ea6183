"""Soft masks on the device: fie_lcm_step_levels against fie_lcm_step (inside, bit for bit) and the closed form (outside),
fie_mask_ramp_u8 / fie_mask_levels_u8 / fie_mask_support_u8 byte for byte against the restatements of fie_amd/mask.py, a levels edit against the
levels oracle, the exact pins that tie it to the masked and the unmasked edit, and the product surfaces (batch, sweep, source-size output,
region, tiles)."""
import numpy as np
import pytest
import torch
from PIL import Image

import levels_oracle
import mask_grow_oracle as mgo
from isolation import flat, isolated
from multiband_oracle import blob_mask

pytestmark = pytest.mark.gpu

KW = dict(strength=0.8, num_inference_steps=4, guidance_scale=1.5, controlnet_conditioning_scale=0.5)
SPECIAL = (0, 1, 84, 85, 86, 127, 128, 170, 171, 254, 255)             # 85 and 170 sit exactly on v K = 255 (K - 1 - j) for K = 3


def _dev(fie, a):
    return torch.from_numpy(np.array(a, order="C")).to(fie.device)


# ------------------------------------------------------------------------------------------------------------------------ the step kernel
@pytest.mark.parametrize("dtype", [torch.float16, torch.float32])
@pytest.mark.parametrize("nb", [1, 2])
@pytest.mark.parametrize("last", [False, True])
def test_lcm_step_levels(fie, dtype, nb, last):
    from fie_amd import hip, mask as hmask
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
    lv = torch.randint(0, 256, (hw,), generator=g, dtype=torch.uint8)
    lv[:4 * len(SPECIAL)] = torch.tensor(SPECIAL * 4, dtype=torch.uint8)
    lv = lv[torch.randperm(hw, generator=g)]
    sc = dict(sab_t=0.35, s1mab_t=0.937, c_skip=0.002, c_out=0.998, sab_p=0.62, s1mab_p=0.785)

    def run(fn, *tail):
        lat = lat0.clone()
        model_in = torch.zeros((nb, lh, lw, 8), device=dev, dtype=dtype)
        dec = torch.zeros((1, lh, lw, 8), device=dev, dtype=dtype)
        fn(eps, nb, 1.7, lat, noise, hw, sc["sab_t"], sc["s1mab_t"], sc["c_skip"], sc["c_out"], sc["sab_p"], sc["s1mab_p"], model_in, 0.13, dec, *tail)
        torch.cuda.synchronize()
        return lat.cpu(), model_in.cpu(), dec.cpu()

    plain = run(ctx.lcm_step)
    # the numpy closed form of the whole step, as tests/test_masked_edit_gpu.py states it
    e = eps.float().cpu().numpy().reshape(nb, hw, 8)[..., :4].astype(np.float64)
    e = e[0] + 1.7 * (e[1] - e[0]) if nb == 2 else e[0]
    x = lat0.cpu().numpy().astype(np.float64)
    den = sc["c_out"] * (x - sc["s1mab_t"] * e) / sc["sab_t"] + sc["c_skip"] * x
    z = z0.cpu().numpy().astype(np.float64)
    if not last:
        den = sc["sab_p"] * den + sc["s1mab_p"] * noise.cpu().numpy().T
        proper = sc["sab_p"] * z + sc["s1mab_p"] * n_init.cpu().numpy().T
    else:
        proper = z
    lv_dev = lv.to(dev)
    seen = set()
    for K in (1, 2, 3, 4, 8):
        for j in range(K):
            inside = np.array([hmask.level_inside(int(v), K, j) for v in lv])
            seen.add(int(inside.sum()))
            lat, model_in, dec = run(ctx.lcm_step_levels, lv_dev, z0, n_init, K, j)
            assert torch.equal(lat[torch.from_numpy(inside)], plain[0][torch.from_numpy(inside)]), (K, j)    # inside: the unmasked step's bits
            assert np.allclose(lat.numpy(), np.where(inside[:, None], den, proper), rtol=1e-5, atol=1e-5), (K, j)
            mi = model_in.float().numpy().reshape(nb, hw, 8)
            for k in range(nb):
                assert np.array_equal(mi[k, :, :4], lat.numpy().astype(np.float16 if dtype == torch.float16 else np.float32).astype(np.float32))
                assert not mi[k, :, 4:].any()
            assert np.allclose(dec.float().numpy().reshape(hw, 8)[:, :4], lat.numpy() * 0.13, rtol=2e-3 if dtype == torch.float16 else 1e-6, atol=1e-6)
            # the binary entry on the same inside set: every output bit for bit -- it is the special case "levels 0 / 1, K = 1, j = 0"
            m01 = torch.from_numpy(inside.astype(np.uint8)).to(dev)
            old = run(ctx.lcm_step_masked, m01, z0, n_init)
            assert all(torch.equal(a, b) for a, b in zip(old, (lat, model_in, dec))), (K, j)
            assert all(torch.equal(a, b) for a, b in zip(old, run(ctx.lcm_step_levels, m01, z0, n_init, 1, 0))), (K, j)
    assert len(seen) > 8                                                 # the thresholds really moved
    # 85 and 170 on the boundary of K = 3: strictly greater decides
    assert not hmask.level_inside(85, 3, 1) and hmask.level_inside(86, 3, 1) and not hmask.level_inside(170, 3, 0) and hmask.level_inside(171, 3, 0)
    for steps, step in ((0, 0), (256, 0), (3, 3), (3, -1), (1, 1)):
        with pytest.raises(hip.FieError, match="step"):
            run(ctx.lcm_step_levels, lv_dev, z0, n_init, steps, step)


# ------------------------------------------------------------------------------------------------------------------------ the mask ops
RADII = (1, 2, 7, 33, 64)


def _masks(h, w):
    return {"empty": np.zeros((h, w), np.uint8), "full": np.full((h, w), 255, np.uint8), "points": 255 - mgo.points_mask(h, w),
            "sparse": mgo.random_mask(h, w, 0.002, 7 * h + w),           # isolated set pixels: level 255 // r each
            "dense": mgo.random_mask(h, w, 0.998, 11 * h + w),           # isolated holes whose ramps straddle tile seams
            "blob": blob_mask(h, w, w), "ramp": mgo.grey_ramp(h, w)}


# the shapes of tests/test_mask_grow_gpu.py: one pixel; odd sides below one tile; an odd side across three tiles; partial tiles on both axes;
# six tiles and their halos in a row
@pytest.mark.parametrize("h,w", [(1, 1), (5, 7), (33, 130), (72, 88), (200, 136), (70, 333)])
def test_ramp_matches_the_restatement(fie, h, w):
    from fie_amd import mask as hmask
    for name, mask in _masks(h, w).items():
        m_dev = _dev(fie, mask)
        for r in RADII:
            out = torch.full((h, w), 0x5A, dtype=torch.uint8, device=fie.device)
            got = fie.mask_ramp(m_dev, r, out=out)
            assert got is out
            want = hmask.ramp_numpy(mask, r)
            bad = np.argwhere(got.cpu().numpy() != want)
            assert bad.size == 0, (name, r, len(bad), bad[:4].tolist())
            assert np.array_equal(fie.mask_support(got).cpu().numpy(), (mask >= 128).astype(np.uint8) * 255), (name, r)
        assert np.array_equal(fie.mask_ramp(m_dev, 5).cpu().numpy(), hmask.ramp_numpy(mask, 5)), name       # an output of its own
        assert np.array_equal(m_dev.cpu().numpy(), mask), name                                             # the operand is unchanged


def test_mask_levels_and_support_match_the_restatements(fie):
    from fie_amd import mask as hmask
    rng = np.random.default_rng(9)
    h, w = 64, 72
    v = rng.integers(0, 256, (h, w), dtype=np.uint8)
    v[rng.random((h, w)) < 0.3] = 0
    v[::8, ::8][rng.random((8, 9)) < 0.3] = 0                            # zeros on the latent grid too
    s = hmask.support_numpy(v)
    assert np.array_equal(fie.mask_support(_dev(fie, v)).cpu().numpy(), s)
    for m_lat in ((s[::8, ::8] >= 128).astype(np.uint8), np.ones((8, 9), np.uint8), (rng.random((8, 9)) < 0.5).astype(np.uint8)):
        got = fie.mask_levels(_dev(fie, v), _dev(fie, m_lat.reshape(-1)))
        assert got.shape == (72,) and np.array_equal(got.cpu().numpy().reshape(8, 9), hmask.levels_lat_numpy(v, m_lat))
    _, lat = fie.mask_prep(_dev(fie, s), 0.0)                            # the pipeline's chain: the latent support is mask_prep's, bit for bit
    lvl = fie.mask_levels(_dev(fie, v), lat).cpu().numpy()
    assert np.array_equal(lvl > 0, lat.cpu().numpy() > 0) and np.array_equal(lvl.reshape(8, 9), levels_oracle.lat_levels(v)[1])


@pytest.mark.parametrize("h,w", [(33, 130), (70, 333)])
def test_ramp_stays_inside_its_operands(fie, h, w):
    """Both tensors inside guard bands (tests/isolation.py): the mask's moat is 0xff in one run and 0 -- an unset pixel -- in the other, so a read
    one byte outside the mask changes the distances, and a store outside the output is found in its arena."""
    from fie_amd import mask as hmask
    masks = _masks(h, w)
    for name in ("full", "dense", "blob"):
        for r in (3, 64):
            got = isolated(lambda i, o: fie.mask_ramp(i["m"], r, out=o), {"m": flat(_dev(fie, masks[name]))},
                           dict(shape=(h, w), dtype=torch.uint8, flat=True))
            assert np.array_equal(got.cpu().numpy(), hmask.ramp_numpy(masks[name], r)), (name, r)


def test_mask_levels_stays_inside_its_operands(fie):
    from fie_amd import mask as hmask
    rng = np.random.default_rng(3)
    v = rng.integers(0, 256, (64, 72), dtype=np.uint8)
    m_lat = (rng.random(72) < 0.7).astype(np.uint8)
    got = isolated(lambda i, o: fie.mask_levels(i["v"], i["m"], out=o), {"v": flat(_dev(fie, v)), "m": flat(_dev(fie, m_lat))},
                   dict(shape=(72,), dtype=torch.uint8, flat=True))
    assert np.array_equal(got.cpu().numpy().reshape(8, 9), hmask.levels_lat_numpy(v, m_lat))
    got = isolated(lambda i, o: fie.mask_support(i["v"], out=o), {"v": flat(_dev(fie, v))}, dict(shape=(64, 72), dtype=torch.uint8, flat=True))
    assert np.array_equal(got.cpu().numpy(), hmask.support_numpy(v))


def test_ops_refuse_bad_arguments(fie):
    from fie_amd import hip
    m = _dev(fie, blob_mask(24, 40, 2))
    for r in (0, 65, -3):
        with pytest.raises(hip.FieError, match="radius"):
            fie.mask_ramp(m, r)
    with pytest.raises(ValueError):
        fie.mask_ramp(m, 2, out=m)                                       # in place would race the halo reads
    with pytest.raises(ValueError):
        fie.mask_ramp(m, 2, out=torch.empty((24, 39), dtype=torch.uint8, device=fie.device))
    with pytest.raises(ValueError):
        fie.mask_ramp(m.float(), 2)
    with pytest.raises(ValueError):
        fie.mask_ramp(m, 1.5)
    flat2 = torch.zeros(2 * 24 * 40 - 8, dtype=torch.uint8, device=fie.device)
    with pytest.raises(hip.FieError, match="overlaps"):                  # a partial overlap is refused by the entry itself
        fie.mask_ramp(flat2[:960].view(24, 40), 2, out=flat2[952:1912].view(24, 40))
    with pytest.raises(ValueError):
        fie.mask_levels(m[:, :36].contiguous(), torch.zeros(15, dtype=torch.uint8, device=fie.device))        # 36 is no multiple of 8
    with pytest.raises(ValueError):
        fie.mask_levels(m, torch.zeros(14, dtype=torch.uint8, device=fie.device))


# ------------------------------------------------------------------------------------------------------------------------ the pipeline, 128x128
def synth_image(seed, size):
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:size, 0:size].astype(np.float32) / size
    img = np.stack([0.5 + 0.4 * np.sin(6.0 * xx + rng.uniform(0, 6)) * np.cos(4.0 * yy + rng.uniform(0, 6)) for _ in range(3)], axis=2)
    for _ in range(6):
        cx, cy, r = rng.uniform(0.1, 0.9), rng.uniform(0.1, 0.9), rng.uniform(0.05, 0.2)
        img[((xx - cx) ** 2 + (yy - cy) ** 2) < r * r] = rng.uniform(0, 1, 3)
    return Image.fromarray((img.clip(0, 1) * 255).astype(np.uint8))


def gradient_map(size=128):
    """Zero except rows 16..112 and columns 8..120, which hold a left-to-right gradient 1..255."""
    v = np.zeros((size, size), np.uint8)
    v[16:112, 8:120] = np.rint(np.linspace(1, 255, 112)).astype(np.uint8)[None, :]
    return v


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


def _edit(pipe, img, seed, graph=False, **kw):
    pipe.use_graph = graph
    try:
        return np.asarray(pipe(prompt="a [red] circle", negative_prompt="", image=img, control_image=_ctrl(img),
                               generator=torch.Generator("cpu").manual_seed(seed), **dict(KW, **kw)).images[0])
    finally:
        pipe.use_graph = True


IMG = synth_image(11, 128)
SRC = np.asarray(IMG)
V = gradient_map()
GREY = box_mask(128, 24, 40, 96, 104)
GREY[40:104, 24:60] = 100                                               # half the box at level 100: n(100, 3) = 2 of 3 steps
GREY[48:64, 96:112] = 30                                                # and a patch below the binary threshold: in the support, not in L >= 128


@pytest.mark.parametrize("strength,guidance", [(0.5, 1.0), (0.8, 1.5), (1.0, 2.0)])
def test_levels_edit_vs_levels_oracle(rig, strength, guidance):
    from fie_amd import mask as hmask
    from oracle import metrics
    cfgs, sds32, pipe = rig
    K = len(pipe.scheduler.plan(4, strength))
    assert K == {0.5: 2, 0.8: 3, 1.0: 4}[strength]
    lvl = levels_oracle.lat_levels(V)[1]
    bands = np.bincount([hmask.level_steps(v, K) for v in lvl.reshape(-1)], minlength=K + 1)
    assert len(bands) == K + 1 and bands.min() >= 8, bands              # every n in 0 .. K occurs in at least 8 latent pixels
    kw = dict(strength=strength, num_inference_steps=4, guidance_scale=guidance, controlnet_conditioning_scale=0.5)
    out = _edit(pipe, IMG, 42, mask_image=V, mask_mode="levels", mask_blur=1.5, **kw)              # eager; test_exact_pins ties the replay to it
    ref = levels_oracle.run_levels(sds32, cfgs, IMG, _ctrl(IMG), _ids(pipe, ["a [red] circle"]), _ids(pipe, [""]), V, mask_blur=1.5,
                                   generator=torch.Generator("cpu").manual_seed(42), **kw)
    s = metrics.ssim(Image.fromarray(out), ref, size=None)
    print(f"levels edit vs levels oracle (K={K}): ssim={s:.5f}")
    assert s >= 0.99
    outside = hmask.feather_numpy((hmask.support_numpy(V) >= 128).astype(np.float32), 1.5) == 0
    assert outside.sum() > 2000 and np.array_equal(out[outside], SRC[outside])


def test_a_grey_map_is_not_its_binarisation(rig):
    """Fails without the feature: `mask_mode="levels"` is accepted, and the greys change the result."""
    from fie_amd import mask as hmask
    _, _, pipe = rig
    soft = _edit(pipe, IMG, 5, mask_image=GREY, mask_mode="levels")
    assert not np.array_equal(soft, _edit(pipe, IMG, 5, mask_image=GREY))                               # binarised at L >= 128, as ever
    assert not np.array_equal(soft, _edit(pipe, IMG, 5, mask_image=hmask.support_numpy(GREY)))          # nor the edit of its support
    outside = GREY == 0
    assert np.array_equal(soft[outside], SRC[outside])
    patch = (GREY == 30)
    assert not np.array_equal(soft[patch], SRC[patch])                  # level 30 is in the support: released on the last step


@pytest.mark.parametrize("graph", [False, True], ids=["eager", "replayed"])
def test_exact_pins(rig, graph):
    from fie_amd import mask as hmask
    _, _, pipe = rig
    runs = (0, 1) if graph else (0,)                                    # replayed: the capture's call, then a replay of it
    ones = np.full((128, 128), 255, np.uint8)
    base = _edit(pipe, IMG, 7, graph=graph)
    hard = box_mask(128, 24, 40, 96, 104)
    masked = _edit(pipe, IMG, 7, graph=graph, mask_image=hard)
    k1 = dict(strength=0.25)
    assert len(pipe.scheduler.plan(4, 0.25)) == 1 and len(pipe.scheduler.plan(4, 0.8)) == 3
    masked_k1 = _edit(pipe, IMG, 7, graph=graph, mask_image=hmask.support_numpy(GREY), **k1)
    for _ in runs:
        assert np.array_equal(_edit(pipe, IMG, 7, graph=graph, mask_image=ones, mask_mode="levels"), base)          # all 255: the unmasked edit
        assert np.array_equal(_edit(pipe, IMG, 7, graph=graph, mask_image=hard, mask_mode="levels"), masked)        # 0 / 255 at K = 3: the masked edit
        for v in (GREY, V):                                                                                       # K = 1: any map is its support
            want = masked_k1 if v is GREY else _edit(pipe, IMG, 7, graph=graph, mask_image=hmask.support_numpy(v), **k1)
            assert np.array_equal(_edit(pipe, IMG, 7, graph=graph, mask_image=v, mask_mode="levels", **k1), want)
    # where the latent level is 0 the final latents are the clean source latents, exactly
    with torch.cuda.stream(pipe.slot_stream(0)):                        # where the pipeline's own call prepares and runs a job
        job = pipe.prepare("a [red] circle", "", IMG, _ctrl(IMG), generator=torch.Generator("cpu").manual_seed(7), mask_image=V,
                           mask_mode="levels", **KW)
    for _ in runs:
        with torch.cuda.stream(pipe.slot_stream(0)):
            pipe.run_device_graphed(job) if graph else pipe._run_eager(job)
        torch.cuda.synchronize()
        lat, z0, lvl = job["_result"]["latents"][0].cpu(), job["_result"]["z0"][0].cpu(), job["lvl_lat"][0].cpu()
        assert np.array_equal(lvl.numpy().reshape(16, 16), levels_oracle.lat_levels(V)[1])
        assert (lvl == 0).sum() > 50 and torch.equal(lat[lvl == 0], z0[lvl == 0])
        assert not torch.equal(lat[lvl > 0], z0[lvl > 0])


def test_replay_takes_another_map_under_one_key(rig):
    _, _, pipe = rig
    maps = [GREY, V, box_mask(128, 0, 0, 64, 128, 140)]
    eager = [_edit(pipe, IMG, 3, mask_image=m, mask_mode="levels", mask_blur=2.0) for m in maps]
    assert len(pipe._graphs) < pipe.max_graphs
    n_graphs = len(pipe._graphs)
    keys = set(pipe._graphs)
    replayed = [_edit(pipe, IMG, 3, graph=True, mask_image=m, mask_mode="levels", mask_blur=2.0) for m in maps]
    assert len(pipe._graphs) == n_graphs + 1                            # one levels graph, replayed with the next maps
    (key,) = set(pipe._graphs) - keys
    assert key[0][-1] == (True, 2.0, True, "levels")                    # the masked key and one flag
    assert len({e.tobytes() for e in eager}) == 3
    for a, b in zip(eager, replayed):
        assert np.array_equal(a, b)
    _edit(pipe, IMG, 3, graph=True, mask_image=GREY, mask_blur=2.0)      # the binary masked key is what it was
    assert (True, 2.0, True) in [k[0][-1] for k in pipe._graphs]


def test_mask_ramp_is_the_levels_call_with_the_ramped_mask(rig):
    from fie_amd import mask as hmask
    _, _, pipe = rig
    mask = box_mask(128, 24, 40, 96, 104)
    mask[56:72, 96:120] = 200                                           # not a rectangle, not only 0 / 255
    ramped = hmask.ramp_numpy(mask, 5)
    want = _edit(pipe, IMG, 5, mask_image=ramped, mask_mode="levels", mask_blur=1.0)
    assert not np.array_equal(want, _edit(pipe, IMG, 5, mask_image=mask, mask_blur=1.0))
    for graph in (False, True):
        assert np.array_equal(_edit(pipe, IMG, 5, graph=graph, mask_image=mask, mask_ramp=5, mask_blur=1.0), want), graph
    assert np.array_equal(_edit(pipe, IMG, 5, mask_image=_dev(pipe.ctx, mask), mask_ramp=5, mask_blur=1.0), want)       # a device tensor
    grown = mgo.grow(mask, 3)
    want = _edit(pipe, IMG, 5, mask_image=hmask.ramp_numpy(grown, 5), mask_mode="levels")
    assert np.array_equal(_edit(pipe, IMG, 5, mask_image=mask, mask_grow=3, mask_ramp=5), want)                       # grown first, ramped second
    assert np.array_equal(_edit(pipe, IMG, 5, mask_image=grown, mask_ramp=5), want)
    job = pipe.prepare("p", "", IMG, _ctrl(IMG), mask_image=mask, mask_ramp=5, masked_content="fill", blend="multiband")
    support = (mask >= 128).astype(np.uint8) * 255                      # every other reader takes the support
    assert np.array_equal(job["mask_l"][0].cpu().numpy(), support) and np.array_equal(job["blend_l"][0].cpu().numpy(), support)
    assert np.array_equal(job["lvl_lat"][0].cpu().numpy().reshape(16, 16), levels_oracle.lat_levels(ramped)[1])


def test_argument_rules_and_the_cabi_walk(rig):
    from fie_amd import cabi
    _, _, pipe = rig
    ctl = _ctrl(IMG)
    with pytest.raises(ValueError, match="needs a mask"):
        pipe.prepare("p", "", IMG, ctl, mask_mode="levels")
    with pytest.raises(ValueError, match="needs a mask"):
        pipe.prepare_batch(["p", "q"], None, [IMG, IMG], [ctl, ctl], mask_image=[None, None], mask_ramp=2)
    with pytest.raises(ValueError, match="discard"):
        pipe.prepare("p", "", IMG, ctl, mask_image=GREY, mask_mode="levels", mask_ramp=2)
    with pytest.raises(ValueError, match="discard"):
        pipe.prepare("p", "", IMG, ctl, mask_image=GREY, mask_mode="levels", mask_grow=2)
    job = pipe.prepare("p", "", IMG, ctl, mask_image=GREY, mask_mode="levels")
    with pytest.raises(NotImplementedError, match="soft mask"):
        cabi.run_edit(pipe, job)
    assert "lvl_lat" not in pipe.prepare("p", "", IMG, ctl, mask_image=GREY)           # a binary masked job is what it was


def test_batch_with_a_levels_image_and_an_unmasked_image(rig):
    _, _, pipe = rig
    imgs = [IMG, synth_image(32, 128)]
    ctls = [_ctrl(im) for im in imgs]
    gens = lambda: [torch.Generator("cpu").manual_seed(11) for _ in imgs]
    run = lambda masks, **kw: [np.asarray(o) for o in pipe(prompt=["a [red] circle", "a [toy] boat"], negative_prompt=["", ""], image=imgs,
                                                           control_image=ctls, generator=gens(), mask_image=masks, **dict(KW, **kw)).images]
    pipe.use_graph = False
    try:
        plain = run([GREY, None])
        got = run([GREY, None], mask_mode="levels")
        ones = run([GREY, np.full((128, 128), 255, np.uint8)], mask_mode="levels")
    finally:
        pipe.use_graph = True
    assert np.array_equal(got[1], plain[1]) and not np.array_equal(got[0], plain[0])                   # no mask of its own: untouched
    assert np.array_equal(got[0], ones[0]) and np.array_equal(got[1], ones[1])


# ------------------------------------------------------------------------------------------------------------------------ the product surface
RES = (512, 512)


@pytest.fixture(scope="module")
def editor(fie):
    from src.pipeline import FastEditor
    return FastEditor(model_name="tiny", enable_cpu_offload=False)


def _soft(size, seed=0):
    """A level map with a 255 core, a grey rim and a faint halo below the binary threshold."""
    v = box_mask(size, size // 8, size // 6, size - size // 4, size - size // 5, 60)
    v[size // 4:size // 2 + size // 8, size // 4:size // 2] = 255
    v[size // 3:size // 2, size // 2:size // 2 + size // 6] = 150 + seed
    return v


def test_edit_batch_with_levels_matches_serial(editor):
    imgs = [synth_image(60 + i, 96) for i in range(3)]
    prompts = [f"a [toy] number {i}" for i in range(3)]
    masks = [_soft(96), None, Image.fromarray(_soft(96, 20))]
    kw = dict(seed=11, strength=0.8, resolution=RES)
    serial = [np.asarray(editor.edit(im, p, mask=m, **(dict(mask_mode="levels") if m is not None else {}), **kw)) for im, p, m in zip(imgs, prompts, masks)]
    batch = [np.asarray(o) for o in editor.edit_batch(imgs, prompts, masks=masks, mask_mode="levels", **kw)]
    for a, b in zip(serial, batch):
        assert a.shape == b.shape == (512, 512, 3)
        assert np.abs(a.astype(int) - b.astype(int)).max() <= 2
    assert not np.array_equal(serial[0], np.asarray(editor.edit(imgs[0], prompts[0], mask=masks[0], **kw)))
    src0 = np.asarray(imgs[0].resize(RES, Image.LANCZOS))
    m0 = np.asarray(Image.fromarray((masks[0] > 0).astype(np.uint8) * 255).resize(RES, Image.LANCZOS)) < 128       # outside the resized support
    assert np.array_equal(batch[0][m0], src0[m0])


def test_edit_sweep_with_levels_matches_serial_edits(editor):
    img = synth_image(64, 128)
    v = _soft(128)
    kw = dict(seed=5, resolution=RES, mask=v, mask_mode="levels")
    imgs, variants = editor.edit_sweep(img, "a [red] kite", strengths="all", **kw)
    assert [x["steps"] for x in variants] == [4, 3, 2, 1] and "bg_ssim" in variants[0]
    for im, var in zip(imgs, variants):
        want = np.asarray(editor.edit(img, "a [red] kite", strength=var["strength"][0], **kw))
        assert np.abs(np.asarray(im).astype(int) - want.astype(int)).max() <= 2, var["steps"]
    assert len({np.asarray(im).tobytes() for im in imgs}) == 4


def test_source_size_output_with_a_ramp(editor):
    img = synth_image(51, 200).crop((0, 0, 200, 152))                    # 200 x 152
    mask = np.zeros((152, 200), np.uint8)
    mask[40:110, 60:140] = 255
    mask[60:70, 140:150] = 255
    kw = dict(seed=9, strength=0.8, resolution=RES, output_size="source")
    got = np.asarray(editor.edit(img, "a [red] kite", mask=mask, mask_ramp=8, **kw))
    src = np.asarray(img)
    assert got.shape == src.shape and np.array_equal(got[mask == 0], src[mask == 0])                  # outside the mask: the caller's bytes
    assert not np.array_equal(got[mask > 0], src[mask > 0])
    assert not np.array_equal(got, np.asarray(editor.edit(img, "a [red] kite", mask=mask, **kw)))
    from fie_amd import mask as hmask
    assert np.array_equal(got, np.asarray(editor.edit(img, "a [red] kite", mask=hmask.ramp_numpy(mask, 8), mask_mode="levels", **kw)))


def test_region_mask_takes_its_box_from_the_support(editor):
    from fie_amd import mask as hmask, region as hregion
    img = synth_image(41, 96).crop((0, 0, 96, 80))                       # 96 x 80
    v = np.zeros((80, 96), np.uint8)
    v[30:52, 40:66] = 255
    v[24:30, 30:40] = 50                                                 # in the support, below the binary threshold
    kw = dict(seed=8, strength=0.8, resolution=RES, region_padding=4)
    box = hregion.resolve("mask", img.size, hmask.support_numpy(v), 4, RES)
    assert box != hregion.resolve("mask", img.size, v, 4, RES)
    got = np.asarray(editor.edit(img, "an [empty] table", mask=v, mask_mode="levels", region="mask", **kw))
    inner = editor.edit(img.crop(box), "an [empty] table", mask=v[box[1]:box[3], box[0]:box[2]], mask_mode="levels", output_size="source",
                        seed=8, strength=0.8, resolution=RES)
    assert np.array_equal(got, np.asarray(hregion.paste(img, inner, box)))
    outside = v == 0
    assert np.array_equal(got[outside], np.asarray(img)[outside]) and not np.array_equal(got[v == 50], np.asarray(img)[v == 50])
    # a ramp is built on the whole mask and cropped second
    m = (v >= 128).astype(np.uint8) * 255
    got = np.asarray(editor.edit(img, "an [empty] table", mask=m, mask_ramp=6, region="mask", **kw))
    want = np.asarray(editor.edit(img, "an [empty] table", mask=hmask.ramp_numpy(m, 6), mask_mode="levels", region="mask", **kw))
    assert np.array_equal(got, want)


def test_tiled_edit_ramps_the_whole_mask_once(editor):
    """One 2 x 2 case: the call equals tiles.blend_numpy of edit_batch on the tiles' crops of the whole mask's ramp."""
    import metrics_oracle as mo
    from fie_amd import mask as hmask, tiles
    W, H = 700, 560
    img = Image.fromarray(mo.textured(71, H, W))
    mask = np.zeros((H, W), np.uint8)
    mask[30:300, 150:400] = 255                                          # across all four tiles and both seams
    plan = tiles.plan((W, H), "auto", 64)
    assert plan == (512, 512, [0, 188], [0, 48])
    kw = dict(seed=9, strength=0.8)
    got = np.asarray(editor.edit(img, "a [red] kite", mask=mask, mask_ramp=24, tiles="auto", tile_overlap=64, tile_batch=2, **kw))
    ramped = hmask.ramp_numpy(mask, 24)
    tw, th, xs, ys = plan
    boxes = tiles.boxes(tw, th, xs, ys)
    R = []
    for c in tiles.chunks(len(boxes), 2):
        R += editor.edit_batch([img.crop(boxes[j]) for j in c], ["a [red] kite"] * len(c), resolution=(tw, th),
                               masks=[ramped[boxes[j][1]:boxes[j][3], boxes[j][0]:boxes[j][2]] for j in c], mask_mode="levels", **kw)
    want = tiles.blend_numpy(np.stack([np.asarray(r) for r in R]), xs, ys, H, W)
    assert np.array_equal(got, want)
    src = np.asarray(img)
    assert np.array_equal(got[mask == 0], src[mask == 0]) and not np.array_equal(got[mask > 0], src[mask > 0])
