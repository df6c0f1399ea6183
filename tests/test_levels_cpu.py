"""Soft masks, host side (no GPU): the release schedule's two statements agree, the ramp restatement against the
brute-force definition (and scipy's exact distance transform where it is installed), the support, the argument rules, the command-line flags, the
C ABI's declarations, and the levels oracle reduced to the masked oracle by a 0 / 255 map."""
import ctypes
import inspect

import numpy as np
import pytest
import torch
from PIL import Image

import fie_amd  # noqa: F401
from fie_amd import hip, mask as hmask, presets as P, tokenizer, weights

import levels_oracle
import mask_grow_oracle as mgo

SHAPES = [(1, 1), (5, 7), (33, 50), (40, 70)]
RADII = (1, 5, 17, 64)


def _masks(h, w):
    rng = np.random.default_rng(13 * h + w)
    box = np.zeros((h, w), np.uint8)
    box[h // 6:h - h // 8, w // 5:w] = 255                                # touches the right border: not an edge
    box[rng.random((h, w)) < 0.01] = 0                                   # random holes
    box[rng.random((h, w)) < 0.01] = 127                                 # and greys just below the threshold: holes too
    return {"box": box, "ones": np.full((h, w), 255, np.uint8), "zeros": np.zeros((h, w), np.uint8), "points": mgo.points_mask(h, w)}


# ---------------------------------------------------------------------------------------------------------------- the release schedule
def test_the_two_statements_of_the_schedule_agree():
    for K in range(1, 9):
        for v in range(256):
            n = hmask.level_steps(v, K)
            assert 0 <= n <= K
            for j in range(K):
                assert hmask.level_inside(v, K, j) == (n >= K - j), (v, K, j)
        assert (hmask.level_steps(0, K), hmask.level_steps(1, K), hmask.level_steps(255, K)) == (0, 1, K)
        for j in range(K):                                               # a 0 / 255 map: today's masked edit at every K and j
            assert not hmask.level_inside(0, K, j) and hmask.level_inside(255, K, j)
        assert all(hmask.level_inside(v, K, K - 1) for v in range(1, 256))          # released on the last step at the latest: the support
        counts = np.bincount([hmask.level_steps(v, K) for v in range(1, 256)], minlength=K + 1)[1:]
        assert counts.max() - counts.min() <= 1                          # the bands are equally wide


# ---------------------------------------------------------------------------------------------------------------- the ramp
@pytest.mark.parametrize("h,w", SHAPES)
def test_ramp_numpy_is_the_definition(h, w):
    for name, m in _masks(h, w).items():
        for r in RADII:
            got = hmask.ramp_numpy(m, r)
            assert got.dtype == np.uint8 and np.array_equal(got, levels_oracle.ramp_literal(m, r)), (name, r)
            assert np.array_equal(hmask.support_numpy(got), (m >= 128).astype(np.uint8) * 255), (name, r)        # the support is the binarised mask
            assert got[m >= 128].min(initial=255) >= 255 // r >= 3
    assert np.array_equal(hmask.ramp_numpy(np.full((h, w), 255, np.uint8), 64), np.full((h, w), 255, np.uint8))
    for bad in (0, 65):
        with pytest.raises(ValueError):
            hmask.ramp_numpy(np.zeros((h, w), np.uint8), bad)


@pytest.mark.parametrize("h,w", SHAPES)
def test_ramp_numpy_against_scipys_distance_transform(h, w):
    ndi = pytest.importorskip("scipy.ndimage")
    for name, m in _masks(h, w).items():
        b = m >= 128
        if b.all():
            continue                                                     # no zero pixel: the transform is meaningless there
        d2 = np.rint(ndi.distance_transform_edt(b) ** 2).astype(np.int64)
        for r in RADII:
            want = np.where(d2 >= r * r, 255, np.minimum(255, hmask._isqrt(65025 * np.minimum(d2, r * r)) // r))
            assert np.array_equal(hmask.ramp_numpy(m, r), np.where(b, want, 0).astype(np.uint8)), (name, r)


def test_the_ramp_is_a_ramp():
    m = np.zeros((40, 60), np.uint8)
    m[:, 10:] = 255                                                      # a straight outline at x = 10, the mask runs into three borders
    v = hmask.ramp_numpy(m, 5)
    assert np.array_equal(v[7], np.array([0] * 10 + [51, 102, 153, 204] + [255] * 46, np.uint8))
    assert (v[0] == v[7]).all() and (v[-1] == v[7]).all() and v[0, -1] == 255           # the border is not an edge


def test_levels_lat_and_support():
    rng = np.random.default_rng(5)
    v = rng.integers(0, 256, (64, 72), dtype=np.uint8)
    v[rng.random((64, 72)) < 0.3] = 0
    s = hmask.support_numpy(v)
    assert set(np.unique(s)) <= {0, 255} and np.array_equal(s > 0, v > 0)
    m_lat = (s[::8, ::8] >= 128).astype(np.uint8)
    lat = hmask.levels_lat_numpy(v, m_lat.reshape(-1))
    assert lat.shape == (8, 9) and np.array_equal(lat, v[::8, ::8])       # the support's latent mask: every level is kept as it is
    assert np.array_equal(lat, levels_oracle.lat_levels(v)[1])
    other = np.ones((8, 9), np.uint8)                                    # a latent mask that is set where the level map is 0: at least 1
    assert np.array_equal(hmask.levels_lat_numpy(v, other), np.maximum(v[::8, ::8], 1))
    assert not hmask.levels_lat_numpy(v, np.zeros((8, 9), np.uint8)).any()


# ---------------------------------------------------------------------------------------------------------------- argument rules
def test_check_levels():
    assert hmask.MASK_MODES == ("binary", "levels") and hmask.MAX_RAMP == 64
    assert hmask.check_levels("binary", 0, 0, False) == ("binary", 0)
    assert hmask.check_levels("levels", 0, 0, True) == ("levels", 0)
    assert hmask.check_levels("binary", np.int64(64), -5, True) == ("binary", 64)          # grow first, ramp second
    for bad in ("soft", None, 1):
        with pytest.raises(ValueError, match="mask_mode"):
            hmask.check_levels(bad, 0, 0, True)
    for bad in (-1, 65, 2.0, True, "3"):
        with pytest.raises(ValueError, match="mask_ramp"):
            hmask.check_levels("binary", bad, 0, True)
    with pytest.raises(ValueError, match="needs a mask"):
        hmask.check_levels("levels", 0, 0, False)
    with pytest.raises(ValueError, match="needs a mask"):
        hmask.check_levels("binary", 3, 0, False)
    with pytest.raises(ValueError, match="discard"):
        hmask.check_levels("levels", 3, 0, True)
    with pytest.raises(ValueError, match="discard"):
        hmask.check_levels("levels", 0, 2, True)


def test_keywords_are_keyword_only_with_their_defaults():
    from fie_amd.pipe import HipImg2ImgPipeline
    from src.pipeline import FastEditor
    for fn in (FastEditor.edit, FastEditor.edit_batch, FastEditor.edit_sweep, HipImg2ImgPipeline.__call__, HipImg2ImgPipeline.prepare,
               HipImg2ImgPipeline.prepare_batch, HipImg2ImgPipeline.prepare_sweep):
        ps = inspect.signature(fn).parameters
        for name, default in (("mask_mode", "binary"), ("mask_ramp", 0)):
            assert ps[name].kind is inspect.Parameter.KEYWORD_ONLY and ps[name].default == default, (fn.__qualname__, name)
    doc = FastEditor.edit.__doc__
    assert "pixels" in doc and "of the mask as passed" in doc and 'region="mask"' in doc


def test_fast_editor_refuses_before_it_touches_a_device():
    from src.pipeline import FastEditor
    editor = FastEditor.__new__(FastEditor)
    img = Image.new("RGB", (32, 24))
    mask = np.zeros((24, 32), np.uint8)
    for kw in (dict(mask_mode="levels"), dict(mask_ramp=4)):
        with pytest.raises(ValueError, match="needs a mask"):
            editor.edit(img, "p", **kw)
        with pytest.raises(ValueError, match="needs a mask"):
            editor.edit_batch([img, img], ["p", "q"], masks=[None, None], **kw)
        with pytest.raises(ValueError, match="needs a mask"):
            editor.edit_sweep(img, "p", **kw)
    for kw in (dict(mask_mode="levels", mask_ramp=4), dict(mask_mode="levels", mask_grow=2), dict(mask_ramp=65), dict(mask_ramp=True),
               dict(mask_mode="grey")):
        with pytest.raises(ValueError, match="mask_mode|mask_ramp"):
            editor.edit(img, "p", mask=mask, **kw)
        with pytest.raises(ValueError, match="mask_mode|mask_ramp"):
            editor.edit_batch([img, img], ["p", "q"], masks=[mask, None], **kw)
        with pytest.raises(ValueError, match="mask_mode|mask_ramp"):
            editor.edit(img, "p", mask=mask, tiles="auto", **kw)


# ---------------------------------------------------------------------------------------------------------------- command line
def test_cli_flags():
    import run_batch
    import run_single_image
    flags = lambda p: {a.option_strings[0] for a in p._actions if a.option_strings}
    assert flags(run_batch.add_levels_args(run_batch.build_parser())) - flags(run_batch.build_parser()) == {"--mask_mode", "--mask_ramp"}
    assert {"--mask_mode", "--mask_ramp"} <= flags(run_batch.full_parser())
    b = run_batch.add_levels_args(run_batch.add_grow_args(run_batch.add_mask_args(run_batch.build_parser())))
    s = run_single_image.build_parser()
    one = ["--image", "i.png", "--prompt", "p"]
    for a in (b.parse_args([]), s.parse_args(one)):
        assert (a.mask_mode, a.mask_ramp) == ("binary", 0)
    for n in (1, 8, 64):
        assert b.parse_args(["--use_mask", "--mask_ramp", str(n)]).mask_ramp == n
        assert s.parse_args(one + ["--mask", "m.png", "--mask_ramp", str(n), "--mask_grow", "4"]).mask_ramp == n
    assert b.parse_args(["--use_mask", "--mask_mode", "levels"]).mask_mode == "levels"
    assert s.parse_args(one + ["--mask", "m.png", "--mask_mode", "levels"]).mask_mode == "levels"
    for bad in (["--mask_ramp", "65"], ["--mask_ramp", "-1"], ["--mask_ramp", "1.5"], ["--mask_mode", "grey"]):
        with pytest.raises(SystemExit):
            b.parse_args(["--use_mask"] + bad)
        with pytest.raises(SystemExit):
            s.parse_args(one + ["--mask", "m.png"] + bad)
    for bad in (["--mask_ramp", "8"], ["--mask_mode", "levels"]):        # refused before anything is loaded: no mask
        with pytest.raises(SystemExit):
            run_batch.main(bad)
        with pytest.raises(SystemExit):
            run_single_image.main(one + bad)
    for bad in (["--mask_ramp", "8"], ["--mask_grow", "2"]):             # the greys would be discarded
        with pytest.raises(SystemExit):
            run_batch.main(["--use_mask", "--mask_mode", "levels"] + bad)
        with pytest.raises(SystemExit):
            run_single_image.main(one + ["--mask", "m.png", "--mask_mode", "levels"] + bad)
    for p in (b, s):
        (act,) = [a for a in p._actions if a.option_strings == ["--mask_ramp"]]
        assert "pixels of the mask" in act.help


# ---------------------------------------------------------------------------------------------------------------- C ABI
def test_entries_in_header_signature_and_library():
    hip.build()
    lib = hip.lib()
    vp, i, i64, f = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64, ctypes.c_float
    masked = hip.SIGNATURES["fie_lcm_step_masked"]
    assert masked == [vp, vp, i64, i, f, vp, vp, i64] + [f] * 6 + [vp, i, f, vp, vp, vp, vp]
    want = {"fie_lcm_step_levels": masked + [i, i], "fie_lcm_step_levels_f32": masked + [i, i], "fie_mask_levels_u8": [vp, vp, vp, i, i, vp],
            "fie_mask_support_u8": [vp, vp, i64, vp], "fie_mask_ramp_u8": [vp, vp, i, i, i, vp]}
    for name, args in want.items():
        assert hip.SIGNATURES[name] == args, name
        fn = getattr(lib, name)                                          # exported by libfie_hip.so
        assert fn.restype is i and list(fn.argtypes) == args
    with pytest.raises(hip.FieError):                                    # argument checks run before any launch
        hip._chk(lib.fie_mask_ramp_u8(None, None, 8, 8, 1, None))
    assert b"NULL argument" in lib.fie_last_error()


def test_cabi_run_edit_refuses_a_levels_job():
    from fie_amd import cabi
    with pytest.raises(NotImplementedError, match="soft mask"):
        cabi.run_edit(None, dict(lvl_lat=torch.zeros((1, 4), dtype=torch.uint8)))


def test_step_records_carry_their_place():
    from fie_amd.lcm import LCMSchedule
    sched = LCMSchedule(**P.LCM_SCHED)
    for n, s in ((4, 1.0), (4, 0.8), (4, 0.5), (4, 0.25), (8, 0.7)):
        plan = sched.plan(n, s)
        assert [st["index"] for st in plan] == list(range(len(plan))) and {st["count"] for st in plan} == {len(plan)}
        assert plan[-1]["last"]


# ---------------------------------------------------------------------------------------------------------------- the oracle
def _tiny():
    st = P.STACKS["tiny"]
    cfgs = dict(unet=st["unet"], controlnet=st["controlnet_full"], vae=st["vae"], clip_l=st["clip_l"], clip_g=st["clip_g"])
    sds = {k: weights.synth_state_dict(cfgs[k], seed=10 + i) for i, k in enumerate(cfgs)}
    return cfgs, sds


def test_levels_oracle_with_a_0_255_map_is_the_masked_oracle():
    import masked_oracle
    from oracle import canny
    cfgs, sds = _tiny()
    img = Image.fromarray(np.random.default_rng(1).integers(0, 255, (64, 64, 3), dtype=np.uint8))
    ctrl = Image.fromarray(canny.canny_rgb(np.asarray(img)))
    ids = (tokenizer.StandInTokenizer(49407)(["a cat"]), tokenizer.StandInTokenizer(0)(["a cat"]))
    neg = (tokenizer.StandInTokenizer(49407)([""]), tokenizer.StandInTokenizer(0)([""]))
    mask = np.zeros((64, 64), np.uint8)
    mask[8:48, 16:56] = 255
    kw = dict(strength=0.8, num_inference_steps=4, guidance_scale=1.5, controlnet_conditioning_scale=0.5, mask_blur=1.0)
    t_ref, t_got = {}, {}
    ref = masked_oracle.run_masked(sds, cfgs, img, ctrl, ids, neg, mask, generator=torch.Generator().manual_seed(3), trace=t_ref, **kw)
    got = levels_oracle.run_levels(sds, cfgs, img, ctrl, ids, neg, mask, generator=torch.Generator().manual_seed(3), trace=t_got, **kw)
    assert torch.equal(torch.from_numpy(got), torch.from_numpy(ref)) and torch.equal(t_got["latents"], t_ref["latents"])
    grey = mask.copy()
    grey[8:48, 16:36] = 90                                               # n(90, 3) = 2 of the 3 steps: another result over the same support
    soft = levels_oracle.run_levels(sds, cfgs, img, ctrl, ids, neg, grey, generator=torch.Generator().manual_seed(3), **kw)
    assert not np.array_equal(soft, ref) and np.array_equal(soft[mask == 0][:200], ref[mask == 0][:200])
