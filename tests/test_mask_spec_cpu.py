"""MaskSpec (fie_amd/mask.py; no GPU): the one checked value every entry point builds from its mask keywords.  check() against the five rule sets
it runs, over the whole grid of their arguments; the round trip through the public keyword names and the derivations; the public signatures and
the command lines' option sets, pinned to what they were before the spec existed; the command lines' shared post-parse helper."""
import dataclasses
import inspect
import itertools

import pytest

import fie_amd  # noqa: F401
from fie_amd import mask as hmask
from fie_amd.mask import MaskSpec

GRID = dict(mask_blur=(0, 1.5, 22, "x"), paste_back=(True, False), masked_content=("original", "fill", "bad"),
            blend=("alpha", "multiband", "bad"), blend_levels=(4, 7), mask_grow=(0, 3, 65), mask_mode=("binary", "levels", "grey"),
            mask_ramp=(0, 4, 65), have_mask=(True, False), paste_later=(True, False))


def _cases():
    return [dict(zip(GRID, values)) for values in itertools.product(*GRID.values())]


def _rules(mask_blur, paste_back, masked_content, blend, blend_levels, mask_grow, mask_mode, mask_ramp, have_mask, paste_later):
    """The five rule sets, called here in the one fixed order: args, content, blend, grow, levels."""
    blur = hmask.check_args(mask_blur, paste_back, have_mask)
    content = hmask.check_content(masked_content, have_mask)
    blend, levels = hmask.check_blend(blend, blend_levels, have_mask, paste_back or paste_later)
    grow = hmask.check_grow(mask_grow, have_mask)
    mode, ramp = hmask.check_levels(mask_mode, mask_ramp, grow, have_mask)
    return dict(blur=blur, paste_back=paste_back, content=content, blend=blend, blend_levels=levels, grow=grow, mode=mode, ramp=ramp,
                paste_later=paste_later)


def _valid_specs():
    out = []
    for case in _cases():
        try:
            _rules(**case)
        except ValueError:
            continue
        out.append((case, MaskSpec.check(**case)))
    return out


def test_check_is_the_five_rule_sets_in_one_order_over_the_full_grid():
    cases = _cases()
    assert len(cases) == 15552
    valid = 0
    for case in cases:
        try:
            want = _rules(**case)
        except ValueError as e:
            with pytest.raises(ValueError) as got:
                MaskSpec.check(**case)
            assert str(got.value) == str(e), case
            continue
        spec = MaskSpec.check(**case)
        assert dataclasses.asdict(spec) == want, case
        assert (type(spec.blur), type(spec.blend_levels), type(spec.grow), type(spec.ramp)) == (float, int, int, int)
        valid += 1
    assert 0 < valid < len(cases)


def test_keywords_round_trip_unmasked_and_value_semantics():
    valid = _valid_specs()
    assert any(s.soft for _, s in valid) and any(s.paste_later and s.blend == "multiband" and not s.paste_back for _, s in valid)
    for case, s in valid:
        kw = s.keywords()
        assert set(kw) - {"paste_later"} == {"mask_blur", "paste_back", "masked_content", "blend", "blend_levels", "mask_grow", "mask_mode",
                                             "mask_ramp"}
        assert MaskSpec.check(**kw, have_mask=True) == s, case
        u = s.unmasked()
        assert u == MaskSpec(paste_back=s.paste_back, paste_later=s.paste_later)          # every other field at its default
        assert MaskSpec.check(**u.keywords(), have_mask=False) == u, case
        assert s.soft == (s.mode != "binary" or s.ramp != 0)
    a = MaskSpec.check(2, True, "fill", "multiband", 3, 4, "binary", 8, have_mask=True)
    b = MaskSpec.check(2.0, True, "fill", "multiband", 3, 4, "binary", 8, have_mask=True)
    assert a == b and hash(a) == hash(b) and len({a, b, a.unmasked()}) == 2
    assert MaskSpec() == MaskSpec.check(have_mask=False) and a != dataclasses.replace(a, ramp=0)
    with pytest.raises(dataclasses.FrozenInstanceError):
        a.grow = 0


def test_the_two_derivations():
    for _, s in _valid_specs():
        f = s.behind_fullres()          # behind the full-resolution back end: no feather, no paste-back in the job, the caller pastes later
        assert f == dataclasses.replace(s, blur=0.0, paste_back=False, paste_later=True)
        p = s.prepared()                # the mask has been grown and ramped on the device already
        assert p == dataclasses.replace(s, grow=0, ramp=0, mode="levels" if s.soft else "binary")
        assert p.soft == s.soft and p.prepared() == p
        assert MaskSpec.check(**f.prepared().keywords(), have_mask=True) == f.prepared()  # what the pipeline is handed passes its own check


def test_a_size_group_without_masks_runs_as_without_the_keywords():
    """edit_batch splits mixed target sizes into one call per size; a group none of whose images has a mask re-enters with unmasked(), so the
    call's mask_blur does not refuse it ("mask_blur needs a mask").  No device here: past the checks an uninitialised editor has no attributes."""
    import numpy as np
    from PIL import Image
    from src.pipeline import FastEditor
    editor = FastEditor.__new__(FastEditor)
    wide, tall = Image.new("RGB", (160, 128)), Image.new("RGB", (128, 192))
    mask = np.zeros((128, 160), np.uint8)
    mask[10:60, 10:60] = 255
    with pytest.raises(AttributeError):
        editor.edit_batch([tall, wide], ["p", "q"], masks=[None, mask], mask_blur=2, mask_grow=3, masked_content="fill", resolution="auto")
    with pytest.raises(ValueError, match="mask_blur needs a mask"):
        editor.edit_batch([tall, wide], ["p", "q"], masks=[None, None], mask_blur=2, resolution="auto")


SIGNATURES = {
    "FastEditor.edit": "(self, image, prompt, negative_prompt='', strength=0.8, num_inference_steps=4, guidance_scale=1.5, "
                       "controlnet_conditioning_scale=0.5, canny_low_threshold=100, canny_high_threshold=200, seed=None, mask=None, mask_blur=0, "
                       "paste_back=True, *, resolution=None, metrics=False, output_size=None, region=None, region_padding=32, "
                       "masked_content='original', blend='alpha', blend_levels=4, mask_grow=0, outpaint=None, tiles=None, tile_overlap=128, "
                       "tile_batch=4, mask_mode='binary', mask_ramp=0)",
    "FastEditor.edit_batch": "(self, images, prompts, negative_prompts=None, strength=0.8, num_inference_steps=4, guidance_scale=1.5, "
                             "controlnet_conditioning_scale=0.5, canny_low_threshold=100, canny_high_threshold=200, seed=None, masks=None, "
                             "mask_blur=0, paste_back=True, *, resolution=None, metrics=False, output_size=None, region=None, region_padding=32, "
                             "masked_content='original', blend='alpha', blend_levels=4, mask_grow=0, outpaint=None, tiles=None, "
                             "tile_overlap=128, tile_batch=4, mask_mode='binary', mask_ramp=0)",
    "FastEditor.edit_sweep": "(self, image, prompt, negative_prompt='', strengths='all', num_inference_steps=4, guidance_scale=1.5, "
                             "controlnet_conditioning_scale=0.5, canny_low_threshold=100, canny_high_threshold=200, seed=None, mask=None, "
                             "mask_blur=0, paste_back=True, *, resolution=None, output_size=None, region=None, tiles=None, "
                             "masked_content='original', blend='alpha', blend_levels=4, mask_grow=0, outpaint=None, select=None, min_ssim=None, "
                             "mask_mode='binary', mask_ramp=0)",
    "HipImg2ImgPipeline.__call__": "(self, prompt, negative_prompt='', image=None, control_image=None, strength=0.8, num_inference_steps=4, "
                                   "guidance_scale=1.5, controlnet_conditioning_scale=0.5, generator=None, output_type='pil', slot=0, "
                                   "post_check=None, mask_image=None, mask_blur=0, paste_back=True, after_device=None, *, "
                                   "masked_content='original', blend='alpha', blend_levels=4, paste_later=False, mask_grow=0, mask_mode='binary', "
                                   "mask_ramp=0, **unused)",
    "HipImg2ImgPipeline.prepare": "(self, prompt, negative_prompt='', image=None, control_image=None, strength=0.8, num_inference_steps=4, "
                                  "guidance_scale=1.5, controlnet_conditioning_scale=0.5, generator=None, mask_image=None, mask_blur=0, "
                                  "paste_back=True, *, masked_content='original', blend='alpha', blend_levels=4, paste_later=False, mask_grow=0, "
                                  "mask_mode='binary', mask_ramp=0)",
    "HipImg2ImgPipeline.prepare_batch": "(self, prompts, negative_prompts, images, control_images, strength=0.8, num_inference_steps=4, "
                                        "guidance_scale=1.5, controlnet_conditioning_scale=0.5, generators=None, mask_image=None, mask_blur=0, "
                                        "paste_back=True, *, masked_content='original', blend='alpha', blend_levels=4, paste_later=False, "
                                        "mask_grow=0, mask_mode='binary', mask_ramp=0)",
    "HipImg2ImgPipeline.prepare_sweep": "(self, prompt, negative_prompt='', image=None, control_image=None, strengths='all', "
                                        "num_inference_steps=4, guidance_scale=1.5, controlnet_conditioning_scale=0.5, generator=None, "
                                        "mask_image=None, mask_blur=0, paste_back=True, *, masked_content='original', blend='alpha', "
                                        "blend_levels=4, paste_later=False, mask_grow=0, mask_mode='binary', mask_ramp=0)",
}
BATCH_OPTIONS = {
    "--auto_strength", "--batch_size", "--blend", "--blend_levels", "--canny_high", "--canny_low", "--clip_score_dir", "--control_scale",
    "--dino_dir", "--editing_types", "--full_controlnet", "--full_precision", "--guidance", "--help", "--image_ids", "--in_flight", "--lpips_dir",
    "--mapping_file", "--mask_grow", "--mask_mode", "--mask_ramp", "--masked_content", "--metrics", "--min_ssim", "--model", "--negative_prompt",
    "--no_cpu_offload", "--num_images", "--outpaint", "--output_dir", "--output_size", "--quality_mode", "--region", "--region_padding",
    "--resolution", "--results_json", "--save_comparisons", "--seed", "--skip_existing", "--source_dir", "--steps", "--strength", "--strengths",
    "--tile_batch", "--tile_overlap", "--tiles", "--use_mask", "--weights_dir", "-h"}
SINGLE_OPTIONS = {
    "--blend", "--blend_levels", "--canny_high", "--canny_low", "--clip_score_dir", "--compute_metrics", "--control_scale", "--dino_dir",
    "--full_controlnet", "--full_precision", "--guidance", "--help", "--image", "--lpips_dir", "--mask", "--mask_blur", "--mask_grow",
    "--mask_mode", "--mask_ramp", "--masked_content", "--model", "--negative_prompt", "--no_cpu_offload", "--no_paste_back", "--outpaint",
    "--output_dir", "--output_size", "--prompt", "--quality_mode", "--region", "--region_padding", "--resolution", "--seed", "--show_plot",
    "--steps", "--strength", "--weights_dir", "-h"}


def test_public_signatures_and_option_sets_are_what_they_were():
    import run_batch
    import run_single_image
    from fie_amd.pipe import HipImg2ImgPipeline
    from src.pipeline import FastEditor
    fns = (FastEditor.edit, FastEditor.edit_batch, FastEditor.edit_sweep, HipImg2ImgPipeline.__call__, HipImg2ImgPipeline.prepare,
           HipImg2ImgPipeline.prepare_batch, HipImg2ImgPipeline.prepare_sweep)
    assert {fn.__qualname__: str(inspect.signature(fn)) for fn in fns} == SIGNATURES
    options = lambda p: {o for a in p._actions for o in a.option_strings}
    assert options(run_batch.full_parser()) == BATCH_OPTIONS
    assert options(run_single_image.build_parser()) == SINGLE_OPTIONS


LEVELS_CLASH = "--mask_mode levels does not go with --mask_ramp or --mask_grow: both work on the outline and would discard the greys"


def _parsers():
    import run_batch
    import run_single_image
    one = ["--image", "i.png", "--prompt", "p"]
    return (("--use_mask", lambda flags: run_batch.full_parser().parse_args(flags), ["--use_mask"], ""),
            ("--mask", lambda flags: run_single_image.build_parser().parse_args(one + flags), ["--mask", "m.png"], " and the paste-back"))


def test_cli_keywords_refuses_with_the_messages_of_the_two_main_functions():
    for flag, parse, with_mask, blend_tail in _parsers():
        refusals = ((["--masked_content", "fill"], f"--masked_content needs {flag}"),
                    (["--blend", "multiband"], f"--blend multiband needs {flag}{blend_tail}"),
                    (["--mask_grow", "4"], f"--mask_grow needs {flag}"),
                    (["--mask_grow", "-4"], f"--mask_grow needs {flag}"),
                    (["--mask_ramp", "8"], f"--mask_mode levels and --mask_ramp need {flag}"),
                    (["--mask_mode", "levels"], f"--mask_mode levels and --mask_ramp need {flag}"))
        for flags, message in refusals:
            with pytest.raises(ValueError) as e:
                hmask.cli_keywords(parse(flags), False, flag)
            assert str(e.value) == message
            assert hmask.cli_keywords(parse(with_mask + flags), True, flag)               # with a mask (or an outpaint border) it passes
        for flags in (["--mask_mode", "levels", "--mask_ramp", "8"], ["--mask_mode", "levels", "--mask_grow", "4"]):
            with pytest.raises(ValueError) as e:
                hmask.cli_keywords(parse(with_mask + flags), True, flag)
            assert str(e.value) == LEVELS_CLASH
    flag, parse, with_mask, _ = _parsers()[1]                                               # run_single_image alone can switch the paste-back off
    with pytest.raises(ValueError) as e:
        hmask.cli_keywords(parse(with_mask + ["--blend", "multiband", "--no_paste_back"]), True, flag)
    assert str(e.value) == "--blend multiband needs --mask and the paste-back"


def test_cli_keywords_returns_exactly_the_non_default_keywords():
    import argparse
    for flag, parse, with_mask, _ in _parsers():
        assert hmask.cli_keywords(parse([]), False, flag) == {} and hmask.cli_keywords(parse(with_mask), True, flag) == {}
        assert hmask.cli_keywords(parse(with_mask + ["--blend_levels", "3"]), True, flag) == {}          # levels of a blend that is not asked for
        assert hmask.cli_keywords(parse(with_mask + ["--masked_content", "fill"]), True, flag) == dict(masked_content="fill")
        assert hmask.cli_keywords(parse(with_mask + ["--blend", "multiband"]), True, flag) == dict(blend="multiband", blend_levels=4)
        assert hmask.cli_keywords(parse(with_mask + ["--mask_grow", "-3"]), True, flag) == dict(mask_grow=-3)
        assert hmask.cli_keywords(parse(with_mask + ["--mask_mode", "levels"]), True, flag) == dict(mask_mode="levels", mask_ramp=0)
        every = ["--masked_content", "latent_noise", "--blend", "multiband", "--blend_levels", "2", "--mask_grow", "5", "--mask_ramp", "9"]
        got = hmask.cli_keywords(parse(with_mask + every), True, flag)
        assert got == dict(masked_content="latent_noise", blend="multiband", blend_levels=2, mask_grow=5, mask_mode="binary", mask_ramp=9)
        assert MaskSpec.check(**got, have_mask=True).keywords() == dict(MaskSpec().keywords(), **got)       # edit()'s keyword names
    bare = argparse.Namespace(use_mask=False)                                               # a parser without the additive groups: all defaults
    assert hmask.cli_keywords(bare, False, "--use_mask") == {} and hmask.cli_keywords(bare, True, "--use_mask") == {}
