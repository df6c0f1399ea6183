"""Masked-content modes, host half (no GPU): the argument rules, the command-line flags, the C ABI's new entries and the
properties of the numpy fill that the device is held to (tests/masked_content_oracle.py)."""
import inspect
import os
import re

import numpy as np
import pytest

import fie_amd  # noqa: F401
from fie_amd import hip
from fie_amd import mask as hmask

import masked_content_oracle as mco

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODES = ("original", "fill", "latent_noise", "latent_nothing")
NEW = ("fie_mask_fill_workspace_bytes", "fie_mask_fill_rgb_u8", "fie_latent_prep_src_content", "fie_latent_prep_src_content_f32")


# ------------------------------------------------------------------------------------------------------------------------ argument rules
def test_argument_rules():
    assert hmask.CONTENT_MODES == MODES
    for mode in MODES:
        assert hmask.check_content(mode, True) == mode
    assert hmask.check_content("original", False) == "original"
    for mode in MODES[1:]:
        with pytest.raises(ValueError, match="needs a mask"):
            hmask.check_content(mode, False)
    for bad in ("noise", "Fill", "", None, 1):
        with pytest.raises(ValueError) as e:
            hmask.check_content(bad, True)
        for mode in MODES:                                   # the message lists the four names
            assert repr(mode) in str(e.value)


def test_keyword_is_keyword_only_with_default_original():
    from fie_amd.pipe import HipImg2ImgPipeline
    from src.pipeline import FastEditor
    for fn in (FastEditor.edit, FastEditor.edit_batch, HipImg2ImgPipeline.__call__, HipImg2ImgPipeline.prepare, HipImg2ImgPipeline.prepare_batch):
        p = inspect.signature(fn).parameters["masked_content"]
        assert p.kind is inspect.Parameter.KEYWORD_ONLY and p.default == "original", fn.__qualname__


def test_cli_flags():
    import run_batch
    import run_single_image
    flags = lambda p: {a.option_strings[0] for a in p._actions if a.option_strings}
    assert "--masked_content" not in flags(run_batch.build_parser())       # build_parser's flag set stays the reference's + earlier additions
    assert flags(run_batch.add_mask_args(run_batch.build_parser())) - flags(run_batch.build_parser()) == {"--use_mask", "--masked_content"}
    b = run_batch.add_mask_args(run_batch.build_parser())
    s = run_single_image.build_parser()
    assert b.parse_args([]).masked_content == "original"
    assert s.parse_args(["--image", "i.png", "--prompt", "p"]).masked_content == "original"
    for mode in MODES:
        assert b.parse_args(["--use_mask", "--masked_content", mode]).masked_content == mode
        assert s.parse_args(["--image", "i.png", "--prompt", "p", "--mask", "m.png", "--masked_content", mode]).masked_content == mode
    with pytest.raises(SystemExit):
        b.parse_args(["--use_mask", "--masked_content", "blur"])
    with pytest.raises(SystemExit):
        s.parse_args(["--image", "i.png", "--prompt", "p", "--mask", "m.png", "--masked_content", "blur"])
    with pytest.raises(SystemExit):                                       # refused before anything is loaded
        run_batch.main(["--masked_content", "fill"])
    with pytest.raises(SystemExit):
        run_single_image.main(["--image", "i.png", "--prompt", "p", "--masked_content", "fill"])


# ------------------------------------------------------------------------------------------------------------------------ C ABI
def test_entries_in_header_signatures_and_library():
    hip.build()
    text = open(os.path.join(ROOT, "include", "fie.h")).read()
    declared = set(re.findall(r"\b(fie_[a-z0-9_]+)\s*\(", text))
    lib = hip.lib()
    for name in NEW:
        assert name in declared, f"{name} missing from include/fie.h"
        assert name in hip.SIGNATURES, f"{name} missing from hip.SIGNATURES"
        assert hasattr(lib, name), f"{name} not exported by libfie_hip.so"
    for i, mode in enumerate(MODES):                                      # the C codes are the positions of the names
        assert re.search(rf"#define FIE_CONTENT_{mode.upper()} {i}\b", text), mode
    # the workspace query is host code: 16 bytes per cell of the pyramid above the image, sides ceil-halved down to 1x1
    cells = lambda h, w: 0 if (h, w) == (1, 1) else ((h + 1) // 2) * ((w + 1) // 2) + cells((h + 1) // 2, (w + 1) // 2)
    for h, w in ((8, 8), (24, 40), (72, 88), (200, 136), (1024, 1024), (1, 7)):
        assert lib.fie_mask_fill_workspace_bytes(h, w) == 16 * cells(h, w), (h, w)
    assert lib.fie_mask_fill_workspace_bytes(1, 1) == 16                  # nothing above a 1x1 image: one cell, never a zero-byte buffer
    assert lib.fie_mask_fill_workspace_bytes(0, 8) == -1 and lib.fie_mask_fill_workspace_bytes(8, -1) == -1
    assert lib.fie_mask_fill_workspace_bytes(4096, 4096) == 16 * cells(4096, 4096) and lib.fie_mask_fill_workspace_bytes(4096, 4097) == -1
    with pytest.raises(hip.FieError):                                     # argument checks run before any launch
        hip._chk(lib.fie_mask_fill_rgb_u8(None, None, None, 8, 8, None, None, None, None))
    assert b"NULL argument" in lib.fie_last_error()


# ------------------------------------------------------------------------------------------------------------------------ oracle properties
_image, _masks = mco.case_image, mco.case_masks
SIZES = [(8, 8), (24, 40), (72, 88), (1, 1), (5, 1), (3, 7)]


@pytest.mark.parametrize("h,w", SIZES)
def test_fill_properties(h, w):
    src = _image(h, w, h * 100 + w)
    for name, mask in _masks(h, w, w).items():
        m = mask >= 128
        out = mco.fill(src, mask)
        assert out.shape == src.shape and out.dtype == np.uint8
        assert np.array_equal(out[~m], src[~m]), name                     # known pixels are byte-identical
        if m.all():
            assert (out == 128).all(), name                               # nothing known: mid grey
            continue
        if not m.any():
            assert np.array_equal(out, src), name
        for c in range(3):                                                # every filled value within the range of the known pixels
            lo, hi = src[..., c][~m].min(), src[..., c][~m].max()
            assert lo <= out[..., c].min() and out[..., c].max() <= hi, (name, c)
        const = np.empty_like(src)
        const[:] = (17, 200, 255)
        assert np.array_equal(mco.fill(const, mask), const), name         # a constant image fills with that constant


@pytest.mark.parametrize("h,w", [(8, 8), (9, 13), (1, 1), (5, 1), (3, 7), (24, 40)])
def test_fill_vectorised_equals_the_cell_by_cell_statement(h, w):
    src = _image(h, w, 7 * h + w)
    for name, mask in _masks(h, w, h).items():
        assert np.array_equal(mco.fill(src, mask), mco.fill_loops(src, mask)), name


def test_fill_is_a_continuation_not_a_copy():
    """A horizontal ramp with a hole in the middle: the fill stays between the hole's left and right neighbours (smooth, monotone enough to
    remove an object), and a bool mask means what the u8 one does."""
    src = np.repeat(np.linspace(0, 255, 64).astype(np.uint8)[None, :, None], 64, 0).repeat(3, 2)
    mask = np.zeros((64, 64), np.uint8)
    mask[16:48, 24:40] = 255
    out = mco.fill(src, mask)
    assert src[0, 23, 0] <= out[16:48, 24:40].min() and out[16:48, 24:40].max() <= src[0, 40, 0]
    assert np.array_equal(out, mco.fill(src, mask >= 128))


def test_edge_clear_and_latent_rules():
    rng = np.random.default_rng(3)
    ctl = rng.integers(0, 2, (16, 24, 1), dtype=np.uint8).repeat(3, 2) * 255
    mask = rng.choice(np.array([0, 127, 128, 255], np.uint8), (16, 24))
    cleared = mco.clear_edges(ctl, mask)
    assert not cleared[mask >= 128].any() and np.array_equal(cleared[mask < 128], ctl[mask < 128])
    assert np.array_equal(mco.latent_mask(mask), (mask >= 128)[::8, ::8])
    hw = 6
    orig = rng.standard_normal((hw, 4)).astype(np.float32)
    n = rng.standard_normal((4, hw)).astype(np.float32)
    m = np.array([1, 0, 1, 0, 0, 1], bool)
    s = np.float32(0.937)
    for mode in ("original", "fill"):
        assert np.array_equal(mco.initial_latents(mode, orig, n, m, s), orig)
    noise = mco.initial_latents("latent_noise", orig, n, m, s)
    nothing = mco.initial_latents("latent_nothing", orig, n, m, s)
    assert np.array_equal(noise[m], n.T[m]) and np.array_equal(noise[~m], orig[~m])
    assert np.array_equal(nothing[m], (s * n.T)[m]) and np.array_equal(nothing[~m], orig[~m]) and nothing.dtype == np.float32
