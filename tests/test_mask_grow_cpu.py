"""`mask_grow`, host half (no GPU): the numpy restatement the device is held to (tests/mask_grow_oracle.py) against scipy's
morphology and its own properties, the argument rules, the box of a region edit, the command-line flags and the C ABI's new entry."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest
from PIL import Image

import fie_amd  # noqa: F401
from fie_amd import hip
from fie_amd import mask as hmask
from fie_amd import region as hregion

import mask_grow_oracle as mgo

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RADII = (1, -1, 2, -2, 5, -5, 16, -16)
DENSITIES = (0.0, 0.002, 0.3, 0.998, 1.0)


# ------------------------------------------------------------------------------------------------------------------------ the restatement
@pytest.mark.parametrize("h,w", [(1, 1), (5, 7), (33, 130), (65, 64)])
def test_oracle_is_scipys_disk_morphology(h, w):
    ndi = pytest.importorskip("scipy.ndimage")
    for r in RADII:
        for i, dens in enumerate(DENSITIES):
            m = mgo.random_mask(h, w, dens, 1000 * h + 10 * w + i)
            if r > 0:
                want = ndi.binary_dilation(m >= 128, structure=mgo.disk(r), border_value=0)
            else:
                want = ndi.binary_erosion(m >= 128, structure=mgo.disk(r), border_value=1)
            got = mgo.grow(m, r)
            assert got.dtype == np.uint8 and np.array_equal(got, want.astype(np.uint8) * 255), (r, dens)


@pytest.mark.parametrize("h,w", [(1, 1), (5, 7), (33, 130)])
def test_oracle_is_the_definition_word_for_word(h, w):
    for r in RADII + (3, -3, 64, -64):
        for i, dens in enumerate(DENSITIES):
            m = mgo.random_mask(h, w, dens, 100 * h + i)
            assert np.array_equal(mgo.grow(m, r), mgo.grow_literal(m, r)), (r, dens)
    assert np.array_equal(mgo.grow(mgo.grey_ramp(h, w), -2), mgo.grow_literal(mgo.grey_ramp(h, w), -2))


def test_a_single_pixel_grows_into_the_lattice_disk():
    m = np.zeros((21, 23), np.uint8)
    m[10, 11] = 255
    for r in (1, 2, 3, 5, 9):
        g = mgo.grow(m, r) > 0
        yy, xx = np.mgrid[0:21, 0:23]
        assert np.array_equal(g, (yy - 10) ** 2 + (xx - 11) ** 2 <= r * r), r
    g = mgo.grow(m, 5) > 0
    assert g[10 + 3, 11 + 4] and g[10 + 4, 11 - 3] and g[10 + 5, 11] and g[10, 11 - 5]          # 9 + 16 = 25 and 25 + 0: on the circle
    assert not g[10 + 4, 11 + 4] and not g[10, 11 + 6]                                        # 32 > 25
    assert np.array_equal(mgo.grow(m, 1) > 0, np.abs(yy - 10) + np.abs(xx - 11) <= 1)         # radius 1 is the plus shape
    assert np.array_equal(mgo.disk(5), mgo.grow(np.pad(np.full((1, 1), 255, np.uint8), 5), 5) > 0)


@pytest.mark.parametrize("h,w", [(5, 7), (40, 52)])
def test_duality_greys_and_the_trivial_masks(h, w):
    for i, dens in enumerate(DENSITIES):
        m = mgo.random_mask(h, w, dens, 7 * h + i)
        for k in (1, 2, 5, 16, 64):
            assert np.array_equal(mgo.grow(m, -k), 255 - mgo.grow(255 - m, k)), (dens, k)
    ramp = mgo.grey_ramp(h, w)
    assert (ramp == 127).any() and (ramp == 128).any()
    for r in (1, -1, 3, -3):
        assert np.array_equal(mgo.grow(ramp, r), mgo.grow((ramp >= 128).astype(np.uint8) * 255, r)), r        # 127 is out, 128 is in
    one = np.full((3, 3), 127, np.uint8)
    one[1, 1] = 128
    assert np.array_equal(mgo.grow(one, 1) > 0, mgo.disk(1)) and not mgo.grow(np.full((3, 3), 127, np.uint8), 1).any()
    empty, full = np.zeros((h, w), np.uint8), np.full((h, w), 255, np.uint8)
    for r in (1, -1, 5, -5, 64, -64):
        assert not mgo.grow(empty, r).any(), r                          # nothing grows in from outside the image
        assert (mgo.grow(full, r) == 255).all(), r                      # the image border does not erode
    assert np.array_equal(mgo.grow(ramp, 0), ramp)                      # 0: the mask as passed, greys included


def test_erosion_keeps_a_mask_that_touches_the_border():
    m = np.zeros((20, 30), np.uint8)
    m[:12, :9] = 255                                                     # in the top-left corner
    want = np.zeros((20, 30), np.uint8)
    want[:9, :6] = 255                                                   # only the two inner edges move
    assert np.array_equal(mgo.grow(m, -3), want)


# ------------------------------------------------------------------------------------------------------------------------ argument rules
def test_check_grow():
    assert hmask.MAX_GROW == mgo.MAX_GROW == 64
    for ok in (0, 64, -64):
        assert hmask.check_grow(ok, True) == ok
    v = hmask.check_grow(np.int64(3), True)
    assert v == 3 and type(v) is int
    assert hmask.check_grow(0, False) == 0                               # the default needs no mask
    for bad in (65, -65, 1.5, True, "3", None):
        with pytest.raises(ValueError, match="mask_grow"):
            hmask.check_grow(bad, True)
    for r in (1, -1):
        with pytest.raises(ValueError, match="needs a mask"):
            hmask.check_grow(r, False)


def test_keyword_is_keyword_only_with_default_0():
    from fie_amd.pipe import HipImg2ImgPipeline
    from src.pipeline import FastEditor
    for fn in (FastEditor.edit, FastEditor.edit_batch, HipImg2ImgPipeline.__call__, HipImg2ImgPipeline.prepare, HipImg2ImgPipeline.prepare_batch):
        p = inspect.signature(fn).parameters["mask_grow"]
        assert p.kind is inspect.Parameter.KEYWORD_ONLY and p.default == 0, fn.__qualname__


def test_fast_editor_refuses_before_it_touches_a_device():
    from src.pipeline import FastEditor
    editor = FastEditor.__new__(FastEditor)
    img = Image.new("RGB", (32, 24))
    mask = np.zeros((24, 32), np.uint8)
    with pytest.raises(ValueError, match="needs a mask"):
        editor.edit(img, "p", mask_grow=4)
    for bad in (65, -65, 1.5, True):
        with pytest.raises(ValueError, match="mask_grow"):
            editor.edit(img, "p", mask=mask, mask_grow=bad)
        with pytest.raises(ValueError, match="mask_grow"):
            editor.edit_batch([img, img], ["p", "q"], masks=[mask, None], mask_grow=bad)
    with pytest.raises(ValueError, match="needs a mask"):
        editor.edit_batch([img, img], ["p", "q"], masks=[None, None], mask_grow=-2)


# ------------------------------------------------------------------------------------------------------------------------ the region's box
def test_the_box_of_a_grown_mask_is_the_grown_box():
    """The bounding box of a grown mask is the original one grown by r and clipped to the image, so region="mask" resolves the grown mask to
    what it resolves a filled rectangle of that box to, whatever padding and aspect do afterwards."""
    from multiband_oracle import blob_mask
    h, w = 120, 160
    blob = np.zeros((h, w), np.uint8)
    blob[30:70, 50:110] = blob_mask(40, 60, 3)
    corner = np.zeros((h, w), np.uint8)
    corner[4:30, 140:158] = 255
    for m in (blob, corner):
        ys, xs = np.nonzero(m >= 128)
        l, t, r, b = xs.min(), ys.min(), xs.max() + 1, ys.max() + 1
        for k in (1, 6, 25):
            rect = np.zeros((h, w), np.uint8)
            rect[max(t - k, 0):min(b + k, h), max(l - k, 0):min(r + k, w)] = 255
            for pad, res in ((0, None), (8, (512, 512)), (32, "auto")):
                assert hregion.resolve("mask", (w, h), mgo.grow(m, k), pad, res) == hregion.resolve("mask", (w, h), rect, pad, res), (k, pad)
    with pytest.raises(ValueError, match="selects nothing"):           # eroded to nothing: the rule for an empty mask
        hregion.resolve("mask", (w, h), mgo.grow(corner, -13), 8, None)


# ------------------------------------------------------------------------------------------------------------------------ command line
def test_cli_flags():
    import run_batch
    import run_single_image
    flags = lambda p: {a.option_strings[0] for a in p._actions if a.option_strings}
    assert flags(run_batch.add_grow_args(run_batch.build_parser())) - flags(run_batch.build_parser()) == {"--mask_grow"}
    b = run_batch.add_grow_args(run_batch.add_mask_args(run_batch.build_parser()))
    s = run_single_image.build_parser()
    one = ["--image", "i.png", "--prompt", "p"]
    assert b.parse_args([]).mask_grow == 0 and s.parse_args(one).mask_grow == 0
    for n in (8, -3, 64, -64):
        assert b.parse_args(["--use_mask", "--mask_grow", str(n)]).mask_grow == n
        assert s.parse_args(one + ["--mask", "m.png", "--mask_grow", str(n)]).mask_grow == n
    for bad in ("65", "-65", "1.5", "x"):
        with pytest.raises(SystemExit):
            b.parse_args(["--use_mask", "--mask_grow", bad])
        with pytest.raises(SystemExit):
            s.parse_args(one + ["--mask", "m.png", "--mask_grow", bad])
    with pytest.raises(SystemExit):                                       # refused before anything is loaded
        run_batch.main(["--mask_grow", "8"])
    with pytest.raises(SystemExit):
        run_single_image.main(one + ["--mask_grow", "8"])
    for p in (b, s):
        (act,) = [a for a in p._actions if a.option_strings == ["--mask_grow"]]
        assert "pixels of the mask" in act.help
    (act,) = [a for a in b._actions if a.option_strings == ["--mask_grow"]]
    assert "frame" in act.help                                            # the decoder's 1-pixel frame grows too


# ------------------------------------------------------------------------------------------------------------------------ C ABI
def test_entry_in_header_signature_and_library():
    hip.build()
    text = open(os.path.join(ROOT, "include", "fie.h")).read()
    declared = set(re.findall(r"\b(fie_[a-z0-9_]+)\s*\(", text))
    lib = hip.lib()
    vp, i = ctypes.c_void_p, ctypes.c_int
    assert "fie_mask_grow_u8" in declared, "fie_mask_grow_u8 missing from include/fie.h"
    args = [vp, vp, i, i, i, vp]
    assert hip.SIGNATURES["fie_mask_grow_u8"] == args
    fn = lib.fie_mask_grow_u8                                             # exported by libfie_hip.so
    assert fn.restype is i and list(fn.argtypes) == args
    with pytest.raises(hip.FieError):                                     # argument checks run before any launch
        hip._chk(fn(None, None, 8, 8, 1, None))
    assert b"NULL argument" in lib.fie_last_error()
