"""The one-sided multi-band paste-back, host half (no GPU): the properties of the numpy restatement that the device is held
to (tests/multiband_oracle.py), the argument rules, the command-line flags and the C ABI's new entries."""
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

import multiband_oracle as mbo

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LEVELS = (1, 2, 4, 6)


# ------------------------------------------------------------------------------------------------------------------------ the restatement
def test_known_answer_4x4():
    S = np.full((4, 4, 3), 100, np.uint8)
    A = S.copy()
    A[..., 0] = 50 + 10 * (4 * np.arange(4)[:, None] + np.arange(4)[None, :])
    m = np.array([[0, 0, 0, 0], [0, 1, 1, 0], [0, 1, 1, 1], [0, 0, 1, 1]], np.uint8) * 255
    D, G = mbo.pyramids(A, S, m, 1)
    assert np.array_equal(mbo.weight(G[1]), [[0, 0], [0, 114]])
    B = mbo.multiband(A, S, m, 1)
    assert np.array_equal(B[..., 0], [[100, 101, 102, 103], [101, 97, 105, 110], [102, 118, 129, 139], [103, 110, 163, 174]])
    assert np.array_equal(B[..., 1:], S[..., 1:])                         # A == S in green and blue
    assert np.array_equal(mbo.multiband(A, S, m >= 128, 1), B)            # a bool mask means what the u8 one does


@pytest.mark.parametrize("h,w", mbo.SIZES)
def test_identities(h, w):
    A, S = mbo.case_images(h, w, 100 * h + w)
    mask = mbo.blob_mask(h, w, w)
    for L in LEVELS:
        assert np.array_equal(mbo.multiband(A, S, np.full((h, w), 255, np.uint8), L), A), L          # all ones: B == A
        assert np.array_equal(mbo.multiband(A, S, np.zeros((h, w), np.uint8), L), S), L              # all zeros: B == S
        assert np.array_equal(mbo.multiband(S, S, mask, L), S), L                                    # A == S: B == S
        B = mbo.multiband(A, S, mask, L)
        assert B.shape == A.shape and B.dtype == np.uint8
        # the product's paste-back of B with the unfeathered mask: outside the source's bytes, inside B
        out = mbo.multiband(A, S, mask, L, alpha=(mask >= 128).astype(np.float32))
        assert np.array_equal(out, np.where((mask >= 128)[..., None], B, S)), L


def test_fade_property():
    rng = np.random.default_rng(0)
    S = rng.integers(60, 120, (128, 128, 3), dtype=np.uint8)
    A = S + 64
    m = np.zeros((128, 128), np.uint8)
    m[24:104, 24:104] = 255
    for L in (1, 2, 3, 4):
        d = mbo.multiband(A, S, m, L).astype(int) - S
        assert (d[64, 64] == 64).all(), L                                 # the centre keeps the edit
        assert d[64, 24].max() <= 26, (L, d[64, 24])                      # the first inside pixel has lost most of the offset
        assert d.max() <= 64, L
    d = mbo.multiband(A, S, m, 5).astype(int) - S                         # the 80-pixel mask is too small for the top level of L = 5
    assert (d[64, 64] == 34).all()


@pytest.mark.parametrize("h,w", [(1, 1), (5, 7), (72, 88), (33, 130)])
def test_extreme_range_stays_inside_32_bits(h, w):
    A, S = np.full((h, w, 3), 255, np.uint8), np.zeros((h, w, 3), np.uint8)
    for seed, (a, s) in enumerate(((A, S), (S, A))):
        mask = np.random.default_rng(seed + w).integers(0, 2, (h, w), dtype=np.uint8) * 255
        B = mbo.multiband(a, s, mask, 6)
        assert np.array_equal(B, mbo.multiband(a, s, mask, 6, dtype=np.int64))
        assert B.dtype == np.uint8 and 0 <= B.min() and B.max() <= 255
        D, G = mbo.pyramids(a, s, mask, 6, dtype=np.int64)
        assert max(np.abs(d).max() for d in D) <= 4080 and all(0 <= g.min() and g.max() <= 256 for g in G)
        laps = [D[k] - mbo.expand(D[k + 1], *G[k].shape) for k in range(6)]
        assert max(np.abs(lp).max() for lp in laps) <= 8160
        # the largest products of the definition: a reduce sum (256 x 4080) and a weighted band (256 x 8160), both under 2^23
        assert 256 * 8160 + 128 < 2 ** 23


def test_composite_restates_blend_u8():
    """alpha <= 0 the source's byte, alpha >= 1 the blended byte, rint of the f32 blend between (image_ops.h::blend_u8)."""
    h, w = 24, 40
    A, S = mbo.case_images(h, w, 5)
    mask = mbo.blob_mask(h, w, 6)
    alpha = hmask.feather_numpy(mask >= 128, 3.0 / 3.0)
    alpha[0, :4] = (0.0, 1.0, 1.5, -0.25)
    B = mbo.multiband(A, S, mask, 3)
    out = mbo.multiband(A, S, mask, 3, alpha=alpha)
    assert np.array_equal(out[alpha <= 0], S[alpha <= 0]) and np.array_equal(out[alpha >= 1], B[alpha >= 1])
    mid = (alpha > 0) & (alpha < 1)
    a = alpha[mid][:, None].astype(np.float64)
    assert mid.any() and np.abs(out[mid] - (a * B[mid] + (1 - a) * S[mid])).max() <= 0.5 + 1e-4


# ------------------------------------------------------------------------------------------------------------------------ argument rules
def test_argument_rules():
    assert hmask.BLEND_MODES == ("alpha", "multiband") and hmask.MAX_BLEND_LEVELS == mbo.MAX_LEVELS == 6
    assert hmask.check_blend("alpha", 4, False, False) == ("alpha", 4)
    for L in range(1, 7):
        assert hmask.check_blend("multiband", L, True, True) == ("multiband", L)
    assert hmask.check_blend("multiband", np.int64(3)) == ("multiband", 3)
    with pytest.raises(ValueError, match="needs a mask"):
        hmask.check_blend("multiband", 4, False, True)
    with pytest.raises(ValueError, match="paste_back=True"):
        hmask.check_blend("multiband", 4, True, False)
    for bad in ("laplacian", "Alpha", "", None, 1):
        with pytest.raises(ValueError) as e:
            hmask.check_blend(bad, 4, True, True)
        assert "'alpha'" in str(e.value) and "'multiband'" in str(e.value)          # the message lists both names
    for bad in (0, 7, -1, 2.0, "4", None, True):
        for blend in hmask.BLEND_MODES:
            with pytest.raises(ValueError, match="blend_levels"):
                hmask.check_blend(blend, bad, True, True)


def test_keywords_are_keyword_only_with_the_old_defaults():
    from fie_amd.pipe import HipImg2ImgPipeline
    from src.pipeline import FastEditor
    for fn in (FastEditor.edit, FastEditor.edit_batch, HipImg2ImgPipeline.__call__, HipImg2ImgPipeline.prepare, HipImg2ImgPipeline.prepare_batch):
        ps = inspect.signature(fn).parameters
        assert ps["blend"].kind is inspect.Parameter.KEYWORD_ONLY and ps["blend"].default == "alpha", fn.__qualname__
        assert ps["blend_levels"].kind is inspect.Parameter.KEYWORD_ONLY and ps["blend_levels"].default == 4, fn.__qualname__


def test_fast_editor_refuses_before_it_touches_a_device():
    """edit() / edit_batch() check their arguments first: an editor that was never initialised (no model, no device) raises the rule's error."""
    from src.pipeline import FastEditor
    editor = FastEditor.__new__(FastEditor)
    img = Image.new("RGB", (32, 24))
    mask = np.zeros((24, 32), np.uint8)
    with pytest.raises(ValueError, match="needs a mask"):
        editor.edit(img, "p", blend="multiband")
    with pytest.raises(ValueError, match="paste_back=True"):
        editor.edit(img, "p", mask=mask, paste_back=False, blend="multiband")
    with pytest.raises(ValueError, match="'multiband'"):
        editor.edit(img, "p", mask=mask, blend="poisson")
    with pytest.raises(ValueError, match="blend_levels"):
        editor.edit(img, "p", mask=mask, blend="multiband", blend_levels=7)
    with pytest.raises(ValueError, match="blend_levels"):
        editor.edit(img, "p", mask=mask, blend_levels=0)
    with pytest.raises(ValueError, match="needs a mask"):
        editor.edit_batch([img, img], ["p", "q"], blend="multiband")
    with pytest.raises(ValueError, match="needs a mask"):
        editor.edit_batch([img, img], ["p", "q"], masks=[None, None], blend="multiband")
    with pytest.raises(ValueError, match="paste_back=True"):
        editor.edit_batch([img, img], ["p", "q"], masks=[mask, None], paste_back=False, blend="multiband")
    with pytest.raises(ValueError, match="blend_levels"):
        editor.edit_batch([img, img], ["p", "q"], masks=[mask, None], blend="multiband", blend_levels=9)


def test_cli_flags():
    import run_batch
    import run_single_image
    flags = lambda p: {a.option_strings[0] for a in p._actions if a.option_strings}
    assert flags(run_batch.add_blend_args(run_batch.build_parser())) - flags(run_batch.build_parser()) == {"--blend", "--blend_levels"}
    b = run_batch.add_blend_args(run_batch.add_mask_args(run_batch.build_parser()))
    s = run_single_image.build_parser()
    one = ["--image", "i.png", "--prompt", "p"]
    assert (b.parse_args([]).blend, b.parse_args([]).blend_levels) == ("alpha", 4)
    assert (s.parse_args(one).blend, s.parse_args(one).blend_levels) == ("alpha", 4)
    for L in range(1, 7):
        a = b.parse_args(["--use_mask", "--blend", "multiband", "--blend_levels", str(L)])
        assert (a.blend, a.blend_levels) == ("multiband", L)
        a = s.parse_args(one + ["--mask", "m.png", "--blend", "multiband", "--blend_levels", str(L)])
        assert (a.blend, a.blend_levels) == ("multiband", L)
    for bad in (["--blend", "poisson"], ["--blend_levels", "0"], ["--blend_levels", "7"]):
        with pytest.raises(SystemExit):
            b.parse_args(["--use_mask"] + bad)
        with pytest.raises(SystemExit):
            s.parse_args(one + ["--mask", "m.png"] + bad)
    with pytest.raises(SystemExit):                                       # refused before anything is loaded
        run_batch.main(["--blend", "multiband"])
    with pytest.raises(SystemExit):
        run_single_image.main(one + ["--blend", "multiband"])
    with pytest.raises(SystemExit):
        run_single_image.main(one + ["--mask", "m.png", "--no_paste_back", "--blend", "multiband"])


def test_cabi_walk_refuses_a_multiband_job():
    from fie_amd import cabi
    with pytest.raises(NotImplementedError, match="multiband"):
        cabi.run_edit(None, dict(blend=("multiband", 4)))


# ------------------------------------------------------------------------------------------------------------------------ C ABI
def test_entries_in_header_signatures_and_library():
    hip.build()
    text = open(os.path.join(ROOT, "include", "fie.h")).read()
    declared = set(re.findall(r"\b(fie_[a-z0-9_]+)\s*\(", text))
    lib = hip.lib()
    vp, i = ctypes.c_void_p, ctypes.c_int
    want = {"fie_multiband_workspace_bytes": (ctypes.c_int64, [i, i, i]),
            "fie_multiband_blend_rgb_u8": (i, [vp, vp, vp, vp, vp, i, i, i, vp, vp])}
    for name, (ret, args) in want.items():
        assert name in declared, f"{name} missing from include/fie.h"
        assert hip.SIGNATURES[name] == args, name
        fn = getattr(lib, name)                                           # exported by libfie_hip.so
        assert fn.restype is ret and list(fn.argtypes) == args, name
    ws = lib.fie_multiband_workspace_bytes
    cells = lambda h, w, L: sum(-(-h // 2 ** k) * -(-w // 2 ** k) for k in range(1, L + 1))
    for h, w in ((1, 1), (5, 7), (24, 40), (72, 88), (200, 136), (1024, 1024), (1, 7)):
        sizes = [ws(h, w, L) for L in range(1, 7)]
        assert all(a < b for a, b in zip(sizes, sizes[1:])), (h, w, sizes)            # monotone in levels
        assert sizes == [24 * cells(h, w, L) for L in range(1, 7)], (h, w)            # short4 {D, G} and int4 C per cell of levels 1 .. L
        assert all(n % 8 == 0 and n > 0 for n in sizes)
    for L in (0, 7, -1):
        assert ws(64, 64, L) == -1, L
    assert ws(4096, 4096, 4) > 0 and ws(4096, 4097, 4) == -1 and ws(0, 8, 4) == -1 and ws(8, -1, 4) == -1
    with pytest.raises(hip.FieError):                                     # argument checks run before any launch
        hip._chk(lib.fie_multiband_blend_rgb_u8(None, None, None, None, None, 8, 8, 4, None, None))
    assert b"NULL argument" in lib.fie_last_error()
