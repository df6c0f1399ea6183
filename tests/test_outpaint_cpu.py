"""`outpaint`, host half (no GPU): the numpy restatement the device is held to (tests/outpaint_oracle.py) against np.pad,
the argument rules, the command-line flags and the C ABI's new entry."""
import ctypes
import inspect
import itertools
import os
import re

import numpy as np
import pytest
from PIL import Image

import fie_amd  # noqa: F401
from fie_amd import hip
from fie_amd import mask as hmask

import outpaint_oracle as opo

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(1, 1), (5, 7), (33, 130)]


def _subsets():
    """Margins (left, top, right, bottom) with zeros on every subset of sides but all four: 15 of them, the non-zero sides of different widths."""
    for on in itertools.product((0, 1), repeat=4):
        if any(on):
            yield tuple(v * k for v, k in zip(on, (3, 2, 5, 4)))


# ------------------------------------------------------------------------------------------------------------------------ the restatement
@pytest.mark.parametrize("h,w", SHAPES)
def test_oracle_is_np_pad_edge_and_the_obvious_mask(h, w):
    rng = np.random.default_rng(100 * h + w)
    src = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    mask = opo.grey_mask(h, w)
    for l, t, r, b in list(_subsets()) + [(1, 0, 0, 0), (0, 0, 0, 1), (40, 0, 0, 33)]:
        got = opo.canvas(src, (l, t, r, b))
        assert got.dtype == np.uint8 and got.flags["C_CONTIGUOUS"]
        assert np.array_equal(got, np.pad(src, ((t, b), (l, r), (0, 0)), mode="edge")), (l, t, r, b)
        assert np.array_equal(got[t:t + h, l:l + w], src)
        for m in (mask, None):
            want = np.full((t + h + b, l + w + r), 255, np.uint8)
            want[t:t + h, l:l + w] = 0 if m is None else m
            gm = opo.canvas_mask(m, (h, w), (l, t, r, b))
            assert gm.dtype == np.uint8 and np.array_equal(gm, want), (l, t, r, b, m is None)


def test_greys_in_the_mask_survive():
    m = opo.grey_mask(33, 130)
    assert {1, 64, 127, 128, 200, 254} <= set(np.unique(m).tolist())
    cm = opo.canvas_mask(m, (33, 130), (4, 0, 2, 7))
    assert np.array_equal(cm[0:33, 4:134], m) and (cm[33:] == 255).all() and (cm[:, :4] == 255).all() and (cm[:, 134:] == 255).all()
    assert set(np.unique(opo.canvas_mask(None, (5, 7), (0, 1, 0, 0))).tolist()) == {0, 255}


# ------------------------------------------------------------------------------------------------------------------------ argument rules
def test_check_outpaint():
    assert hmask.MAX_OUTPAINT == opo.MAX_OUTPAINT == 4096
    assert hmask.check_outpaint(None) is None
    for ok in ((0, 0, 256, 0), [1, 0, 0, 0], (4096, 4096, 4096, 4096), (0, 0, 0, 1)):
        got = hmask.check_outpaint(ok)
        assert got == tuple(ok) and type(got) is tuple and all(type(v) is int for v in got)
    got = hmask.check_outpaint(np.array([0, 3, 0, 0]))
    assert got == (0, 3, 0, 0) and all(type(v) is int for v in got)
    bad = [(True, 0, 0, 0), (0, 0, False, 1), (1.0, 0, 0, 0), (0, 0, 2.5, 0),      # bools, floats
           (1, 2, 3), (1, 2, 3, 4, 5), (), 8, "1,2,3,4",                         # wrong length, not a sequence
           (-1, 0, 0, 0), (0, 0, 8, -8), (0, 0, 4097, 0), (0, 0, 0, 0), (None, 0, 0, 1)]
    for b in bad:
        with pytest.raises(ValueError, match="outpaint"):
            hmask.check_outpaint(b)
    assert hmask.canvas_size((200, 150), (0, 0, 56, 0)) == (256, 150) and hmask.canvas_size((200, 150), (1, 2, 3, 4)) == (204, 156)
    assert hmask.canvas_size((200, 150), None) == (200, 150)


def test_keyword_is_keyword_only_with_default_none():
    from fie_amd.pipe import HipImg2ImgPipeline
    from src.pipeline import FastEditor
    for fn in (FastEditor.edit, FastEditor.edit_batch):
        p = inspect.signature(fn).parameters["outpaint"]
        assert p.kind is inspect.Parameter.KEYWORD_ONLY and p.default is None, fn.__qualname__
    assert list(inspect.signature(FastEditor.outpaint_canvas).parameters) == ["self", "image", "outpaint", "mask"]
    for fn in (HipImg2ImgPipeline.__call__, HipImg2ImgPipeline.prepare, HipImg2ImgPipeline.prepare_batch):     # its control image comes at the edit size
        assert "outpaint" not in inspect.signature(fn).parameters, fn.__qualname__


def test_fast_editor_refuses_before_it_touches_a_device():
    from src.pipeline import FastEditor
    editor = FastEditor.__new__(FastEditor)                              # no pipe, no context: anything past the checks is an AttributeError
    img = Image.new("RGB", (32, 24))
    mask = np.zeros((24, 32), np.uint8)
    for bad in ((True, 0, 0, 0), (1.0, 0, 0, 0), (1, 2, 3), (-1, 0, 0, 0), (0, 0, 4097, 0), (0, 0, 0, 0)):
        with pytest.raises(ValueError, match="outpaint"):
            editor.edit(img, "p", outpaint=bad)
        with pytest.raises(ValueError, match="outpaint"):
            editor.edit(img, "p", mask=mask, outpaint=bad, region="mask")
        with pytest.raises(ValueError, match="outpaint"):
            editor.edit_batch([img, img], ["p", "q"], outpaint=bad)
        with pytest.raises(ValueError, match="outpaint"):
            editor.edit_batch([img, img], ["p", "q"], outpaint=[(0, 0, 8, 0), bad])
        with pytest.raises(ValueError, match="outpaint"):
            editor.outpaint_canvas(img, bad)
    with pytest.raises(ValueError, match="outpaint"):
        editor.edit_batch([img, img], ["p", "q"], outpaint=[(0, 0, 8, 0)])                      # one entry for two images
    with pytest.raises(ValueError, match="outpaint"):
        editor.outpaint_canvas(img, None)
    # the border is a mask: what needs one is satisfied by the keyword alone -- the call gets past every argument check
    for kw in (dict(mask_grow=4), dict(mask_blur=2), dict(masked_content="fill"), dict(blend="multiband")):
        with pytest.raises(AttributeError):
            editor.edit(img, "p", outpaint=(0, 0, 8, 0), **kw)
        with pytest.raises(AttributeError):
            editor.edit_batch([img, img], ["p", "q"], outpaint=[None, (0, 0, 8, 0)], **kw)
        with pytest.raises(ValueError, match="needs a mask"):
            editor.edit(img, "p", **kw)
        with pytest.raises(ValueError, match="needs a mask"):
            editor.edit_batch([img, img], ["p", "q"], outpaint=[None, None], **kw)
    with pytest.raises(ValueError, match="needs a mask"):
        editor.edit(img, "p", mask_grow=4)


# ------------------------------------------------------------------------------------------------------------------------ command line
def test_cli_flags():
    import run_batch
    import run_single_image
    flags = lambda p: {a.option_strings[0] for a in p._actions if a.option_strings}
    assert flags(run_batch.add_outpaint_args(run_batch.build_parser())) - flags(run_batch.build_parser()) == {"--outpaint"}
    b = run_batch.add_outpaint_args(run_batch.add_grow_args(run_batch.add_mask_args(run_batch.build_parser())))
    s = run_single_image.build_parser()
    one = ["--image", "i.png", "--prompt", "p"]
    assert b.parse_args([]).outpaint is None and s.parse_args(one).outpaint is None
    assert b.parse_args(["--outpaint", "0,0,256,0"]).outpaint == (0, 0, 256, 0)
    assert s.parse_args(one + ["--outpaint", "0,0,256,0"]).outpaint == (0, 0, 256, 0)
    assert s.parse_args(one + ["--outpaint", "4096, 1,2 ,3"]).outpaint == (4096, 1, 2, 3)
    for bad in ("1,2,3", "a,b,c,d", "0,0,0,0", "0,0,5000,0", "1,2,3,4,5", "-1,0,0,0", "1.5,0,0,0", ""):
        with pytest.raises(SystemExit):
            b.parse_args(["--outpaint=" + bad])
        with pytest.raises(SystemExit):
            s.parse_args(one + ["--outpaint=" + bad])
    a = s.parse_args(one + ["--mask_grow", "8", "--outpaint", "0,0,64,0"])                       # no --mask
    assert a.mask is None and a.mask_grow == 8 and a.outpaint == (0, 0, 64, 0)
    a = b.parse_args(["--mask_grow", "8", "--outpaint", "0,0,64,0"])                             # no --use_mask
    assert not a.use_mask and a.mask_grow == 8 and a.outpaint == (0, 0, 64, 0)
    # no default moves with the flag
    plain, out = s.parse_args(one), s.parse_args(one + ["--outpaint", "0,0,64,0"])
    assert {k: v for k, v in vars(out).items() if k != "outpaint"} == {k: v for k, v in vars(plain).items() if k != "outpaint"}
    plain, out = b.parse_args([]), b.parse_args(["--outpaint", "0,0,64,0"])
    assert {k: v for k, v in vars(out).items() if k != "outpaint"} == {k: v for k, v in vars(plain).items() if k != "outpaint"}


def test_cli_flags_that_need_a_mask_take_outpaint(tmp_path, capsys):
    """main() refuses --mask_grow & co. without a mask before anything is loaded (SystemExit); with --outpaint the same command line gets past
    that check -- here to the missing input, which ends the run before any model is built."""
    import run_single_image
    one = ["--image", str(tmp_path / "missing.png"), "--prompt", "p", "--output_dir", str(tmp_path / "out")]
    for flags in (["--mask_grow", "8"], ["--masked_content", "fill"], ["--blend", "multiband"], ["--region", "mask"]):
        with pytest.raises(SystemExit):
            run_single_image.main(one + flags)
        capsys.readouterr()
        assert run_single_image.main(one + flags + ["--outpaint", "0,0,64,0"]) is None
        assert "Image not found" in capsys.readouterr().out


def test_run_batch_takes_outpaint_as_a_mask():
    import run_batch
    p = run_batch.add_outpaint_args(run_batch.add_region_args(run_batch.add_grow_args(run_batch.add_blend_args(run_batch.add_mask_args(
        run_batch.build_parser())))))
    for flags in (["--mask_grow", "8"], ["--masked_content", "fill"], ["--blend", "multiband"], ["--region", "mask"]):
        with pytest.raises(ValueError, match="needs --use_mask"):
            run_batch._process_entries(None, [], p.parse_args(flags), "e", "c")
        with pytest.raises(SystemExit):
            run_batch.main(flags)
        res = run_batch._process_entries(None, [], p.parse_args(flags + ["--outpaint", "0,0,64,0"]), "e", "c")
        assert res["processed"] == 0 and res["failed"] == 0


# ------------------------------------------------------------------------------------------------------------------------ C ABI
def test_entry_in_header_signature_and_library():
    hip.build()
    text = open(os.path.join(ROOT, "include", "fie.h")).read()
    declared = set(re.findall(r"\b(fie_[a-z0-9_]+)\s*\(", text))
    lib = hip.lib()
    vp, i = ctypes.c_void_p, ctypes.c_int
    assert "fie_outpaint_canvas_rgb_u8" in declared, "fie_outpaint_canvas_rgb_u8 missing from include/fie.h"
    args = [vp, vp, vp, i, i, i, i, i, i, vp, vp]
    assert hip.SIGNATURES["fie_outpaint_canvas_rgb_u8"] == args
    fn = lib.fie_outpaint_canvas_rgb_u8                                  # exported by libfie_hip.so
    assert fn.restype is i and list(fn.argtypes) == args
    with pytest.raises(hip.FieError):                                    # argument checks run before any launch
        hip._chk(fn(None, None, None, 8, 8, 1, 0, 0, 0, None, None))
    assert b"NULL argument" in lib.fie_last_error()
