"""Tiled edits, the device-free half (fie_amd/tiles.py): the plan's properties over its whole range, the worked examples,
the split into device jobs, every argument error, the three properties of the integer blend, the command-line flags and the C entry's place
in the header and the library."""
import ctypes
import os
import re

import numpy as np
import pytest

import fie_amd  # noqa: F401
from fie_amd import hip, tiles

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OVERLAPS = (0, 1, 64, 128, 200, 256)


def _axis_facts(S, t, pos, o):
    """The properties every planned axis has; -> the largest number of tiles that share a pixel."""
    assert pos[0] == 0 and pos[-1] == S - t, (S, t, pos)
    assert all(a < b for a, b in zip(pos, pos[1:])), (S, t, pos)                       # strictly increasing
    assert all(a + t - b >= o for a, b in zip(pos, pos[1:])), (S, t, o, pos)           # neighbours overlap by at least o (so: no gap)
    cover = np.zeros(S, np.int64)
    for p in pos:
        cover[p:p + t] += 1
    assert cover.min() >= 1, (S, t, pos)
    return int(cover.max())


def test_auto_plan_properties():
    """512 <= t <= 1024, t % 64 == 0, t <= S; first at 0, last at S - t, increasing; overlaps >= o; all covered; per-axis coverage <= 2.  S over
    512..5999: every S up to 1100 (all residues mod 64 below and around the one-tile limit), then a stride of 7 (coprime to 64), plus the
    multiples of 64 and their neighbours."""
    sides = sorted(set(range(512, 1101)) | set(range(1100, 6000, 7)) | {s + d for s in range(1088, 6000, 64) for d in (-1, 0, 1) if s + d < 6000})
    for o in OVERLAPS:
        for S in sides:
            t, _, xs, _ = tiles.plan((S, 512), "auto", o)
            assert 512 <= t <= 1024 and t % 64 == 0 and t <= S, (S, o, t)
            assert _axis_facts(S, t, xs, o) <= 2, (S, o, t, xs)
            if S <= 1024 and S % 64 == 0:
                assert (t, xs) == (S, [0])
            _, _, xs2, ys2 = tiles.plan((512, S), "auto", o)                            # the axes are planned alike, each on its own
            assert ys2 == xs and xs2 == [0]


def test_explicit_plan_properties():
    most = 0
    for t in (512, 576, 1024):
        for o in OVERLAPS:
            for S in list(range(t, t + 130)) + list(range(t + 130, 6000, 11)):
                tw, th, xs, ys = tiles.plan((S, t), (t, t), o)
                assert (tw, th, ys) == (t, t, [0])
                most = max(most, _axis_facts(S, t, xs, o))
                if S == t:
                    assert xs == [0]
                else:
                    assert len(xs) == max(2, -(-(S - o) // (t - o)))
    assert most == 3                                                                    # explicit sides reach triple coverage, never more
    assert tiles.plan((2047, 2047), (1024, 1024), 2)[2:] == ([0, 511, 1023], [0, 511, 1023])       # the blend's worst case


def test_worked_examples():
    tw, th, xs, ys = tiles.plan((4000, 3000), "auto", 128)
    assert (tw, th, len(xs), len(ys)) == (960, 896, 5, 4)
    assert xs == [0, 760, 1520, 2280, 3040] and ys == [0, 701, 1402, 2104]
    tw, th, xs, ys = tiles.plan((700, 560), "auto", 64)
    assert (tw, th, xs, ys) == (512, 512, [0, 188], [0, 48])
    assert tiles.plan((1024, 768), "auto", 128) == (1024, 768, [0], [0])
    assert tiles.plan((1024, 768), "1024x768", 0) == (1024, 768, [0], [0])
    assert tiles.boxes(512, 512, [0, 188], [0, 48]) == [(0, 0, 512, 512), (188, 0, 700, 512), (0, 48, 512, 560), (188, 48, 700, 560)]
    for size in ((4000, 3000), (5999, 5999), (1025, 513)):                              # th * tw <= 1024^2 follows from the rules
        tw, th, _, _ = tiles.plan(size, "auto", 256)
        assert tw * th <= 1024 * 1024


def test_chunks():
    assert tiles.chunks(4, 3) == [[0, 1], [2, 3]]
    assert tiles.chunks(20, 8) == [[0, 1, 2, 3, 4, 5, 6], [7, 8, 9, 10, 11, 12, 13], [14, 15, 16, 17, 18, 19]]
    assert tiles.chunks(1, 16) == [[0]] and tiles.chunks(5, 1) == [[i] for i in range(5)]
    for n in range(1, 70):
        for k in range(1, 17):
            c = tiles.chunks(n, k)
            assert len(c) == -(-n // k) and [j for job in c for j in job] == list(range(n))
            sizes = {len(job) for job in c}
            assert max(sizes) <= k and max(sizes) - min(sizes) <= 1
    for bad in ((0, 1), (1, 0), (2.0, 1), (True, 1)):
        with pytest.raises(ValueError):
            tiles.chunks(*bad)


def test_check_and_plan_errors():
    assert tiles.check(None) == (None, 128, 4)
    assert tiles.check("auto", 0, 16) == ("auto", 0, 16) and tiles.check("AUTO", 256, 1) == ("auto", 256, 1)
    assert tiles.check((512, 640)) == ((512, 640), 128, 4) and tiles.check("512x640")[0] == (512, 640) and tiles.check([1024, 1024])[0] == (1024, 1024)
    for bad in ("tiles", "512", "512x", (512,), (512, 500), (448, 512), (2112, 512), (1024, 1088), (512.5, 512), (True, 512), 512, 3.0):
        with pytest.raises(ValueError, match="tiles"):
            tiles.check(bad)
    for bad in (-1, 257, 1.0, "64", None, True):
        with pytest.raises(ValueError, match="tile_overlap"):
            tiles.check("auto", bad)
        with pytest.raises(ValueError, match="tile_overlap"):                           # the rule holds with the feature off, too
            tiles.check(None, bad)
    for bad in (0, 17, 2.0, "4", None, True):
        with pytest.raises(ValueError, match="tile_batch"):
            tiles.check("auto", 128, bad)
    with pytest.raises(ValueError, match="no plan"):
        tiles.plan((1024, 1024), None)
    with pytest.raises(ValueError, match="width 511"):
        tiles.plan((511, 600), "auto")
    with pytest.raises(ValueError, match="height 300"):
        tiles.plan((600, 300), "auto")
    with pytest.raises(ValueError, match="width 1000 is below the tile's 1024"):
        tiles.plan((1000, 2000), (1024, 512))
    with pytest.raises(ValueError, match="height 600 is below the tile's 640"):
        tiles.plan((2000, 600), (512, 640))
    with pytest.raises(ValueError, match="at most 32"):                                 # 33 tiles of 512 at overlap 0
        tiles.plan((512 * 32 + 1, 512), (512, 512), 0)
    assert len(tiles.plan((512 * 32, 512), (512, 512), 0)[2]) == 32
    with pytest.raises(ValueError, match="at most 32"):
        tiles.plan((1024, 30000), "auto", 128)
    with pytest.raises(ValueError, match="tile_overlap"):
        tiles.plan((2000, 2000), "auto", 300)


def test_axis_weight():
    assert tiles.axis_weight(5, 0, 1).tolist() == [5] * 5                               # the only tile of its axis: nothing fades
    assert tiles.axis_weight(5, 0, 3).tolist() == [5, 4, 3, 2, 1]                       # the first: the far edge fades
    assert tiles.axis_weight(5, 2, 3).tolist() == [1, 2, 3, 4, 5]                       # the last: the near edge fades
    assert tiles.axis_weight(5, 1, 3).tolist() == [1, 2, 3, 2, 1] and tiles.axis_weight(4, 1, 3).tolist() == [1, 2, 2, 1]


def _random_tiles(seed, n, th, tw):
    return np.random.default_rng(seed).integers(0, 256, (n, th, tw, 3), dtype=np.uint8)


BLEND_CASES = [(29, 37, 12, 16, [0, 8, 17], [0, 10, 21]), (16, 26, 16, 16, [0], [0, 5, 10]), (12, 17, 12, 16, [0], [0, 1]), (8, 32, 8, 16, [0], [0, 16]),
               (40, 24, 24, 24, [0, 16], [0])]


@pytest.mark.parametrize("H,W,th,tw,ys,xs", BLEND_CASES)
def test_blend_numpy_properties(H, W, th, tw, ys, xs):
    t = _random_tiles(H * W, len(xs) * len(ys), th, tw)
    out = tiles.blend_numpy(t, xs, ys, H, W)
    assert out.shape == (H, W, 3) and out.dtype == np.uint8
    count = np.zeros((H, W), np.int64)
    lo, hi, only = np.full((H, W, 3), 255, np.uint8), np.zeros((H, W, 3), np.uint8), np.zeros((H, W, 3), np.uint8)
    for j, (l, tp, r, b) in enumerate(tiles.boxes(tw, th, xs, ys)):
        count[tp:b, l:r] += 1
        lo[tp:b, l:r] = np.minimum(lo[tp:b, l:r], t[j])
        hi[tp:b, l:r] = np.maximum(hi[tp:b, l:r], t[j])
        only[tp:b, l:r] = t[j]
    assert count.min() >= 1 and (count == 1).any()
    assert np.array_equal(out[count == 1], only[count == 1])                            # one covering tile: its byte
    assert (out >= lo).all() and (out <= hi).all()                                      # between the covering tiles' minimum and maximum
    if count.max() > 1:
        assert not np.array_equal(out[count > 1], only[count > 1])                      # and the overlaps are really mixed
    src = np.random.default_rng(7).integers(0, 256, (H, W, 3), dtype=np.uint8)          # a source's own crops reproduce it exactly
    crops = np.stack([src[tp:b, l:r] for l, tp, r, b in tiles.boxes(tw, th, xs, ys)])
    assert np.array_equal(tiles.blend_numpy(crops, xs, ys, H, W), src)


def test_blend_numpy_is_a_linear_crossfade():
    """Two 8-wide tiles 4 apart, black and white: across the 4 shared columns the weights are (4, 1), (3, 2), (2, 3), (1, 4) fifths."""
    t = np.zeros((2, 1, 8, 3), np.uint8)
    t[1] = 255
    out = tiles.blend_numpy(t, [0, 4], [0], 1, 12)[0, :, 0].tolist()
    assert out == [0, 0, 0, 0, 51, 102, 153, 204, 255, 255, 255, 255]


def test_blend_numpy_largest_numerator():
    """Three 1024-tiles per axis over 2047 pixels, all bytes 255: the largest numerator the plans reach stays far below 2^32 (the device op's
    32-bit accumulator; csrc/tile_blend.hip derives the bound)."""
    pos = [0, 511, 1023]
    num = np.zeros(2047, np.int64)
    for i, p in enumerate(pos):
        num[p:p + 1024] += tiles.axis_weight(1024, i, 3)
    s = int(num.max()) ** 2
    assert s * 255 + (s >> 1) == 267_386_880 + (s >> 1) and s * 256 < 2 ** 32


def test_blend_numpy_errors():
    t = _random_tiles(0, 2, 8, 16)
    for xs, W in (([1, 16], 32), ([0, 17], 33), ([0, 16], 33), ([0, 0], 16), ([16, 0], 32), ([], 16), ([0, 8.0], 24), (None, 16)):
        with pytest.raises(ValueError, match="xs"):
            tiles.blend_numpy(t, xs, [0], 8, W)
    with pytest.raises(ValueError, match="ys"):
        tiles.blend_numpy(t, [0, 16], [1], 9, 32)
    with pytest.raises(ValueError, match="grid"):
        tiles.blend_numpy(t, [0, 8, 16], [0], 8, 32)
    with pytest.raises(ValueError, match="uint8"):
        tiles.blend_numpy(t.astype(np.int32), [0, 16], [0], 8, 32)


def test_cli_flags():
    import run_batch
    import run_single_image
    for mod in (run_batch, run_single_image):
        base = {a.option_strings[0] for a in mod.build_parser()._actions if a.option_strings}
        assert not {"--tiles", "--tile_overlap", "--tile_batch"} & base                  # kept apart from build_parser()
    p = run_batch.add_tile_args(run_batch.add_region_args(run_batch.add_resolution_args(run_batch.build_parser())))
    a = p.parse_args([])
    assert (a.tiles, a.tile_overlap, a.tile_batch) == (None, 128, 4) and run_batch.tile_kwargs(a) == {}
    a = p.parse_args(["--tiles", "auto", "--tile_overlap", "64", "--tile_batch", "2"])
    assert run_batch.tile_kwargs(a) == dict(tiles="auto", tile_overlap=64, tile_batch=2)
    assert run_batch.tile_kwargs(p.parse_args(["--tiles", "640x512"]))["tiles"] == (640, 512)
    for bad in (["--tiles", "500x512"], ["--tiles", "big"], ["--tile_overlap", "257"], ["--tile_batch", "0"]):
        with pytest.raises(SystemExit):
            p.parse_args(bad)
    for clash in (["--resolution", "auto"], ["--region", "mask"]):
        with pytest.raises(ValueError, match="--tiles with"):
            run_batch.tile_kwargs(p.parse_args(["--tiles", "auto"] + clash))
    with pytest.raises(SystemExit):
        run_batch.main(["--tiles", "auto", "--resolution", "auto"])
    res = run_batch._process_entries(None, [], p.parse_args(["--tiles", "auto"]), "e", "c")
    assert res["processed"] == 0 and res["failed"] == 0


def test_run_single_image_flags(tmp_path, capsys):
    import run_single_image
    one = ["--image", str(tmp_path / "missing.png"), "--prompt", "p", "--output_dir", str(tmp_path / "out")]
    for clash in (["--resolution", "auto"], ["--region", "mask", "--mask", "m.png"], ["--outpaint", "0,0,64,0"]):
        with pytest.raises(SystemExit):
            run_single_image.main(one + ["--tiles", "auto"] + clash)
        capsys.readouterr()
    assert run_single_image.main(one + ["--tiles", "640x512", "--tile_overlap", "0", "--tile_batch", "16"]) is None
    assert "Image not found" in capsys.readouterr().out


def test_entry_in_header_signature_and_library():
    hip.build()
    text = open(os.path.join(ROOT, "include", "fie.h")).read()
    declared = set(re.findall(r"\b(fie_[a-z0-9_]+)\s*\(", text))
    lib = hip.lib()
    vp, i = ctypes.c_void_p, ctypes.c_int
    assert "fie_tile_blend_rgb_u8" in declared, "fie_tile_blend_rgb_u8 missing from include/fie.h"
    args = [vp, vp, i, i, vp, vp, i, i, i, i, vp]
    assert hip.SIGNATURES["fie_tile_blend_rgb_u8"] == args
    fn = lib.fie_tile_blend_rgb_u8                                                      # exported by libfie_hip.so
    assert fn.restype is i and list(fn.argtypes) == args
    with pytest.raises(hip.FieError):                                                   # argument checks run before any launch
        hip._chk(fn(None, None, 1, 1, None, None, 8, 8, 8, 8, None))
    assert b"NULL argument" in lib.fie_last_error()


def test_editor_signatures_carry_the_keywords():
    import inspect
    from src.pipeline import FastEditor
    for fn in (FastEditor.edit, FastEditor.edit_batch):
        ps = inspect.signature(fn).parameters
        for name, default in (("tiles", None), ("tile_overlap", 128), ("tile_batch", 4)):
            assert ps[name].kind is inspect.Parameter.KEYWORD_ONLY and ps[name].default == default
