"""Host side of full-resolution edits (fie_amd/region.py), without a GPU: the box rule of region="mask" on pinned
answers, the argument rules, the numpy restatement of the device back end against Pillow, and the command-line flags."""
import numpy as np
import pytest
from PIL import Image

import fie_amd  # noqa: F401
from fie_amd import buckets, region


def _mask(w, h, x0, x1, y0, y1, value=255):
    m = np.zeros((h, w), np.uint8)
    m[y0:y1, x0:x1] = value
    return m


@pytest.mark.parametrize("sel,box", [((100, 180, 120, 160), (90, 90, 190, 190)),        # grows the short axis, centred
                                     ((0, 50, 0, 20), (0, 0, 60, 60)),                  # clipped at the corner, shifted back inside
                                     ((10, 390, 100, 200), (0, 0, 400, 300))])          # wider than the image is high: capped at the image
def test_mask_box_known_answers(sel, box):
    assert region.mask_box(_mask(400, 300, *sel), padding=10) == box
    assert region.resolve("mask", (400, 300), _mask(400, 300, *sel), 10, None) == box


def test_mask_box_threshold_padding_and_auto_bucket():
    m = _mask(400, 300, 100, 180, 120, 160, value=127)              # below the threshold everywhere but one pixel block
    m[130:150, 110:170] = 128
    assert region.mask_box(m, padding=0) == (110, 110, 170, 170)
    assert region.mask_box(m, padding=1000) == (0, 0, 400, 300)     # padded box = the image: a box only grows, capped at the image
    # "auto": the bucket comes from the PADDED box (400 x 120 -> 1536x640, the widest), then the height grows to its aspect
    wide = _mask(400, 300, 10, 390, 100, 200)
    assert buckets.target_size("auto", (400, 120)) == (1536, 640)
    assert region.mask_box(wide, padding=10, resolution="auto") == (0, 67, 400, 234)           # want_h = ceil(400 * 640 / 1536) = 167
    tall = _mask(300, 400, 140, 160, 20, 380)
    assert buckets.target_size("auto", (40, 380)) == (640, 1536)
    l, t, r, b = region.mask_box(tall, padding=10, resolution="auto")
    assert (t, b) == (10, 390) and r - l == -(-380 * 640 // 1536) and l <= 130 and r >= 170
    assert region.mask_box(wide, padding=10, resolution=(1024, 512)) == (0, 50, 400, 250)


def test_explicit_box_passes_through_and_is_validated():
    assert region.resolve((3, 5, 40, 90), (400, 300)) == (3, 5, 40, 90)
    assert region.resolve([0, 0, 400, 300], (400, 300), None) == (0, 0, 400, 300)
    assert region.resolve((3, 5, 40, 90), (400, 300), _mask(400, 300, 0, 9, 0, 9)) == (3, 5, 40, 90)      # the mask does not move an explicit box
    assert region.resolve(None, (400, 300)) is None
    for bad in ((0, 0, 401, 300), (-1, 0, 40, 40), (50, 0, 50, 40), (0, 40, 30, 20), (0, 0, 15, 300), (0, 0, 400, 15), (0, 0, 16.5, 40), (1, 2, 3)):
        with pytest.raises(ValueError):
            region.resolve(bad, (400, 300))
    with pytest.raises(ValueError):
        region.resolve("face", (400, 300), _mask(400, 300, 0, 50, 0, 50))


def test_region_value_errors():
    with pytest.raises(ValueError, match="selects nothing"):
        region.mask_box(_mask(400, 300, 0, 50, 0, 50, value=127))
    with pytest.raises(ValueError, match="needs a mask"):
        region.resolve("mask", (400, 300), None)
    with pytest.raises(ValueError, match="at least 16|below 16"):
        region.mask_box(_mask(12, 300, 2, 8, 100, 110), padding=1)            # the image itself is 12 wide: the side cannot reach 16
    with pytest.raises(ValueError):
        region.mask_box(_mask(400, 300, 0, 50, 0, 50), padding=-1)
    assert region.check_output(None, None) is False and region.check_output("edit", None) is False
    assert region.check_output("source", None) is True and region.check_output(None, "mask") is True and region.check_output("source", (0, 0, 20, 20)) is True
    with pytest.raises(ValueError):
        region.check_output("edit", "mask")
    with pytest.raises(ValueError):
        region.check_output("full", None)
    with pytest.raises(ValueError):
        region.check_output((512, 512), None)


SHAPES = [((48, 64), (131, 173)), ((80, 96), (50, 70)), ((64, 64), (64, 150)), ((40, 56), (40, 56))]


@pytest.mark.parametrize("hw,HW", SHAPES)
def test_numpy_back_end_equals_pillow_composite_for_binary_masks(hw, HW):
    """r = 0: Pillow is the oracle -- LANCZOS resize, then Image.composite through the binary mask."""
    rng = np.random.default_rng(hw[0] * 1000 + HW[1])
    d = rng.integers(0, 256, hw + (3,), dtype=np.uint8)
    src = rng.integers(0, 256, HW + (3,), dtype=np.uint8)
    mask = rng.integers(0, 256, HW, dtype=np.uint8)
    up = Image.fromarray(d).resize((HW[1], HW[0]), Image.LANCZOS)
    assert np.array_equal(region.fullres_paste_numpy(d, src), np.asarray(up))
    binary = (mask >= 128).astype(np.uint8) * 255
    want = np.asarray(Image.composite(up, Image.fromarray(src), Image.fromarray(binary)))
    assert np.array_equal(region.fullres_paste_numpy(d, src, mask, 0.0), want)
    assert np.array_equal(region.fullres_paste_numpy(d, src, np.zeros(HW, np.uint8), 3.0), src)
    assert np.array_equal(region.fullres_paste_numpy(d, src, np.full(HW, 255, np.uint8), 0.0), np.asarray(up))


def test_numpy_back_end_feathered_is_the_blend():
    from fie_amd import mask as hmask
    rng = np.random.default_rng(5)
    d = rng.integers(0, 256, (32, 40, 3), dtype=np.uint8)
    src = rng.integers(0, 256, (70, 90, 3), dtype=np.uint8)
    mask = _mask(90, 70, 20, 60, 15, 50)
    out = region.fullres_paste_numpy(d, src, mask, 2.0)
    m = hmask.feather_numpy(mask >= 128, 2.0)
    up = np.asarray(Image.fromarray(d).resize((90, 70), Image.LANCZOS))
    assert np.array_equal(out[m == 0], src[m == 0]) and (m == 0).any() and ((m > 0) & (m < 1)).any()
    lo, hi = np.minimum(up, src).astype(int), np.maximum(up, src).astype(int)
    assert ((out >= lo) & (out <= hi)).all()                              # a convex combination, rounded
    mid = (m > 0.4) & (m < 0.6)
    assert np.abs(out[mid].astype(float) - (up[mid].astype(float) + src[mid]) / 2).max() <= 0.1 * 255 + 1


def test_paste_returns_an_rgb_copy_with_the_crop_in_place():
    src = Image.fromarray(np.random.default_rng(1).integers(0, 256, (30, 40, 4), dtype=np.uint8), "RGBA")
    crop = Image.fromarray(np.full((10, 12, 3), 7, np.uint8))
    out = region.paste(src, crop, (5, 6, 17, 16))
    a, want = np.asarray(out), np.asarray(src.convert("RGB")).copy()
    want[6:16, 5:17] = 7
    assert out.mode == "RGB" and np.array_equal(a, want) and src.mode == "RGBA"


def test_cli_flags():
    import run_batch
    import run_single_image
    flags = lambda p: {a.option_strings[0] for a in p._actions if a.option_strings}
    new = {"--output_size", "--region", "--region_padding"}
    assert flags(run_batch.add_region_args(run_batch.build_parser())) - flags(run_batch.build_parser()) == new
    assert not new & flags(run_batch.build_parser())                       # build_parser's flag set stays the reference's + earlier additions
    p = run_batch.add_region_args(run_batch.add_mask_args(run_batch.build_parser()))
    a = p.parse_args([])
    assert (a.output_size, a.region, a.region_padding) == ("edit", "none", 32) and run_batch.region_kwargs(a, False) == {}
    a = p.parse_args(["--use_mask", "--region", "mask", "--region_padding", "8"])
    assert run_batch.region_kwargs(a, a.use_mask) == {"region": "mask", "region_padding": 8}
    assert run_batch.region_kwargs(p.parse_args(["--output_size", "source"]), False) == {"output_size": "source"}
    with pytest.raises(ValueError, match="--use_mask"):
        run_batch.region_kwargs(p.parse_args(["--region", "mask"]), False)
    assert run_batch.region_kwargs(run_batch.build_parser().parse_args([]), False) == {}      # a parser without the flags: today's call
    for bad in (["--region", "box"], ["--output_size", "1024"]):
        with pytest.raises(SystemExit):
            p.parse_args(bad)
    with pytest.raises(SystemExit):
        run_batch.main(["--region", "mask"])                              # refused before anything is loaded
    s = run_single_image.build_parser()
    assert new <= flags(s)
    a = s.parse_args(["--image", "i.png", "--prompt", "p", "--mask", "m.png", "--region", "mask", "--region_padding", "5", "--output_size", "source"])
    assert (a.region, a.region_padding, a.output_size) == ("mask", 5, "source")
    with pytest.raises(SystemExit):
        run_single_image.main(["--image", "i.png", "--prompt", "p", "--region", "mask"])
