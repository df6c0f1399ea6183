"""Full-resolution edits on the device: the fused back end (csrc/fullres.hip through ctx.fullres_paste) against Pillow and
the numpy restatement (fie_amd/region.py), then the product surfaces: edit(output_size="source"), region edits, batches, inline metrics, run_batch.

Bounds of the kernel checks: the LANCZOS resize is integer arithmetic, so everything that is not a blend is exact -- the whole image without a mask or
with r = 0, and every pixel where the restated feather is 0 (the source's byte).  Where the feather is positive the device contracts m * d + (1 - m) * s
into fused multiply-adds and the restatement does not: the two can differ only at a rounding tie of the final rint, one u8 level (the bound of the
edit-size composite, tests/test_masked_edit_gpu.py)."""
import json

import numpy as np
import pytest
import torch
from PIL import Image

import metrics_oracle as mo

pytestmark = pytest.mark.gpu

SHAPES = [((48, 64), (131, 173)),        # up, odd sizes, several tiles on both axes, a partial last tile
          ((80, 96), (50, 70)),          # down
          ((64, 64), (64, 150)),         # one axis kept: no vertical pass
          ((40, 56), (40, 56))]          # no resample at all
BLURS = [0.0, 1.0, 21.0]                 # 21: radius 63, larger than every image here (the halo is all clamped border)
RES = (512, 512)


def _masks(H, W, seed):
    rng = np.random.default_rng(seed)
    box = np.zeros((H, W), np.uint8)
    box[H // 4:H // 4 + H // 3, W // 5:W // 5 + W // 2] = 255
    rnd = (rng.random((H, W)) < 0.5).astype(np.uint8) * 255
    rnd[H // 3:H // 3 + 12, W // 3:W // 3 + 20] = rng.integers(90, 171, (12, 20), dtype=np.uint8)      # grey levels either side of the threshold
    return {"zero": np.zeros((H, W), np.uint8), "one": np.full((H, W), 255, np.uint8), "box": box, "random": rnd}


def _case(hw, HW):
    rng = np.random.default_rng(hw[0] * 131 + HW[1])
    return rng.integers(0, 256, hw + (3,), dtype=np.uint8), rng.integers(0, 256, HW + (3,), dtype=np.uint8)


def _dev(fie, a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(fie.device)


@pytest.mark.parametrize("blur", BLURS)
@pytest.mark.parametrize("hw,HW", SHAPES)
def test_kernel_matches_the_restatement(fie, hw, HW, blur):
    from fie_amd import mask as hmask
    from fie_amd import region
    d, src = _case(hw, HW)
    for name, mask in _masks(*HW, seed=hw[1]).items():
        got = fie.fullres_paste(_dev(fie, d), _dev(fie, src), _dev(fie, mask), blur).cpu().numpy()
        want = region.fullres_paste_numpy(d, src, mask, blur)
        m = hmask.feather_numpy(mask >= 128, blur)
        diff = np.abs(got.astype(int) - want.astype(int))
        print(f"[fullres] {hw}->{HW} r={blur} {name}: max diff {diff.max()}, differing bytes {(diff > 0).sum()}, feather 0 on {(m == 0).mean():.2f}")
        assert got.shape == src.shape and got.dtype == np.uint8
        assert np.array_equal(got[m == 0], src[m == 0]), name                 # untouched where the feather is 0
        if blur == 0:
            assert np.array_equal(got, want), name
            up = Image.fromarray(d).resize((HW[1], HW[0]), Image.LANCZOS)
            pil = Image.composite(up, Image.fromarray(src), Image.fromarray((mask >= 128).astype(np.uint8) * 255))
            assert np.array_equal(got, np.asarray(pil)), name
        assert diff.max() <= 1, name
        if name == "zero":
            assert np.array_equal(got, src)


@pytest.mark.parametrize("hw,HW", SHAPES)
def test_no_mask_is_pillows_resize(fie, hw, HW):
    d, src = _case(hw, HW)
    got = fie.fullres_paste(_dev(fie, d), _dev(fie, src)).cpu().numpy()
    assert np.array_equal(got, np.asarray(Image.fromarray(d).resize((HW[1], HW[0]), Image.LANCZOS)))


@pytest.mark.parametrize("blur", [0.0, 1.0])
def test_pitched_region_inside_a_larger_image(fie, blur):
    """source / dst / mask are views into larger images at a byte offset that is no multiple of 4, with an odd pitch (so the rows' alignment
    takes every value): the region is right and every byte outside it keeps its sentinel.  Then in place: dst is the source view."""
    from fie_amd import region
    (h, w), (H, W) = (48, 64), (131, 173)
    d, src = _case((h, w), (H, W))
    mask = _masks(H, W, 3)["random"]
    want = region.fullres_paste_numpy(d, src, mask, blur)
    HB, WB, top, left = 150, 211, 7, 5
    assert ((top * WB + left) * 3) % 4 != 0 and (WB * 3) % 4 != 0
    src_big = torch.full((HB, WB, 3), 0x5A, dtype=torch.uint8, device=fie.device)
    dst_big = torch.full((HB, WB, 3), 0xA5, dtype=torch.uint8, device=fie.device)
    mask_big = torch.full((HB, WB), 0xFF, dtype=torch.uint8, device=fie.device)         # white outside the view: a read past the view would show
    src_big[top:top + H, left:left + W] = _dev(fie, src)
    mask_big[top:top + H, left:left + W] = _dev(fie, mask)
    sv, dv, mv = (t[top:top + H, left:left + W] for t in (src_big, dst_big, mask_big))
    assert sv.data_ptr() % 4 != 0 and dv.data_ptr() % 4 != 0
    out = fie.fullres_paste(_dev(fie, d), sv, mv, blur, out=dv)
    assert out.data_ptr() == dv.data_ptr()
    big = dst_big.cpu().numpy()
    roi = big[top:top + H, left:left + W]
    assert np.abs(roi.astype(int) - want.astype(int)).max() <= (0 if blur == 0 else 1)
    outside = np.ones((HB, WB), bool)
    outside[top:top + H, left:left + W] = False
    assert (big[outside] == 0xA5).all()
    fie.fullres_paste(_dev(fie, d), sv, mv, blur, out=sv)                                # in place inside the source's own image
    big2 = src_big.cpu().numpy()
    assert np.array_equal(big2[top:top + H, left:left + W], roi) and (big2[outside] == 0x5A).all()


def test_bad_arguments_fail_loudly(fie):
    d, src = _case((48, 64), (131, 173))
    with pytest.raises(ValueError):
        fie.fullres_paste(_dev(fie, d), _dev(fie, src), _dev(fie, np.zeros((131, 172), np.uint8)))
    with pytest.raises(ValueError):
        fie.fullres_paste(_dev(fie, d), _dev(fie, src), out=torch.empty((131, 173, 4), dtype=torch.uint8, device=fie.device)[..., :3])


# ------------------------------------------------------------------------------------------------------------------------ product surfaces
@pytest.fixture(scope="module")
def editor(fie):
    from src.pipeline import FastEditor
    return FastEditor(model_name="tiny", enable_cpu_offload=False)


def _box_mask(W, H, x0, x1, y0, y1):
    m = np.zeros((H, W), np.uint8)
    m[y0:y1, x0:x1] = 255
    return m


def test_edit_at_the_sources_size(editor, fie):
    from fie_amd import mask as hmask
    img = Image.fromarray(mo.textured(51, 150, 200))
    mask = _box_mask(200, 150, 60, 140, 40, 110)
    kw = dict(seed=9, strength=0.6, resolution=RES)
    out = editor.edit(img, "a [red] kite", mask=mask, mask_blur=2, output_size="source", **kw)
    assert isinstance(out, Image.Image) and out.size == img.size and out.mode == "RGB"
    got, src = np.asarray(out), np.asarray(img)
    m = hmask.feather_numpy(mask >= 128, 2.0)
    assert np.array_equal(got[m == 0], src[m == 0]) and 0.3 < (m == 0).mean() < 0.9
    inside = m > 0.99                                    # the f32 taps sum to 1 - 2^-24 or so: the interior is a blend a hair from the result
    assert inside.any() and not np.array_equal(got[inside], src[inside])
    d = editor.edit(img, "a [red] kite", mask=mask, paste_back=False, **kw)               # the edit-size result before any paste-back
    assert d.size == RES
    want = fie.fullres_paste(_dev(fie, np.asarray(d)), _dev(fie, src), _dev(fie, mask), 2.0).cpu().numpy()
    assert np.array_equal(got, want)
    # without a mask, and with paste_back off: Pillow's resize of the edit-size result
    plain = editor.edit(img, "a [red] kite", **kw)
    assert plain.size == RES                                                              # the default is unchanged
    up = editor.edit(img, "a [red] kite", output_size="source", **kw)
    assert np.array_equal(np.asarray(up), np.asarray(plain.resize(img.size, Image.LANCZOS)))
    nopaste = editor.edit(img, "a [red] kite", mask=mask, paste_back=False, output_size="source", **kw)
    assert np.array_equal(np.asarray(nopaste), np.asarray(d.resize(img.size, Image.LANCZOS)))
    assert np.array_equal(np.asarray(editor.edit(img, "a [red] kite", output_size="edit", **kw)), np.asarray(plain))


@pytest.mark.parametrize("region", ["mask", (37, 21, 250, 190)])
def test_region_edit_is_the_crop_edit_pasted_into_the_source(editor, region):
    from fie_amd import region as hregion
    img = Image.fromarray(mo.textured(52, 240, 320))
    mask = _box_mask(320, 240, 101, 171, 60, 133)
    kw = dict(seed=4, strength=0.6, resolution=RES, mask=None, mask_blur=1.5)
    out = editor.edit(img, "a [blue] ball", region=region, region_padding=20, **dict(kw, mask=mask))
    box = hregion.resolve(region, img.size, mask, 20, RES)
    if region == "mask":
        assert box == (80, 40, 193, 153)                     # 70 x 73, + 20 each side = 110 x 113, widened to the square 113 x 113
    l, t, r, b = box
    crop = editor.edit(img.crop(box), "a [blue] ball", output_size="source", **dict(kw, mask=Image.fromarray(mask).crop(box)))
    assert crop.size == (r - l, b - t)
    want = np.asarray(img).copy()
    want[t:b, l:r] = np.asarray(crop)
    got = np.asarray(out)
    assert out.size == img.size and np.array_equal(got, want)
    outside = np.ones((240, 320), bool)
    outside[t:b, l:r] = False
    assert np.array_equal(got[outside], np.asarray(img)[outside])
    assert not np.array_equal(got[mask >= 128], np.asarray(img)[mask >= 128])


def test_region_argument_errors(editor):
    img = Image.fromarray(mo.textured(53, 64, 64))
    with pytest.raises(ValueError, match="needs a mask"):
        editor.edit(img, "p", region="mask")
    with pytest.raises(ValueError, match="output_size"):
        editor.edit(img, "p", region=(0, 0, 32, 32), output_size="edit")
    with pytest.raises(ValueError, match="selects nothing"):
        editor.edit(img, "p", region="mask", mask=np.zeros((64, 64), np.uint8))
    with pytest.raises(ValueError):
        editor.edit(img, "p", output_size="full")


def test_edit_batch_with_a_region_an_unmasked_and_a_masked_image(editor, fie):
    from fie_amd import region as hregion
    imgs = [Image.fromarray(mo.textured(60, 200, 300)), Image.fromarray(mo.textured(61, 120, 160)), Image.fromarray(mo.textured(62, 128, 128))]
    prompts = [f"a [toy] number {i}" for i in range(3)]
    masks = [_box_mask(300, 200, 120, 200, 50, 120), None, _box_mask(128, 128, 30, 100, 20, 90)]
    kw = dict(seed=11, strength=0.5, resolution=RES)
    outs = editor.edit_batch(imgs, prompts, masks=masks, mask_blur=1.5, region=["mask", None, None], region_padding=16, output_size="source", **kw)
    assert [o.size for o in outs] == [im.size for im in imgs]                              # input order, every image at its source's size
    box = hregion.mask_box(masks[0], 16, RES)
    crops = [imgs[0].crop(box), imgs[1], imgs[2]]
    cmasks = [masks[0][box[1]:box[3], box[0]:box[2]], None, masks[2]]
    raw = editor.edit_batch(crops, prompts, masks=cmasks, paste_back=False, **kw)          # the batch's own edit-size results
    for i, (im, c, cm, d, out) in enumerate(zip(imgs, crops, cmasks, raw, outs)):
        assert d.size == RES
        want = fie.fullres_paste(_dev(fie, np.asarray(d)), _dev(fie, np.asarray(c)), None if cm is None else _dev(fie, cm), 1.5 if cm is not None else 0.0)
        full = np.asarray(im).copy()
        if i == 0:
            full[box[1]:box[3], box[0]:box[2]] = want.cpu().numpy()
        else:
            full = want.cpu().numpy()
        assert np.array_equal(np.asarray(out), full), i
    assert np.array_equal(np.asarray(outs[1]), np.asarray(raw[1].resize(imgs[1].size, Image.LANCZOS)))


@pytest.fixture(scope="module")
def tol():
    return 4 * mo.d0(mo.pair_set())                # the SSIM bound of tests/test_metrics_gpu.py


def _close(m, want, tol, keys):                    # the tolerances of tests/test_metrics_gpu.py
    for k in keys:
        if k.endswith("mse"):
            assert abs(m[k] - want[k]) <= 1e-6 * want[k] + 1e-12, (k, m[k], want[k])
        elif k.endswith("psnr"):
            assert abs(m[k] - want[k]) <= 1e-4, (k, m[k], want[k])
        else:
            assert abs(m[k] - want[k]) <= tol, (k, m[k], want[k])


def test_metrics_score_the_source_size_output(editor, tol):
    from src.metrics import MetricsCalculator
    img = Image.fromarray(mo.textured(54, 300, 420))
    mask = _box_mask(420, 300, 100, 300, 80, 220)
    kw = dict(seed=42, strength=0.6, resolution=RES, mask=mask, mask_blur=1.0, output_size="source")
    out, m = editor.edit(img, "a [green] door", metrics=True, **kw)
    assert out.size == img.size and np.array_equal(np.asarray(out), np.asarray(editor.edit(img, "a [green] door", **kw)))
    keys = ("ssim", "psnr", "mse", "bg_ssim", "bg_psnr", "bg_mse")
    assert set(m) == set(keys)
    ra, rb = np.asarray(img.resize((512, 512), Image.LANCZOS)), np.asarray(out.resize((512, 512), Image.LANCZOS))
    assert m["mse"] == mo.sse(ra, rb) / (65025.0 * ra.size)
    _close(m, MetricsCalculator("cpu").calculate_all_metrics(img, out, "a [green] door", mask=mask), tol, keys)
    assert m["bg_mse"] < m["mse"]
    # a region edit scores the crop and its output
    out_r, m_r = editor.edit(img, "a [green] door", metrics=True, region="mask", **dict(kw, output_size=None))
    from fie_amd import region as hregion
    box = hregion.mask_box(mask, 32, RES)
    want = MetricsCalculator("cpu").calculate_all_metrics(img.crop(box), out_r.crop(box), "a [green] door", mask=mask[box[1]:box[3], box[0]:box[2]])
    _close(m_r, want, tol, keys)


def test_run_batch_region_mask_end_to_end(editor, tmp_path):
    import run_batch
    from fie_amd import mask as hmask
    from tools import make_synthetic_piebench as msp
    data = tmp_path / "pie"
    msp.main(["--out", str(data), "--num", "2", "--with_masks"])
    mapping = json.load(open(data / "mapping_file.json"))
    entries = [(i, k, e) for i, (k, e) in enumerate(mapping.items())]
    out = tmp_path / "out"
    parser = run_batch.add_region_args(run_batch.add_resolution_args(run_batch.add_mask_args(run_batch.build_parser())))
    args = parser.parse_args(["--source_dir", str(data / "annotation_images"), "--output_dir", str(out), "--seed", "42", "--strength", "0.5",
                              "--use_mask", "--region", "mask", "--resolution", "512x512"])
    args.resolution = RES
    r = run_batch.process_shard(editor, entries, args, str(out / "e"), str(out / "c"))
    assert (r["processed"], r["skipped"], r["failed"]) == (2, 0, 0)
    for k, e in mapping.items():
        src = Image.open(data / "annotation_images" / e["image_path"]).convert("RGB")
        got = np.asarray(Image.open(out / "e" / e["image_path"]).convert("RGB")).astype(int)
        m = hmask.rle_decode(e["mask"], (src.height, src.width))
        want = np.asarray(editor.edit(src, e["editing_prompt"], seed=42, strength=0.5, mask=m, region="mask", resolution=RES)).astype(int)
        assert got.shape == (src.height, src.width, 3) and np.abs(got - want).mean() < 4.0       # a JPEG round trip apart
