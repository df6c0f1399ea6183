"""Tiled edits on the device: fie_tile_blend_rgb_u8 byte for byte against the numpy restatement (fie_amd/tiles.py:
blend_numpy) at every alignment, inside guard bands and against every malformed position list, then the defining identity on FastEditor (tiny
stack, 512-pixel tiles: the smallest legal): a tiled edit is the blend of edit_batch's results on the tiles' crops.  Every comparison is a bit
equality: all of it is integer arithmetic."""
import numpy as np
import pytest
import torch
from PIL import Image

import mask_grow_oracle as mgo
import metrics_oracle as mo
from isolation import flat, isolated

import fie_amd  # noqa: F401
from fie_amd import tiles

pytestmark = pytest.mark.gpu


def _dev(fie, a):
    return torch.from_numpy(np.array(a, order="C")).to(fie.device)


def _even(S, t, n):
    return [0] if n == 1 else [(i * (S - t)) // (n - 1) for i in range(n)]


def _random(seed, n, th, tw):
    return np.random.default_rng(seed).integers(0, 256, (n, th, tw, 3), dtype=np.uint8)


# ------------------------------------------------------------------------------------------------------------------------ the op
# (H, W, th, tw, ys, xs).  One tile that is the image; a 3 x 3 grid with odd sizes; rows of 3 W bytes with every residue mod 4 (W = 61 .. 64), so
# a row's head and tail take every length; three tiles over one pixel; neighbours one pixel apart; abutting tiles that share nothing; the same
# with the axes exchanged; rows longer than one block of 256 dwords with a seam inside a block and one on a block's edge.
ROW_CASES = [(12, 16, 12, 16, [0], [0]),
             (29, 37, 12, 16, _even(29, 12, 3), _even(37, 16, 3))] \
    + [(24, W, 24, 24, [0], _even(W, 24, 4)) for W in (61, 62, 63, 64)] \
    + [(16, 26, 16, 16, [0], [0, 5, 10]), (16, 17, 16, 16, [0], [0, 1]), (16, 32, 16, 16, [0], [0, 16])]
CASES = ROW_CASES + [(W, H, tw, th, xs, ys) for H, W, th, tw, ys, xs in ROW_CASES[2:]] \
    + [(9, 700, 7, 400, [0, 2], [0, 300]), (5, 1024, 5, 683, [0], [0, 341])]


def _id(c):
    return f"{c[0]}x{c[1]}-t{c[2]}x{c[3]}-y{'.'.join(map(str, c[4]))}-x{'.'.join(map(str, c[5]))}"


@pytest.mark.parametrize("case", CASES, ids=_id)
def test_op_matches_the_restatement(fie, case):
    H, W, th, tw, ys, xs = case
    t = _random(H * 1000 + W, len(xs) * len(ys), th, tw)
    t_dev = _dev(fie, t)
    want = tiles.blend_numpy(t, xs, ys, H, W)
    got = fie.tile_blend(t_dev, xs, ys, H, W)
    bad = np.argwhere(got.cpu().numpy() != want)
    assert got.shape == (H, W, 3) and got.dtype == torch.uint8 and bad.size == 0, (len(bad), bad[:4].tolist())
    out = torch.full((H, W, 3), 0x5A, dtype=torch.uint8, device=fie.device)               # an output of the caller's
    assert fie.tile_blend(t_dev, tuple(xs), np.asarray(ys), H, W, out=out) is out and np.array_equal(out.cpu().numpy(), want)
    assert np.array_equal(t_dev.cpu().numpy(), t)                                          # the operand is unchanged
    src = np.random.default_rng(5).integers(0, 256, (H, W, 3), dtype=np.uint8)             # a source's own crops reproduce it
    crops = np.stack([src[tp:b, l:r] for l, tp, r, b in tiles.boxes(tw, th, xs, ys)])
    assert np.array_equal(fie.tile_blend(_dev(fie, crops), xs, ys, H, W).cpu().numpy(), src)


@pytest.mark.parametrize("fill", ["255", "random"])
def test_op_at_the_accumulators_worst_case(fie, fill):
    """2047 x 2047 from three 1024-tiles per axis at 0, 511, 1023: the largest numerator a plan reaches (267 386 880 with all bytes 255), on the
    32-bit kernel."""
    pos = [0, 511, 1023]
    t = np.full((9, 1024, 1024, 3), 255, np.uint8) if fill == "255" else _random(77, 9, 1024, 1024)
    got = fie.tile_blend(_dev(fie, t), pos, pos, 2047, 2047).cpu().numpy()
    assert np.array_equal(got, tiles.blend_numpy(t, pos, pos, 2047, 2047))
    if fill == "255":
        assert (got == 255).all()


def test_op_on_64_bit_accumulators(fie):
    """32 tiles of 4 x 131072 one pixel apart: 32 tiles share a pixel, so the host's bound on the weight sum (32 * 131072 * 4 = 2^24) sends the
    call to the 64-bit kernel."""
    th, tw, xs = 4, 1 << 17, list(range(32))
    W = tw + 31
    t = _random(78, 32, th, tw)
    got = fie.tile_blend(_dev(fie, t), xs, [0], th, W).cpu().numpy()
    assert np.array_equal(got, tiles.blend_numpy(t, xs, [0], th, W))


@pytest.mark.parametrize("off", [1, 2, 3])
def test_op_at_every_alignment_of_its_output(fie, off):
    """The split of a row into head, dwords and tail follows its ADDRESS: an output that starts 1, 2 and 3 bytes past a dword boundary, the
    bytes on either side of it checked."""
    H, W, th, tw, ys, xs = 29, 37, 12, 16, _even(29, 12, 3), _even(37, 16, 3)
    t = _random(off, 9, th, tw)
    buf = torch.full((H * W * 3 + 8,), 0xA5, dtype=torch.uint8, device=fie.device)
    assert buf.data_ptr() % 4 == 0
    out = buf[off:off + H * W * 3].view(H, W, 3)
    fie.tile_blend(_dev(fie, t), xs, ys, H, W, out=out)
    assert np.array_equal(out.cpu().numpy(), tiles.blend_numpy(t, xs, ys, H, W))
    assert (buf[:off] == 0xA5).all() and (buf[off + H * W * 3:] == 0xA5).all()


@pytest.mark.parametrize("case", [(29, 37, 12, 16, _even(29, 12, 3), _even(37, 16, 3)), (24, 61, 24, 24, [0], _even(61, 24, 4)),
                                  (9, 700, 7, 400, [0, 2], [0, 300])], ids=_id)
def test_op_stays_inside_its_operands(fie, case):
    """Tiles and output inside guard bands (tests/isolation.py): the tiles' moat is 0xff in one run and 0 in the other, so a read one byte
    outside them changes a result, and a store outside the output is found in its arena."""
    H, W, th, tw, ys, xs = case
    t = _random(9, len(xs) * len(ys), th, tw)
    got = isolated(lambda i, o: fie.tile_blend(i["t"], xs, ys, H, W, out=o), {"t": flat(_dev(fie, t))},
                   dict(shape=(H, W, 3), dtype=torch.uint8, flat=True))
    assert np.array_equal(got.cpu().numpy(), tiles.blend_numpy(t, xs, ys, H, W))


def test_op_refuses_bad_arguments(fie):
    from fie_amd import hip
    th, tw, H, W = 8, 16, 8, 32
    t = _dev(fie, _random(1, 2, th, tw))
    # every malformed position list: not from 0, a gap, not ending at W - tw, not increasing, decreasing, empty, not integers, not a list, too many
    for xs in ([1, 16], [0, 17], [0, 15], [0, 0], [16, 0], [], [0, 16.0], [0, True], None, 7):
        with pytest.raises(ValueError, match="xs"):
            fie.tile_blend(t, xs, [0], H, W)
    with pytest.raises(ValueError, match="xs"):
        fie.tile_blend(_dev(fie, _random(2, 33, 2, 2)), list(range(33)), [0], 2, 34)
    with pytest.raises(ValueError, match="ys"):
        fie.tile_blend(t, [0, 16], [1], H + 1, W)
    with pytest.raises(ValueError, match="ys"):
        fie.tile_blend(t, [0], [0, 9], 17, tw)                                              # a gap between the rows of tiles
    with pytest.raises(ValueError, match="grid"):
        fie.tile_blend(t, [0], [0], th, tw)                                                 # two tiles for a grid of one
    for bad in (t.float(), t[:, :, :15], t[..., 0], t.cpu().numpy()):
        with pytest.raises(ValueError, match="tiles"):
            fie.tile_blend(bad, [0, 16], [0], H, W)
    for hw in ((0, W), (H, -1), (H, 32.0), (True, W)):
        with pytest.raises(ValueError):
            fie.tile_blend(t, [0, 16], [0], *hw)
    u8 = lambda *shape: torch.empty(shape, dtype=torch.uint8, device=fie.device)
    for bad_out in (u8(H, W, 4)[..., :3], u8(H, W + 1, 3), u8(H, W, 3).float(), t.view(-1)[:H * W * 3].view(H, W, 3)):
        with pytest.raises(ValueError, match="out must be"):
            fie.tile_blend(t, [0, 16], [0], H, W, out=bad_out)

    # the entry itself
    def raw(tl, nx, ny, xs, ys, th_, tw_, H_, W_, out):
        import ctypes
        arr = lambda p: None if p is None else (ctypes.c_int * max(len(p), 1))(*p)
        ptr = lambda x: None if x is None else x.data_ptr()
        hip._chk(hip.lib().fie_tile_blend_rgb_u8(fie.h, ptr(tl), nx, ny, arr(xs), arr(ys), th_, tw_, H_, W_, ptr(out)))

    o = u8(H, W, 3)
    for args in ((None, 2, 1, [0, 16], [0], th, tw, H, W, o), (t, 2, 1, None, [0], th, tw, H, W, o), (t, 2, 1, [0, 16], None, th, tw, H, W, o),
                 (t, 2, 1, [0, 16], [0], th, tw, H, W, None),                                                           # NULL
                 (t, 0, 1, [0], [0], th, tw, H, W, o), (t, 2, 33, [0, 16], [0] * 33, th, tw, H, W, o),                  # nx, ny outside 1 .. 32
                 (t, 2, 1, [0, 16], [0], 0, tw, H, W, o), (t, 2, 1, [0, 16], [0], th, tw, H, 0, o),                     # a size below 1
                 (t, 2, 1, [1, 16], [0], th, tw, H, W, o), (t, 2, 1, [0, 17], [0], th, tw, H, W + 1, o),
                 (t, 2, 1, [0, 15], [0], th, tw, H, W, o), (t, 2, 1, [0, 0], [0], th, tw, H, tw, o), (t, 2, 1, [0, 16], [1], th, tw, H + 1, W, o),
                 (t, 1, 1, [0], [0], 1, 1 << 16, 1 << 15, 1 << 16, o),                                                  # H * W >= 2^31
                 (t, 2, 1, [0, 16], [0], th, tw, H, W, t.view(-1)[8:])):                                                # the output inside the tiles
        with pytest.raises(hip.FieError):
            raw(*args)
    raw(t, 2, 1, [0, 16], [0], th, tw, H, W, o)                                             # and the good call goes through
    torch.cuda.synchronize()
    assert np.array_equal(o.cpu().numpy(), tiles.blend_numpy(t.cpu().numpy(), [0, 16], [0], H, W))


# ------------------------------------------------------------------------------------------------------------------------ the product surface
PROMPT = "a [red] kite"
SIZE = (700, 560)                      # "auto" at overlap 64, and (512, 512): four 512 x 512 tiles at x 0, 188 and y 0, 48
KW = dict(seed=9, strength=0.6)
AUTO = dict(tiles="auto", tile_overlap=64, tile_batch=3)


@pytest.fixture(scope="module")
def editor(fie):
    from src.pipeline import FastEditor
    return FastEditor(model_name="tiny", enable_cpu_offload=False)


@pytest.fixture(scope="module")
def img():
    return Image.fromarray(mo.textured(71, SIZE[1], SIZE[0]))


def _box_mask(W, H, x0, x1, y0, y1):
    m = np.zeros((H, W), np.uint8)
    m[y0:y1, x0:x1] = 255
    return m


def _reference(editor, image, prompt, plan, tile_batch, mask=None, **kw):
    """The right-hand side of the defining identity: edit_batch on the PIL crops, job by job, and the blend on the host."""
    tw, th, xs, ys = plan
    boxes = tiles.boxes(tw, th, xs, ys)
    rgb = image.convert("RGB")
    R = []
    for c in tiles.chunks(len(boxes), tile_batch):
        masks = None if mask is None else [mask[boxes[j][1]:boxes[j][3], boxes[j][0]:boxes[j][2]] for j in c]
        R += editor.edit_batch([rgb.crop(boxes[j]) for j in c], [prompt] * len(c), resolution=(tw, th), masks=masks, **kw)
    return tiles.blend_numpy(np.stack([np.asarray(r) for r in R]), xs, ys, image.height, image.width)


@pytest.fixture(scope="module")
def auto_plain(editor, img):
    """edit(img, tiles="auto", ...) and its reference, computed once for the tests that compare against them."""
    plan = tiles.plan(SIZE, "auto", 64)
    assert plan == (512, 512, [0, 188], [0, 48])
    return np.asarray(editor.edit(img, PROMPT, **AUTO, **KW)), _reference(editor, img, PROMPT, plan, 3, **KW)


def test_tiled_edit_is_the_blend_of_the_tile_edits(editor, img, auto_plain, monkeypatch):
    got, want = auto_plain
    assert got.shape == (SIZE[1], SIZE[0], 3) and np.array_equal(got, want)
    assert not np.array_equal(got, np.asarray(img))                                         # and it is an edit
    # explicit tiles, two per job
    out = editor.edit(img, PROMPT, tiles=(512, 512), tile_overlap=64, tile_batch=2, **KW)
    assert out.size == SIZE and out.mode == "RGB" and np.array_equal(np.asarray(out), want)
    # tile_batch=3 over four tiles: two jobs of two (tiles.chunks), not three and one
    assert tiles.chunks(4, 3) == [[0, 1], [2, 3]]
    jobs = []
    call = type(editor.pipe).__call__
    monkeypatch.setattr(type(editor.pipe), "__call__", lambda self, *a, **k: (jobs.append(len(k["prompt"])), call(self, *a, **k))[1])
    assert np.array_equal(np.asarray(editor.edit(img, PROMPT, **AUTO, **KW)), want)
    assert jobs == [2, 2]


def _near(sel, k):
    """sel grown by the (2k + 1)^2 square: the feather is separable, so its support around a set pixel is that square for k = ceil(3 sigma)."""
    h, w = sel.shape
    p = np.pad(sel, k)
    out = np.zeros_like(sel)
    for dy in range(2 * k + 1):
        for dx in range(2 * k + 1):
            out |= p[dy:dy + h, dx:dx + w]
    return out


def test_tiled_edit_with_a_mask(editor, img):
    """A box across all four tiles and both seams, grown by 4 and feathered: the mask grows whole and is cropped second, every tile pastes
    back through its crop, and where the grown, feathered mask is 0 the bytes are the source's."""
    mask = _box_mask(*SIZE, 150, 400, 30, 300)
    kw = dict(KW, mask_blur=1.5)
    got = np.asarray(editor.edit(img, PROMPT, mask=mask, mask_grow=4, **AUTO, **kw))
    grown = mgo.grow(mask, 4)
    want = _reference(editor, img, PROMPT, tiles.plan(SIZE, "auto", 64), 3, mask=grown, **kw)
    assert np.array_equal(got, want)
    far = ~_near(grown >= 128, 6)                           # 6 > ceil(3 sigma) = 5 pixels from the grown mask, per axis
    src = np.asarray(img)
    assert 0.3 < far.mean() < 0.9 and np.array_equal(got[far], src[far])
    assert not np.array_equal(got[mask >= 128], src[mask >= 128])


def test_metrics_score_source_and_output(editor, img, auto_plain):
    out, m = editor.edit(img, PROMPT, metrics=True, **AUTO, **KW)
    assert out.size == SIZE and np.array_equal(np.asarray(out), auto_plain[0])
    assert set(m) == {"ssim", "psnr", "mse"}
    ra, rb = np.asarray(img.resize((512, 512), Image.LANCZOS)), np.asarray(out.resize((512, 512), Image.LANCZOS))
    assert m["mse"] == mo.sse(ra, rb) / (65025.0 * ra.size)


def test_edit_batch_tiles_each_image_on_its_own(editor, img, auto_plain):
    other = Image.fromarray(mo.textured(72, 512, 640))          # 640 x 512: one tile, the image itself
    prompts = [PROMPT, "a [blue] ball"]
    outs = editor.edit_batch([img, other], prompts, **AUTO, **KW)
    assert [o.size for o in outs] == [SIZE, (640, 512)]
    assert np.array_equal(np.asarray(outs[0]), auto_plain[0])
    assert np.array_equal(np.asarray(outs[1]), np.asarray(editor.edit(other, prompts[1], **AUTO, **KW)))
    assert tiles.plan((640, 512), "auto", 64) == (640, 512, [0], [0])
    assert np.array_equal(np.asarray(outs[1]), np.asarray(editor.edit_batch([other], [prompts[1]], resolution=(640, 512), **KW)[0]))


def test_forbidden_combinations(editor, img):
    for clash in (dict(resolution=(512, 512)), dict(region=(0, 0, 64, 64)), dict(outpaint=(0, 0, 8, 0)), dict(output_size="edit")):
        with pytest.raises(ValueError, match="tiles with"):
            editor.edit(img, PROMPT, **AUTO, **clash)
        with pytest.raises(ValueError, match="tiles with"):
            editor.edit_batch([img], [PROMPT], **AUTO, **clash)
    with pytest.raises(ValueError, match="below the tile"):
        editor.edit(img, PROMPT, tiles=(1024, 512))
    with pytest.raises(ValueError, match="tile_batch"):
        editor.edit(img, PROMPT, tiles="auto", tile_batch=0)
    assert editor.edit(img, PROMPT, output_size="source", **AUTO, **KW).size == SIZE       # the source's size in so many words


def test_none_changes_nothing(editor, monkeypatch):
    small = Image.fromarray(mo.textured(73, 96, 80))
    kw = dict(KW, resolution=(512, 512))
    want = np.asarray(editor.edit(small, PROMPT, **kw))
    want_b = [np.asarray(x) for x in editor.edit_batch([small, small], [PROMPT, PROMPT], **kw)]

    def boom(*a, **k):
        raise AssertionError("tiles=None must not reach the op")
    monkeypatch.setattr(type(editor.pipe.ctx), "tile_blend", boom)
    assert np.array_equal(np.asarray(editor.edit(small, PROMPT, tiles=None, **kw)), want)
    got = editor.edit_batch([small, small], [PROMPT, PROMPT], tiles=None, tile_overlap=0, tile_batch=16, **kw)
    assert all(np.array_equal(np.asarray(g), w) for g, w in zip(got, want_b))


def test_run_single_image_tiles_auto(editor, img, tmp_path, monkeypatch):
    """run_single_image.py --tiles auto writes an image of the source's size (the command line's own models are the full-size ones: the run is
    handed this module's tiny editor)."""
    import run_single_image
    import src.pipeline
    monkeypatch.setattr(src.pipeline, "FastEditor", lambda **kw: editor)
    path = tmp_path / "in.png"
    img.save(path)
    run_single_image.main(["--image", str(path), "--prompt", PROMPT, "--seed", "9", "--tiles", "auto", "--tile_overlap", "64", "--output_dir",
                           str(tmp_path / "out")])
    written = sorted((tmp_path / "out").rglob("edited_*.jpg"))
    assert len(written) == 1 and Image.open(written[0]).size == SIZE
