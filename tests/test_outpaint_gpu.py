"""`outpaint` on the device: fie_outpaint_canvas_rgb_u8 byte for byte against the numpy restatement
(tests/outpaint_oracle.py), inside guard bands and against every bad argument, and the one identity every layer above it is held to -- a call
with `outpaint=o` returns exactly what the call on the canvas with the canvas mask returns -- on FastEditor (tiny stack; every comparison a bit
equality)."""
import numpy as np
import pytest
import torch
from PIL import Image

import mask_grow_oracle as mgo
import outpaint_oracle as opo
from isolation import flat, isolated

pytestmark = pytest.mark.gpu


def _dev(fie, a):
    return torch.from_numpy(np.array(a, order="C")).to(fie.device)                 # a writable copy (PIL arrays are read-only)


def _src(h, w):
    return np.random.default_rng(1000 * h + w).integers(0, 256, (h, w, 3), dtype=np.uint8)


# ------------------------------------------------------------------------------------------------------------------------ the op
# Rows of 3 Wc and Wc bytes start wherever the rows before them end: the cases give both row lengths every residue mod 4 (so a row's head
# and tail take every length 0 .. 3), the interior every start residue, rows shorter than one dword, one block and several per row.
# (16, 61) with left and right 0: all four margins 0 is no outpainting, so that one case gets a bottom row.
CASES = ([((1, 1), (1, 0, 0, 0)), ((1, 1), (0, 0, 0, 1)), ((5, 7), (3, 2, 1, 4)),
          ((33, 130), (1, 0, 2, 0)), ((33, 130), (0, 5, 0, 0)), ((33, 130), (4, 4, 4, 4)), ((72, 88), (7, 1, 6, 3))]
         + [((16, 61), (l, 0, r, 0 if l or r else 1)) for l in range(4) for r in range(4)]
         + [((2, 3), (0, 0, 4096, 0)), ((2, 3), (0, 4096, 0, 0))])


def _pattern(shape, device):
    n = int(np.prod(shape))
    return (torch.arange(n, device=device) % 251).to(torch.uint8).view(shape)


@pytest.mark.parametrize("shape,margins", CASES, ids=[f"{s[0]}x{s[1]}+{'.'.join(map(str, m))}" for s, m in CASES])
def test_op_matches_the_restatement(fie, shape, margins):
    h, w = shape
    l, t, r, b = margins
    hc, wc = t + h + b, l + w + r
    src, mask = _src(h, w), opo.grey_mask(h, w)
    s_dev, m_dev = _dev(fie, src), _dev(fie, mask)
    for m_np, m_t in ((mask, m_dev), (None, None)):
        out = _pattern((hc, wc, 3), fie.device), _pattern((hc, wc), fie.device)
        got = fie.outpaint_canvas(s_dev, m_t, margins, out=out)
        assert got[0] is out[0] and got[1] is out[1]
        bad = np.argwhere(got[0].cpu().numpy() != opo.canvas(src, margins))
        assert bad.size == 0, (m_np is None, len(bad), bad[:4].tolist())
        bad = np.argwhere(got[1].cpu().numpy() != opo.canvas_mask(m_np, shape, margins))
        assert bad.size == 0, (m_np is None, len(bad), bad[:4].tolist())
    c, cm = fie.outpaint_canvas(s_dev, m_dev, list(margins))                       # outputs of its own
    assert np.array_equal(c.cpu().numpy(), opo.canvas(src, margins)) and np.array_equal(cm.cpu().numpy(), opo.canvas_mask(mask, shape, margins))
    assert np.array_equal(s_dev.cpu().numpy(), src) and np.array_equal(m_dev.cpu().numpy(), mask)      # the operands are unchanged


@pytest.mark.parametrize("co,mo", [(1, 3), (2, 2), (3, 1)])
def test_op_at_every_alignment_of_its_outputs(fie, co, mo):
    """The split of a row into head, dwords and tail follows its ADDRESS: outputs that start 1, 2 and 3 bytes past a dword boundary, the bytes
    around them checked."""
    (h, w), margins = (16, 61), (3, 2, 1, 0)
    hc, wc = 18, 65
    src, mask = _src(h, w), opo.grey_mask(h, w)
    cbuf, mbuf = torch.full((hc * wc * 3 + 8,), 0xA5, dtype=torch.uint8, device=fie.device), torch.full((hc * wc + 8,), 0xA5, dtype=torch.uint8, device=fie.device)
    assert cbuf.data_ptr() % 4 == 0 and mbuf.data_ptr() % 4 == 0
    out = cbuf[co:co + hc * wc * 3].view(hc, wc, 3), mbuf[mo:mo + hc * wc].view(hc, wc)
    fie.outpaint_canvas(_dev(fie, src), _dev(fie, mask), margins, out=out)
    assert np.array_equal(out[0].cpu().numpy(), opo.canvas(src, margins)) and np.array_equal(out[1].cpu().numpy(), opo.canvas_mask(mask, (h, w), margins))
    for buf, o, n in ((cbuf, co, hc * wc * 3), (mbuf, mo, hc * wc)):
        assert (buf[:o] == 0xA5).all() and (buf[o + n:] == 0xA5).all()


@pytest.mark.parametrize("shape,margins", [((33, 130), (1, 0, 2, 3)), ((16, 61), (3, 2, 1, 0))])
def test_op_stays_inside_its_operands(fie, shape, margins):
    """All four tensors inside guard bands (tests/isolation.py): the moats of source and mask are 0xff in one run and 0 in the other, so a read
    one byte outside either changes a result, and a store outside either output is found in its arena."""
    h, w = shape
    l, t, r, b = margins
    hc, wc = t + h + b, l + w + r
    src, mask = _src(h, w), opo.grey_mask(h, w)
    specs = [dict(shape=(hc, wc, 3), dtype=torch.uint8, flat=True), dict(shape=(hc, wc), dtype=torch.uint8, flat=True)]
    got = isolated(lambda i, o: fie.outpaint_canvas(i["s"], i["m"], margins, out=(o[0], o[1])),
                   {"s": flat(_dev(fie, src)), "m": flat(_dev(fie, mask))}, specs)
    assert np.array_equal(got[0].cpu().numpy(), opo.canvas(src, margins)) and np.array_equal(got[1].cpu().numpy(), opo.canvas_mask(mask, shape, margins))
    got = isolated(lambda i, o: fie.outpaint_canvas(i["s"], None, margins, out=(o[0], o[1])), {"s": flat(_dev(fie, src))}, specs)
    assert np.array_equal(got[0].cpu().numpy(), opo.canvas(src, margins)) and np.array_equal(got[1].cpu().numpy(), opo.canvas_mask(None, shape, margins))


def test_op_refuses_bad_arguments(fie):
    from fie_amd import hip
    h, w, o = 24, 40, (2, 0, 1, 3)
    s, m = _dev(fie, _src(h, w)), _dev(fie, opo.grey_mask(h, w))
    u8 = lambda *shape: torch.empty(shape, dtype=torch.uint8, device=fie.device)
    # the wrapper
    for bad in ((True, 0, 0, 0), (1.0, 0, 0, 0), (1, 2, 3), (1, 2, 3, 4, 5), 7, (-1, 0, 0, 0), (0, 4097, 0, 0), (0, 0, 0, 0)):
        with pytest.raises(ValueError, match="margins"):
            fie.outpaint_canvas(s, m, bad)
    for bad_src in (s.float(), s[:, :39], s[:, :, 0], s.cpu().numpy()):         # dtype, not contiguous, not [H, W, 3], not a tensor
        with pytest.raises(ValueError, match="source"):
            fie.outpaint_canvas(bad_src, None, o)
    for bad_mask in (m.float(), m[:, :39], u8(h, w + 1), u8(h, w, 1)):
        with pytest.raises(ValueError, match="mask_l"):
            fie.outpaint_canvas(s, bad_mask, o)
    for bad_out in ((u8(27, 43, 3),), (u8(27, 43, 3), u8(27, 44)), (u8(27, 44, 3), u8(27, 43)), (u8(27, 43, 3).float(), u8(27, 43)),
                    (u8(27, 43, 4)[..., :3], u8(27, 43)), u8(27, 43, 3)):
        with pytest.raises(ValueError, match="out must be"):
            fie.outpaint_canvas(s, m, o, out=bad_out)
    big = u8(27 * 43 * 3)
    s_in = big[:h * w * 3].view(h, w, 3)
    with pytest.raises(ValueError, match="of their own"):                          # the canvas starts where the source starts
        fie.outpaint_canvas(s_in, m, o, out=(big.view(27, 43, 3), u8(27, 43)))
    with pytest.raises(ValueError, match="of their own"):                          # one buffer for both outputs
        fie.outpaint_canvas(s, m, o, out=(big.view(27, 43, 3), big[:27 * 43].view(27, 43)))
    wide = u8(1, 1 << 18, 3)
    with pytest.raises(ValueError, match="2\\^31"):                                # 8193 x 262144 = 2^31 + 2^18 pixels
        fie.outpaint_canvas(wide, None, (0, 4096, 0, 4096))

    # the entry itself
    def raw(src, mask, hh, ww, margins, canvas, cmask):
        ptr = lambda t: None if t is None else t.data_ptr()
        hip._chk(hip.lib().fie_outpaint_canvas_rgb_u8(fie.h, ptr(src), ptr(mask), hh, ww, *margins, ptr(canvas), ptr(cmask)))

    c, cm = u8(27, 43, 3), u8(27, 43)
    for args in ((None, m, h, w, o, c, cm), (s, m, h, w, o, None, cm), (s, m, h, w, o, c, None),                # NULL
                 (s, m, 0, w, o, c, cm), (s, m, h, 0, o, c, cm), (s, m, -1, w, o, c, cm),                          # H or W < 1
                 (s, m, h, w, (-1, 0, 0, 0), c, cm), (s, m, h, w, (0, 0, 4097, 0), c, cm), (s, m, h, w, (0, 0, 0, -2), c, cm),
                 (s, m, h, w, (0, 0, 0, 0), c, cm),                                                                # no margin at all
                 (wide, None, 1, 1 << 18, (0, 4096, 0, 4096), c, cm)):                                              # Hc * Wc >= 2^31
        with pytest.raises(hip.FieError):
            raw(*args)
    # overlaps: the canvas reaches into the source's last bytes; the canvas mask lies inside the canvas; the canvas mask reaches into the mask
    arena = u8(h * w * 3 + 27 * 43 * 3 - 8)
    with pytest.raises(hip.FieError, match="overlaps"):
        raw(arena[:h * w * 3].view(h, w, 3), m, h, w, o, arena[h * w * 3 - 8:].view(27, 43, 3), cm)
    with pytest.raises(hip.FieError, match="overlaps"):
        raw(s, m, h, w, o, c, c.view(-1)[100:100 + 27 * 43].view(27, 43))
    arena = u8(h * w + 27 * 43 - 1)
    with pytest.raises(hip.FieError, match="overlaps"):
        raw(s, arena[:h * w].view(h, w), h, w, o, c, arena[h * w - 1:].view(27, 43))
    raw(s, None, h, w, o, c, cm)                                                  # and the good call goes through
    torch.cuda.synchronize()
    assert np.array_equal(c.cpu().numpy(), opo.canvas(s.cpu().numpy(), o))


# ------------------------------------------------------------------------------------------------------------------------ the product surface
RES = (512, 512)
PROMPT = "a [wide] beach"


def synth_image(seed, w, h):
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float32) / max(h, w)
    img = np.stack([0.5 + 0.4 * np.sin(6.0 * xx + rng.uniform(0, 6)) * np.cos(4.0 * yy + rng.uniform(0, 6)) for _ in range(3)], axis=2)
    for _ in range(4):
        cx, cy, r = rng.uniform(0.1, 0.9), rng.uniform(0.1, 0.7), rng.uniform(0.1, 0.25)
        img[((xx - cx) ** 2 + (yy - cy) ** 2) < r * r] = rng.uniform(0, 1, 3)
    return Image.fromarray((img.clip(0, 1) * 255).astype(np.uint8))


def _reference(img, margins, mask=None):
    """The right-hand side of the identity: (canvas as a PIL image, canvas mask as an array), from the oracle."""
    return Image.fromarray(opo.canvas(np.asarray(img), margins)), opo.canvas_mask(mask, (img.height, img.width), margins)


def _near(sel, k):
    """sel grown by the (2k + 1)^2 square: the feather is separable, so its support around a set pixel is that square for k = ceil(3 sigma)."""
    h, w = sel.shape
    p = np.pad(sel, k)
    out = np.zeros_like(sel)
    for dy in range(2 * k + 1):
        for dx in range(2 * k + 1):
            out |= p[dy:dy + h, dx:dx + w]
    return out


@pytest.fixture(scope="module")
def editor(fie):
    from src.pipeline import FastEditor
    return FastEditor(model_name="tiny", enable_cpu_offload=False)


@pytest.mark.parametrize("user_mask", [False, True], ids=["plain", "user_mask"])
def test_edit_is_the_edit_of_the_canvas(editor, user_mask):
    img = synth_image(51, 200, 150)
    o = (0, 0, 56, 0)
    mask = None
    if user_mask:                                                        # the union is carried: a block of 255, greys on both sides of 128
        mask = np.zeros((150, 200), np.uint8)
        mask[30:70, 40:90] = 255
        mask[70:90, 40:60] = 130
        mask[100:120, 100:140] = 100
    kw = dict(seed=9, strength=0.6, resolution=RES, masked_content="fill", mask_grow=6, mask_blur=2, output_size="source")
    canvas, cmask = _reference(img, o, mask)
    got = editor.edit(img, PROMPT, mask=mask, outpaint=o, **kw)
    want = editor.edit(canvas, PROMPT, mask=cmask, **kw)
    assert got.size == canvas.size == (256, 150)
    g = np.asarray(got)
    assert np.array_equal(g, np.asarray(want))
    # 7 px (more than the 6 = ceil(3 sigma) the feather reaches) from the grown mask, per axis: the caller's bytes, at the shifted position
    far = ~_near(mgo.grow(cmask, 6) > 0, 7)
    shifted = np.zeros_like(g)
    shifted[o[1]:o[1] + 150, o[0]:o[0] + 200] = np.asarray(img)
    assert far.sum() > 150 * 100 and not far[:, 200 - 6:].any()
    assert np.array_equal(g[far], shifted[far])
    assert not np.array_equal(g[:, 200:], np.asarray(canvas)[:, 200:])   # the border is new
    if user_mask:
        assert not np.array_equal(g[30:70, 40:90], np.asarray(img)[30:70, 40:90])
        assert not np.array_equal(g, np.asarray(editor.edit(img, PROMPT, outpaint=o, **kw)))


def test_region_mask_and_metrics_see_the_canvas(editor):
    from fie_amd import region as hregion
    img = synth_image(41, 96, 80)
    o = (0, 0, 24, 0)
    canvas, cmask = _reference(img, o)
    kw = dict(seed=8, strength=0.6, resolution=RES, mask_blur=1.0, masked_content="fill", region="mask", region_padding=8, metrics=True)
    got, scores = editor.edit(img, PROMPT, outpaint=o, **kw)
    want, want_scores = editor.edit(canvas, PROMPT, mask=cmask, **kw)
    assert got.size == (120, 80) and np.array_equal(np.asarray(got), np.asarray(want)) and scores == want_scores
    assert {"ssim", "psnr", "mse", "bg_ssim", "bg_psnr", "bg_mse"} <= set(scores)
    l, t, r, b = hregion.resolve("mask", canvas.size, cmask, 8, RES)
    outside = np.ones((80, 120), bool)
    outside[t:b, l:r] = False
    assert outside.any() and np.array_equal(np.asarray(got)[outside], np.asarray(canvas)[outside])
    assert not np.array_equal(np.asarray(got)[:, 96:], np.asarray(canvas)[:, 96:])
    # an explicit box is in canvas coordinates: one across the seam that ends at the canvas's right edge, past the source's
    kw = dict(seed=8, strength=0.6, resolution=RES, region=(88, 10, 120, 42))
    got = editor.edit(img, PROMPT, outpaint=o, **kw)
    assert np.array_equal(np.asarray(got), np.asarray(editor.edit(canvas, PROMPT, mask=cmask, **kw)))


@pytest.mark.parametrize("mode", ["latent_noise", "original"])
def test_content_modes(editor, mode):
    img = synth_image(43, 96, 80)
    o = (16, 8, 0, 0)
    canvas, cmask = _reference(img, o)
    kw = dict(seed=5, strength=0.6, resolution="auto", masked_content=mode)
    got = editor.edit(img, PROMPT, outpaint=o, **kw)
    want = editor.edit(canvas, PROMPT, mask=cmask, **kw)
    assert got.size == want.size and np.array_equal(np.asarray(got), np.asarray(want))       # "auto": the bucket of the canvas's 112 : 88


def test_edit_batch(editor):
    imgs = [synth_image(42, 96, 96), synth_image(44, 96, 96)]
    prompts = ["a [toy] number 0", "a [toy] number 1"]
    o = (8, 0, 8, 0)
    kw = dict(seed=11, strength=0.5, resolution=RES)
    refs = [_reference(im, o) for im in imgs]
    arr = lambda outs: [np.asarray(x) for x in outs]
    got = arr(editor.edit_batch(imgs, prompts, outpaint=[o, None], **kw))
    want = arr(editor.edit_batch([refs[0][0], imgs[1]], prompts, masks=[refs[0][1], None], **kw))
    plain = arr(editor.edit_batch(imgs, prompts, **kw))
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    assert np.array_equal(got[1], plain[1]) and not np.array_equal(got[0], plain[0])         # an entry of None: as without the keyword
    got = arr(editor.edit_batch(imgs, prompts, outpaint=o, **kw))                             # one tuple for both
    want = arr(editor.edit_batch([c for c, _ in refs], prompts, masks=[m for _, m in refs], **kw))
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    # canvases of two target sizes under "auto", a user mask on one, source-size outputs: one device job per size, results in input order
    mask = np.zeros((96, 96), np.uint8)
    mask[20:40, 30:70] = 255
    os_ = [(0, 0, 96, 0), (0, 0, 0, 4)]
    kw = dict(seed=11, strength=0.5, resolution="auto", output_size="source", mask_grow=3)
    refs = [_reference(imgs[0], os_[0]), _reference(imgs[1], os_[1], mask)]
    got = editor.edit_batch(imgs, prompts, masks=[None, mask], outpaint=os_, **kw)
    want = editor.edit_batch([c for c, _ in refs], prompts, masks=[m for _, m in refs], **kw)
    assert [g.size for g in got] == [(192, 96), (96, 100)]
    assert all(np.array_equal(np.asarray(g), np.asarray(x)) for g, x in zip(got, want))
    # regions per image
    kw = dict(seed=11, strength=0.5, resolution=RES, region=["mask", None], region_padding=8)
    got = editor.edit_batch(imgs, prompts, outpaint=[o, None], **kw)
    want = editor.edit_batch([_reference(imgs[0], o)[0], imgs[1]], prompts, masks=[_reference(imgs[0], o)[1], None], **kw)
    assert all(np.array_equal(np.asarray(g), np.asarray(x)) for g, x in zip(got, want))


def test_outpaint_canvas_returns_the_oracles_pair(editor):
    img = synth_image(45, 61, 16)
    mask = opo.grey_mask(16, 61)
    for o in ((3, 2, 1, 0), (0, 0, 0, 7)):
        for m in (None, mask, Image.fromarray(mask)):
            c, cm = editor.outpaint_canvas(img, o, mask=m)
            assert c.mode == "RGB" and cm.mode == "L" and c.size == cm.size == (61 + o[0] + o[2], 16 + o[1] + o[3])
            assert np.array_equal(np.asarray(c), opo.canvas(np.asarray(img), o))
            assert np.array_equal(np.asarray(cm), opo.canvas_mask(None if m is None else mask, (16, 61), o))
    grey = img.convert("L")                                              # another mode goes through convert("RGB")
    assert np.array_equal(np.asarray(editor.outpaint_canvas(grey, (1, 0, 0, 0))[0]), opo.canvas(np.asarray(grey.convert("RGB")), (1, 0, 0, 0)))


def test_none_launches_nothing(editor, monkeypatch):
    img = synth_image(46, 96, 80)
    mask = np.zeros((80, 96), np.uint8)
    mask[20:50, 30:70] = 255
    kw = dict(seed=3, strength=0.6, resolution=RES)
    want = np.asarray(editor.edit(img, PROMPT, **kw))
    want_m = np.asarray(editor.edit(img, PROMPT, mask=mask, mask_grow=2, **kw))
    want_b = [np.asarray(x) for x in editor.edit_batch([img, img], [PROMPT, PROMPT], **kw)]

    def boom(*a, **k):
        raise AssertionError("outpaint=None must not reach the op")
    monkeypatch.setattr(type(editor.pipe.ctx), "outpaint_canvas", boom)
    assert np.array_equal(np.asarray(editor.edit(img, PROMPT, outpaint=None, **kw)), want)
    assert np.array_equal(np.asarray(editor.edit(img, PROMPT, mask=mask, mask_grow=2, outpaint=None, **kw)), want_m)
    for none in (None, [None, None]):
        got = editor.edit_batch([img, img], [PROMPT, PROMPT], outpaint=none, **kw)
        assert all(np.array_equal(np.asarray(g), w) for g, w in zip(got, want_b))
    with pytest.raises(AssertionError, match="must not reach"):
        editor.edit(img, PROMPT, outpaint=(0, 0, 8, 0), **kw)
