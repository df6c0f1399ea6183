"""Edge-budget Canny on the device.  Everything is integer arithmetic, so every comparison of the op is a byte equality:
the pair from the device, the host C++ entry and the numpy restatement (tests/canny_auto_oracle.py), and the edge map against the oracle's Canny
under that pair; the two-call form; one workspace under two images; guard bands; then `set_canny_density` on FastEditor (tiny stack, 512 x 512)."""
import contextlib

import numpy as np
import pytest
import torch
from PIL import Image

import canny_auto_oracle as oracle
import isolation as iso

import fie_amd  # noqa: F401
from fie_amd import hip

pytestmark = pytest.mark.gpu


def _dev(fie, a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(fie.device)


def _budgets(n):
    return sorted({1, max(1, n // 50), max(1, n // 4)})


def _shape_image(h, w):
    return oracle.to_u8(oracle.disks_float(h * 1000 + w, h, w, disks=10))


def _three_way(fie, img, seeds, lo=100, hi=200):
    """The pair from the device == the host entry == the restatement, and the device's map == the oracle's Canny under that pair == the host's."""
    want_map, want = oracle.canny_auto(img, seeds, lo, hi)
    src = _dev(fie, img)
    assert fie.canny_thresholds(src, seeds, lo, hi) == want, (img.shape, seeds)
    assert hip.canny_auto_thresholds(img, seeds, lo, hi) == want, (img.shape, seeds)
    got = fie.canny_device(src, lo, hi, budget=seeds).cpu().numpy()
    assert fie.canny_pair == want, (img.shape, seeds)
    bad = np.argwhere(got != want_map)
    assert bad.size == 0, (img.shape, seeds, want, len(bad), bad[:4].tolist())
    assert np.array_equal(got, hip.canny_rgb(img, *want))
    assert np.array_equal(src.cpu().numpy(), img)                                          # the operand is unchanged
    return want


# ------------------------------------------------------------------------------------------------------------------------ 7. three ways, byte exact
@pytest.mark.parametrize("h,w", [(8, 8), (5, 3), (33, 70), (97, 131), (64, 64), (256, 256)])
def test_three_way_byte_exact(fie, h, w):
    img = _shape_image(h, w)
    pairs = [_three_way(fie, img, seeds) for seeds in _budgets(h * w)]
    assert pairs == sorted(pairs, reverse=True)                                            # a larger budget never raises the thresholds
    mid = _budgets(h * w)[1]
    assert _three_way(fie, img, mid, 150, 50) == _three_way(fie, img, mid, 50, 150)        # lo > hi is swapped
    assert _three_way(fie, img, mid, 0, 7)[0] == 0


def test_three_way_at_1024(fie):
    low, high = _three_way(fie, _shape_image(1024, 1024), oracle.budget(1024 * 1024, 0.01))
    assert high > 16 and low == high // 2


@pytest.mark.parametrize("h,w", [(64, 1024), (256, 256)])
def test_special_images(fie, h, w):
    n = h * w
    # stripes: every ridge pixel in one histogram bin, and the tie rule: all of them or none.  Two pixels wide the suppression keeps one column;
    # three wide it keeps a third of the image: the atomics' worst contention
    for width, least in ((2, h), (3, n // 4)):
        img = oracle.stripes(h, w, width)
        r = oracle.ridge(img)
        level, count = int(r.max()), int((r > 0).sum())
        assert set(np.unique(r)) == {0, level} and count >= least
        assert _three_way(fie, img, count - 1) == (level // 2, level)                       # ties fall on the "fewer seeds" side: an empty map
        assert fie.canny_device(_dev(fie, img), budget=count - 1).max().item() == 0
        assert _three_way(fie, img, count)[1] == 16                                        # the budget that holds them all
    # the long chain: ridge pixels at 120 but for the seed's -- `>` against `>=` at the threshold
    img = oracle.long_chain(h, w)
    r = oracle.ridge(img)
    above = int((r > 120).sum())
    assert 0 < above < (r == 120).sum()
    assert _three_way(fie, img, above) == (60, 120)                                        # the chain stays weak, the seed strong
    assert _three_way(fie, img, above - 1)[1] > 120 and _three_way(fie, img, n // 4)[1] < 120
    # the floor: a histogram that is all zero, and one that lies wholly below 16
    for img in (oracle.flat(h, w), oracle.plus_minus_one(h, w)):
        for seeds in (1, n // 4):
            assert _three_way(fie, img, seeds) == (8, 16)
            assert fie.canny_device(_dev(fie, img), budget=seeds).max().item() == 0


def test_bad_arguments_are_refused(fie):
    src = _dev(fie, _shape_image(8, 8))
    for seeds, lo, hi in ((0, 100, 200), (65, 100, 200), (1, 0, 0), (1, -1, 200)):
        with pytest.raises(hip.FieError):
            fie.canny_thresholds(src, seeds, lo, hi)
        with pytest.raises(hip.FieError):
            fie.canny_device(src, lo, hi, budget=seeds)
    ws = torch.empty(hip.lib().fie_canny_auto_workspace_bytes(8, 8) + 16, device=fie.device, dtype=torch.uint8)
    with pytest.raises(hip.FieError):                                                      # a workspace off the 16-byte grid
        fie.canny_thresholds(src, 1, workspace=ws[1:])


# ------------------------------------------------------------------------------------------------------------------------ 8. the two-call form
def test_two_call_form(fie):
    img = _shape_image(256, 256)
    seeds = oracle.budget(256 * 256, 0.01)
    src = _dev(fie, img)
    one = fie.canny_device(src, budget=seeds).cpu().numpy()
    pair = fie.canny_pair
    edges, state = fie.canny_begin(src, rounds=4, budget=seeds)
    assert fie.canny_finish(state) is edges and np.array_equal(edges.cpu().numpy(), one)
    assert fie.canny_more == 0 and fie.canny_passes == 16 and fie.canny_pair == pair == oracle.thresholds(img, seeds)
    assert state[4].tolist()[4:] == list(pair)                                             # the pinned words: four flags, then low and high
    chain = oracle.long_chain(64, 1024)
    seeds = int((oracle.ridge(chain) > 120).sum())
    src = _dev(fie, chain)
    one = fie.canny_device(src, budget=seeds).cpu().numpy()
    edges, state = fie.canny_begin(src, rounds=4, budget=seeds)                            # 16 passes cannot finish this one
    assert np.array_equal(fie.canny_finish(state).cpu().numpy(), one) and fie.canny_more > 0 and fie.canny_pair == (60, 120)
    assert np.array_equal(one, oracle.canny_auto(chain, seeds)[0]) and one[:, 900:].max() == 255
    assert state[4].tolist()[4:] == [60, 120]                                              # finish's own flag copies leave the pair alone


# ------------------------------------------------------------------------------------------------------------------------ 9. repeat and determinism
def test_one_workspace_two_images_and_determinism(fie):
    h, w = 97, 131
    a, b = _shape_image(h, w), oracle.clutter(5, h, w)
    seeds = _budgets(h * w)[1]
    ws = torch.empty(hip.lib().fie_canny_auto_workspace_bytes(h, w), device=fie.device, dtype=torch.uint8)
    want = [oracle.canny_auto(x, seeds) for x in (a, b)]
    assert want[0][1] != want[1][1]
    for _ in range(2):                                                                      # a, b, a, b through the one workspace: the histogram is clean each time
        for x, (want_map, want_pair) in zip((a, b), want):
            assert fie.canny_thresholds(_dev(fie, x), seeds, workspace=ws) == want_pair
            edges, state = fie.canny_begin(_dev(fie, x), rounds=4, budget=seeds, workspace=ws)
            assert np.array_equal(fie.canny_finish(state).cpu().numpy(), want_map) and fie.canny_pair == want_pair
    src = _dev(fie, oracle.stripes(256, 256))
    first = fie.canny_device(src, budget=300).cpu().numpy()
    assert all(np.array_equal(fie.canny_device(src, budget=300).cpu().numpy(), first) for _ in range(3))


# ------------------------------------------------------------------------------------------------------------------------ 10. guard bands
@pytest.mark.parametrize("h,w", [(33, 70), (97, 131)])
def test_entries_stay_inside_their_operands(fie, h, w):
    """The image in a moat (0xff in one run, 0 in the other: a read outside it changes a result), the edge map and the workspace guarded views."""
    img = _shape_image(h, w)
    seeds = _budgets(h * w)[1]
    need = hip.lib().fie_canny_auto_workspace_bytes(h, w)
    want_map, want_pair = oracle.canny_auto(img, seeds)
    guards, pairs = [], []

    def run(i, o):
        (ws_map, g_map), (ws_pair, g_pair) = (iso.guarded((need,), dtype=torch.uint8, device=fie.device, flat=True) for _ in range(2))
        guards.extend((g_map, g_pair))
        fie.canny_device(i["img"], budget=seeds, out=o, workspace=ws_map)                   # begin_auto + finish
        pairs.append(fie.canny_pair)
        pairs.append(fie.canny_thresholds(i["img"], seeds, workspace=ws_pair))              # ridge + select alone

    got = iso.isolated(run, {"img": iso.flat(_dev(fie, img))}, dict(shape=(h, w, 3), dtype=torch.uint8, flat=True))
    for g in guards:
        g.check("workspace")
    assert len(guards) == 4 and pairs == [want_pair] * 4 and np.array_equal(got.cpu().numpy(), want_map)


# ------------------------------------------------------------------------------------------------------------------------ 11. end to end
PROMPT = "a [red] kite"
KW = dict(seed=9, strength=0.6, resolution=(512, 512))
D = 0.01


@pytest.fixture(scope="module")
def editor(fie):
    from src.pipeline import FastEditor
    return FastEditor(model_name="tiny", enable_cpu_offload=False)


@contextlib.contextmanager
def density(editor, d):
    """The editor's setting for the calls inside, put back behind them (the editor is the module's)."""
    before = editor.set_canny_density(d)
    try:
        yield
    finally:
        editor.set_canny_density(before)


@pytest.fixture(scope="module")
def hazy():
    return Image.fromarray(oracle.to_u8(oracle.low_contrast(oracle.disks_float(2))))


@pytest.fixture(scope="module")
def hazy_pair(editor, hazy):
    pair = editor.canny_thresholds(hazy, D, resolution=(512, 512))
    src = np.asarray(hazy.resize((512, 512), Image.LANCZOS))
    assert pair == oracle.thresholds(src, oracle.budget(512 * 512, D)) and 16 < pair[1] < 200          # the statistics of the image the Canny sees
    return pair


@pytest.fixture(scope="module")
def hazy_auto(editor, hazy):
    with density(editor, D):
        return np.asarray(editor.edit(hazy, PROMPT, **KW))


def _close(a, b):
    """edit_batch's bound against serial edits (tests/test_pipeline_gpu.py): max |du8| <= 2 and SSIM > 0.999."""
    from oracle import metrics
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and np.abs(a.astype(int) - b.astype(int)).max() <= 2 and metrics.ssim(Image.fromarray(a), Image.fromarray(b), size=None) > 0.999


def test_edit_equals_the_explicit_thresholds(editor, hazy, hazy_pair, hazy_auto):
    low, high = hazy_pair
    explicit = np.asarray(editor.edit(hazy, PROMPT, canny_low_threshold=low, canny_high_threshold=high, **KW))
    assert np.array_equal(hazy_auto, explicit) and editor.last_canny_thresholds() == [None]
    assert not np.array_equal(hazy_auto, np.asarray(editor.edit(hazy, PROMPT, **KW)))       # Canny(100, 200) draws another map of a hazy image
    edges = np.asarray(editor.preprocess_image(hazy.resize((512, 512), Image.LANCZOS), canny_density=D))
    assert np.array_equal(edges, oracle.canny_auto(np.asarray(hazy.resize((512, 512), Image.LANCZOS)), oracle.budget(512 * 512, D))[0])
    assert (edges[..., 0] > 0).mean() >= 0.01 > (np.asarray(editor.preprocess_image(hazy.resize((512, 512), Image.LANCZOS)))[..., 0] > 0).mean()


def test_metrics_report_the_pair(editor, hazy, hazy_pair, hazy_auto):
    with density(editor, D):
        out, m = editor.edit(hazy, PROMPT, metrics=True, **KW)
    assert editor.canny_density is None
    assert np.array_equal(np.asarray(out), hazy_auto) and (m["canny_low"], m["canny_high"]) == hazy_pair
    assert set(m) == {"ssim", "psnr", "mse", "canny_low", "canny_high"} and editor.last_canny_thresholds() == [hazy_pair]


def test_edit_batch_gives_every_image_its_own_pair(editor, hazy, hazy_pair):
    full = Image.fromarray(oracle.to_u8(oracle.disks_float(2)))
    full_pair = editor.canny_thresholds(full, D, resolution=(512, 512))
    assert full_pair[1] > 2 * hazy_pair[1]
    with density(editor, D):
        outs, ms = editor.edit_batch([full, hazy], [PROMPT, PROMPT], metrics=True, **KW)
    assert [(m["canny_low"], m["canny_high"]) for m in ms] == [full_pair, hazy_pair] == editor.last_canny_thresholds()
    for im, out, (low, high) in zip((full, hazy), outs, (full_pair, hazy_pair)):
        assert _close(out, editor.edit(im, PROMPT, canny_low_threshold=low, canny_high_threshold=high, **KW))


def test_edit_sweep_carries_one_pair(editor, hazy, hazy_pair, hazy_auto):
    with density(editor, D):
        images, variants = editor.edit_sweep(hazy, PROMPT, strengths=[0.6, 0.3], seed=9, resolution=(512, 512))
    assert len(images) == 2 and all((v["canny_low"], v["canny_high"]) == hazy_pair for v in variants)
    assert editor.last_canny_thresholds() == [hazy_pair] and _close(images[0], hazy_auto)
    low, high = hazy_pair
    explicit, _ = editor.edit_sweep(hazy, PROMPT, strengths=[0.6, 0.3], canny_low_threshold=low, canny_high_threshold=high, seed=9, resolution=(512, 512))
    assert all(np.array_equal(np.asarray(a), np.asarray(b)) for a, b in zip(images, explicit))


def test_tiles_take_one_pair_from_the_whole_source(editor):
    """700 x 560 at overlap 64: 2 x 2 tiles of 512 x 512.  The pair comes from the whole source at its own size and every tile job gets it as
    explicit thresholds."""
    img = Image.fromarray(oracle.to_u8(oracle.low_contrast(oracle.disks_float(3, 560, 700))))
    tiled = dict(tiles=(512, 512), tile_overlap=64, seed=9, strength=0.6)
    low, high = editor.canny_thresholds(img, D, tiles=(512, 512))
    assert (low, high) == oracle.thresholds(np.asarray(img), oracle.budget(700 * 560, D))
    with density(editor, D):
        out, m = editor.edit(img, PROMPT, metrics=True, **tiled)
    assert out.size == (700, 560) and (m["canny_low"], m["canny_high"]) == (low, high)
    assert np.array_equal(np.asarray(out), np.asarray(editor.edit(img, PROMPT, canny_low_threshold=low, canny_high_threshold=high, **tiled)))
    assert not np.array_equal(np.asarray(out), np.asarray(editor.edit(img, PROMPT, **tiled)))


def test_none_changes_nothing(editor, hazy, monkeypatch):
    """set_canny_density(None) behind a density is the editor that never had one: the same bytes, no key, none of the new entries."""
    assert editor.canny_density is None
    want = np.asarray(editor.edit(hazy, PROMPT, **KW))
    want_b = [np.asarray(o) for o in editor.edit_batch([hazy, hazy], [PROMPT, PROMPT], **KW)]
    want_s = [np.asarray(o) for o in editor.edit_sweep(hazy, PROMPT, strengths=[0.6, 0.3], seed=9, resolution=(512, 512))[0]]
    with density(editor, D):
        assert not np.array_equal(np.asarray(editor.edit(hazy, PROMPT, **KW)), want)
        assert editor.set_canny_density(None) == D

        def boom(*a, **k):
            raise AssertionError("canny_density=None must not reach the new entries")
        for name in ("fie_canny_rgb_device_begin_auto_u8", "fie_canny_thresholds_device_u8"):
            monkeypatch.setattr(hip.lib(), name, boom)
        out, m = editor.edit(hazy, PROMPT, metrics=True, **KW)
        assert np.array_equal(np.asarray(out), want) and set(m) == {"ssim", "psnr", "mse"} and editor.last_canny_thresholds() == [None]
        got = editor.edit_batch([hazy, hazy], [PROMPT, PROMPT], **KW)
        assert all(np.array_equal(np.asarray(g), w) for g, w in zip(got, want_b)) and editor.last_canny_thresholds() == [None, None]
        got, variants = editor.edit_sweep(hazy, PROMPT, strengths=[0.6, 0.3], seed=9, resolution=(512, 512))
        assert all(np.array_equal(np.asarray(g), w) for g, w in zip(got, want_s)) and all("canny_low" not in v for v in variants)
    assert editor.canny_density is None


def test_constructor_keyword(fie, hazy, hazy_pair, hazy_auto):
    """FastEditor(canny_density=d) is set_canny_density(d) from the start."""
    from src.pipeline import FastEditor
    other = FastEditor(model_name="tiny", enable_cpu_offload=False, canny_density=D)
    assert other.canny_density == D and np.array_equal(np.asarray(other.edit(hazy, PROMPT, **KW)), hazy_auto)
    assert other.last_canny_thresholds() == [hazy_pair]
