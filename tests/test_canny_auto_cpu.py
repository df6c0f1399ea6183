"""Edge-budget Canny without a GPU: the numpy restatement against a sort-based brute force of the definition, the host C++
entry against the restatement, what the rule does to low-contrast and cluttered images, the floor of 16, the host logic of the `canny_density`
setting behind a stub device and the ABI's new names."""
import os
import re
import threading
import types

import numpy as np
import pytest
from PIL import Image

import fie_amd  # noqa: F401
from fie_amd import canny_auto as hcanny, hip
from oracle import canny as ocanny

import canny_auto_oracle as oracle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(8, 8), (5, 3), (33, 70), (97, 131), (64, 64), (256, 256)]          # the GPU test's shapes (1024 x 1024 runs there, once)
NEW_ENTRIES = ("fie_canny_auto_workspace_bytes", "fie_canny_rgb_device_begin_auto_u8", "fie_canny_thresholds_device_u8", "fie_canny_auto_thresholds_u8")


@pytest.fixture(scope="module")
def lib():
    hip.build()
    return hip.lib()


# ---------------------------------------------------------------- 1. the restatement against brute force
def brute_ridge(rgb):
    """Rule 1, pixel by pixel in Python integers."""
    gray = ocanny.rgb_to_gray(rgb).astype(int)
    h, w = gray.shape
    g = lambda y, x: int(gray[min(max(y, 0), h - 1), min(max(x, 0), w - 1)])
    dx, dy = np.zeros((h, w), int), np.zeros((h, w), int)
    for y in range(h):
        for x in range(w):
            dx[y, x] = (g(y - 1, x + 1) + 2 * g(y, x + 1) + g(y + 1, x + 1)) - (g(y - 1, x - 1) + 2 * g(y, x - 1) + g(y + 1, x - 1))
            dy[y, x] = (g(y + 1, x - 1) + 2 * g(y + 1, x) + g(y + 1, x + 1)) - (g(y - 1, x - 1) + 2 * g(y - 1, x) + g(y - 1, x + 1))
    mag = np.abs(dx) + np.abs(dy)
    m = lambda y, x: int(mag[y, x]) if 0 <= y < h and 0 <= x < w else 0
    tg22 = int(0.4142135623730950488016887242097 * (1 << 15) + 0.5)
    r = np.zeros((h, w), int)
    for y in range(h):
        for x in range(w):
            c, ax, ay = m(y, x), abs(int(dx[y, x])), abs(int(dy[y, x])) << 15
            if ay < ax * tg22:
                keep = c > m(y, x - 1) and c >= m(y, x + 1)
            elif ay > ax * tg22 + (ax << 16):
                keep = c > m(y - 1, x) and c >= m(y + 1, x)
            else:
                s = -1 if (int(dx[y, x]) ^ int(dy[y, x])) < 0 else 1
                keep = c > m(y - 1, x - s) and c > m(y + 1, x + s)
            r[y, x] = c if keep else 0
    return r


def brute_thresholds(r, pixels, density, lo, hi):
    """Rules 2-4 on the sorted ridge values: the budget in plain integers, the first h that leaves few enough above it."""
    seeds = max(1, pixels * int(round(density * 10 ** 6)) // 10 ** 6)
    ordered = np.sort(r.ravel())
    lo, hi = min(lo, hi), max(lo, hi)
    for h in range(16, 2041):
        if len(ordered) - np.searchsorted(ordered, h, side="right") <= seeds:
            return h * lo // hi, h
    raise AssertionError("no threshold up to 2040")


def _random_images():
    rng = np.random.default_rng(7)
    for h, w in ((1, 1), (2, 7), (9, 9), (31, 33), (64, 64), (40, 64)):
        yield rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
        smooth = np.cumsum(rng.integers(-20, 21, (h, w, 3)), axis=1).clip(-128, 127) + 128
        yield smooth.astype(np.uint8)
    yield oracle.stripes(24, 40)                    # ties only: every ridge pixel has one magnitude
    yield oracle.stripes(24, 40, 3)
    yield oracle.long_chain(32, 64)                 # ties but for one seed
    yield np.kron(np.indices((6, 6)).sum(0) % 2, np.ones((8, 8), int))[..., None].repeat(3, 2).astype(np.uint8) * 255      # a checkerboard
    yield oracle.flat(16, 16)
    yield oracle.plus_minus_one(32, 32)


def test_restatement_equals_brute_force():
    for img in _random_images():
        r = oracle.ridge(img)
        assert np.array_equal(r, brute_ridge(img)) and 0 <= r.min() and r.max() <= 2040
        n = img.shape[0] * img.shape[1]
        for d in (0.001, 0.01, 0.02, 0.1, 0.25):
            assert oracle.budget(n, d) == max(1, n * int(round(d * 10 ** 6)) // 10 ** 6)
            for lo, hi in ((100, 200), (200, 100), (1, 3), (0, 5), (7, 7)):
                got = oracle.thresholds(img, oracle.budget(n, d), lo, hi)
                assert got == brute_thresholds(r, n, d, lo, hi), (img.shape, d, lo, hi)
                low, high = got
                above = lambda h: int((r > h).sum())
                assert 16 <= high <= 2040 and above(high) <= oracle.budget(n, d) and (high == 16 or above(high - 1) > oracle.budget(n, d))
                assert low == high * min(lo, hi) // max(lo, hi)


def test_ridge_is_the_candidate_set_of_the_oracle_at_every_threshold():
    """Rule 1's claim: the direction test does not depend on the thresholds, so Canny(low, high) is the hysteresis of r > low seeded by r > high."""
    from scipy import ndimage
    img = oracle.to_u8(oracle.disks_float(1, 64, 80))
    r = oracle.ridge(img)
    for low, high in ((10, 30), (50, 150), (100, 200), (300, 301)):
        lab, n = ndimage.label(r > low, structure=np.ones((3, 3), bool))
        keep = np.zeros(n + 1, bool)
        keep[np.unique(lab[r > high])] = True
        keep[0] = False
        assert np.array_equal(keep[lab].astype(np.uint8) * 255, ocanny.canny_rgb(img, low, high)[..., 0])


# ---------------------------------------------------------------- 2. the host C++ entry
def _budgets(n):
    return sorted({1, max(1, n // 50), max(1, n // 4)})


def _shape_image(h, w):
    return oracle.to_u8(oracle.disks_float(h * 1000 + w, h, w, disks=10))


@pytest.mark.parametrize("h,w", SHAPES)
def test_host_entry_equals_restatement(lib, h, w):
    img = _shape_image(h, w)
    for seeds in _budgets(h * w):
        assert hip.canny_auto_thresholds(img, seeds) == oracle.thresholds(img, seeds)
    assert hip.canny_auto_thresholds(img, _budgets(h * w)[1], 150, 50) == oracle.thresholds(img, _budgets(h * w)[1], 50, 150)      # lo > hi is swapped


def test_host_entry_on_the_special_images(lib):
    for img in (oracle.stripes(64, 1024), oracle.stripes(256, 256), oracle.stripes(64, 1024, 3), oracle.stripes(256, 256, 3), oracle.long_chain(64, 1024), oracle.long_chain(256, 256), oracle.flat(64, 1024),
                oracle.plus_minus_one(256, 256)):
        n = img.shape[0] * img.shape[1]
        for seeds in _budgets(n):
            assert hip.canny_auto_thresholds(img, seeds) == oracle.thresholds(img, seeds)
    chain = oracle.long_chain(64, 1024)
    assert oracle.thresholds(chain, 1)[1] >= 120 > oracle.thresholds(chain, 64 * 1024 // 4)[1]      # > against >=: the ties at 120 stay under a high of 120


def test_host_entry_refuses_bad_arguments(lib):
    img = np.zeros((4, 4, 3), np.uint8)
    pair = (hip.ctypes.c_int * 2)()
    for h, w, seeds, lo, hi in ((0, 4, 1, 100, 200), (4, 4, 0, 100, 200), (4, 4, 17, 100, 200), (4, 4, 1, 0, 0), (4, 4, 1, -1, 200)):
        assert lib.fie_canny_auto_thresholds_u8(img.ctypes.data, h, w, seeds, lo, hi, pair) == hip.header.DEFINES["EINVAL"]
        assert b"bad argument" in lib.fie_last_error()
    assert lib.fie_canny_auto_workspace_bytes(0, 5) == -1 and lib.fie_canny_auto_workspace_bytes(1 << 16, 1 << 15) == -1
    need = lib.fie_canny_auto_workspace_bytes(33, 70)
    assert need >= 33 * 70 * 3 + 2048 * 4 + 24 and need >= lib.fie_canny_workspace_bytes(33, 70)


# ---------------------------------------------------------------- 3. what the rule does (numbers: DESIGN.md section 22)
def _density(edges):
    return float((edges[..., 0] > 0).mean())


def _iou(a, b):
    a, b = a[..., 0] > 0, b[..., 0] > 0
    return float((a & b).sum()) / float((a | b).sum())


@pytest.mark.parametrize("seed", range(4))
def test_low_contrast_copy_keeps_its_edge_map(seed):
    x = oracle.disks_float(seed)
    full, hazy = oracle.to_u8(x), oracle.to_u8(oracle.low_contrast(x))
    seeds = oracle.budget(256 * 256, 0.01)
    auto_full, auto_hazy = oracle.canny_auto(full, seeds)[0], oracle.canny_auto(hazy, seeds)[0]
    print(f"seed {seed}: fixed full {_density(ocanny.canny_rgb(full)):.4f} hazy {_density(ocanny.canny_rgb(hazy)):.4f}; auto full "
          f"{_density(auto_full):.4f} hazy {_density(auto_hazy):.4f}, IoU {_iou(auto_hazy, auto_full):.3f}")
    assert _iou(auto_hazy, auto_full) >= 0.8
    assert _density(ocanny.canny_rgb(hazy)) < 0.005 and _density(auto_hazy) >= 0.01


@pytest.mark.parametrize("seed", range(4))
def test_clutter_is_not_nailed_to_its_noise(seed):
    img = oracle.clutter(seed)
    fixed, auto = _density(ocanny.canny_rgb(img)), _density(oracle.canny_auto(img, oracle.budget(256 * 256, 0.02))[0])
    print(f"seed {seed}: fixed {fixed:.3f}, auto at 2 % {auto:.3f}")
    assert auto < fixed / 2


# ---------------------------------------------------------------- 4. the floor
@pytest.mark.parametrize("img", [oracle.flat(64, 64), oracle.plus_minus_one(64, 64), oracle.plus_minus_one(97, 131, seed=3)], ids=["flat", "pm1", "pm1-odd"])
def test_floor_of_16(lib, img):
    n = img.shape[0] * img.shape[1]
    assert oracle.ridge(img).max() <= 16
    for seeds in (1, n // 4):
        edges, (low, high) = oracle.canny_auto(img, seeds)
        assert (low, high) == (8, 16) and edges.max() == 0
        assert hip.canny_auto_thresholds(img, seeds) == (8, 16)


# ---------------------------------------------------------------- 5. host logic behind a stub device
def test_keyword_range_and_ratio_errors():
    for bad in (0, 0.0005, 0.3, 1, True, "0.01", [0.01], float("nan")):
        with pytest.raises(ValueError, match="canny_density"):
            hcanny.check_density(bad)
    assert hcanny.check_density(None) is None and hcanny.check_density(0.001) == 0.001 and hcanny.check_density(0.25) == 0.25
    with pytest.raises(ValueError, match="0 / 0"):
        hcanny.check(0.01, 0, 0)
    for lo, hi in ((-1, 200), (100.0, 200), (True, 200), (100, None)):
        with pytest.raises(ValueError, match="integers >= 0"):
            hcanny.check(0.01, lo, hi)
    assert hcanny.check(None, 0, 0) is None and hcanny.check(0.02, 200, 100) == 0.02          # without a density the pair is not this check's
    assert hcanny.check_ratio(200, 100) == (100, 200) and hcanny.check_ratio(0, 5) == (0, 5)
    assert hcanny.budget(1024 * 1024, 0.01) == 10485 and hcanny.budget(64, 0.001) == 1 and hcanny.budget(10 ** 9, 0.25) == 25 * 10 ** 7
    assert hcanny.low_of(57, 100, 200) == 28 and hcanny.low_of(16, 0, 5) == 0


def _stub_editor():
    """A FastEditor with no device behind it: the device jobs, the tiled tail and the threshold read-back record their arguments and the density
    the job would hand its Canny (FastEditor._density)."""
    from src.pipeline import FastEditor
    ed = FastEditor.__new__(FastEditor)
    ed._tls, ed.jobs, ed.asked = threading.local(), [], []

    def single(image, prompt, negative_prompt, k, resolution, mask_l, margins, spec, metrics, full, kw, select=None):
        ed.jobs.append(("single", image.size, dict(kw), ed._density(kw)))
        return types.SimpleNamespace(images=[image] * k, extra=None, canny_pair=(11, 22) if ed._density(kw) is not None else None)

    def batch(images, prompts, negative_prompts, size, mask_ls, margins, spec, metrics, full, kw, after=None):
        ed.jobs.append(("batch", [im.size for im in images], dict(kw), ed._density(kw)))
        return types.SimpleNamespace(images=list(images), extra=None, canny_pairs=[None] * len(images)), [None] * len(images)

    def tiled(image, prompt, negative_prompt, plan, tile_batch, mask_l, spec, metrics, kw):
        ed.jobs.append(("tiled", image.size, dict(kw), ed._density(kw)))
        return (image, {}) if metrics else image

    def thresholds(image, canny_density, canny_low_threshold=100, canny_high_threshold=200, resolution=None, outpaint=None, mask=None, *, tiles=None):
        ed.asked.append((image.size, canny_density, canny_low_threshold, canny_high_threshold, tiles))
        return 33, 66

    ed._single_job, ed._batch_job, ed._edit_tiled, ed.canny_thresholds = single, batch, tiled, thresholds
    ed._scores = lambda extra, has_mask: [{} for _ in has_mask]
    return ed


def test_errors_come_before_any_device_work():
    from src.pipeline import FastEditor
    ed = FastEditor.__new__(FastEditor)              # no pipe, no context: anything past the checks is an AttributeError
    img = Image.new("RGB", (64, 64))
    assert ed.canny_density is None
    for bad in (0.5, 0.0001, "dense", True):
        for call in (ed.set_canny_density, lambda d: ed.preprocess_image(img, canny_density=d), lambda d: ed.canny_thresholds(img, d)):
            with pytest.raises(ValueError, match="canny_density"):
                call(bad)
        assert ed.canny_density is None              # a refused value leaves the setting alone
    with pytest.raises(ValueError, match="0 / 0"):
        ed.canny_thresholds(img, 0.01, 0, 0)
    with pytest.raises(ValueError, match="canny_density=None"):
        ed.canny_thresholds(img, None)
    assert ed.set_canny_density(0.01) is None and ed.canny_density == 0.01
    for call in (lambda **k: ed.edit(img, "p", **k), lambda **k: ed.edit_batch([img], ["p"], **k), lambda **k: ed.edit_sweep(img, "p", **k)):
        with pytest.raises(ValueError, match="0 / 0"):
            call(canny_low_threshold=0, canny_high_threshold=0)
        with pytest.raises(ValueError, match="integers >= 0"):
            call(canny_low_threshold=-5)
        with pytest.raises(AttributeError):          # a legal ratio passes the checks and reaches for the device
            call()
    assert ed.set_canny_density(None) == 0.01 and ed.canny_density is None


def test_constructor_reads_the_keyword_and_the_environment(monkeypatch):
    """The density is checked in front of everything else the constructor does: a bad one is refused before the device is looked for."""
    from src.pipeline import FastEditor
    with pytest.raises(ValueError, match="canny_density"):
        FastEditor(model_name="tiny", device="cpu", canny_density=0.9)
    monkeypatch.setenv("FIE_CANNY_DENSITY", "dense")
    with pytest.raises(ValueError, match="FIE_CANNY_DENSITY"):
        FastEditor(model_name="tiny", device="cpu")
    monkeypatch.setenv("FIE_CANNY_DENSITY", "0.5")
    with pytest.raises(ValueError, match="canny_density"):
        FastEditor(model_name="tiny", device="cpu")
    monkeypatch.setenv("FIE_CANNY_DENSITY", "0.02")
    with pytest.raises(RuntimeError, match="device='cpu'"):          # a good one passes on to the next check
        FastEditor(model_name="tiny", device="cpu")


def test_setting_reaches_the_jobs():
    ed = _stub_editor()
    img = Image.new("RGB", (96, 64))
    ed.set_canny_density(0.02)
    ed.edit(img, "p", canny_low_threshold=200, canny_high_threshold=50)
    kind, _, kw, density = ed.jobs[-1]
    assert kind == "single" and density == 0.02 and (kw["canny_low_threshold"], kw["canny_high_threshold"]) == (200, 50)
    assert ed.last_canny_thresholds() == [(11, 22)]
    assert ed.edit(img, "p", metrics=True)[1] == dict(canny_low=11, canny_high=22)
    ed.set_canny_density(None)
    ed.edit(img, "p")
    assert ed.jobs[-1][3] is None and ed.last_canny_thresholds() == [None]
    assert ed.edit(img, "p", metrics=True)[1] == {}                           # no density, no key
    ed.set_canny_density(0.03)
    ed.edit_batch([img, img], ["p", "q"])
    assert ed.jobs[-1][0] == "batch" and ed.jobs[-1][3] == 0.03
    ed.edit_batch([img, Image.new("RGB", (64, 128))], ["p", "q"], resolution="auto")          # two target sizes: two jobs
    assert [j[0] for j in ed.jobs[-2:]] == ["batch", "batch"] and all(j[3] == 0.03 for j in ed.jobs[-2:])
    ed.set_canny_density(0.01)
    images, variants = ed.edit_sweep(img, "p")
    kind, _, kw, density = ed.jobs[-1]
    assert kind == "single" and density == 0.01 and isinstance(kw["strength"], list) and len(images) == len(variants) == 4
    assert all((v["canny_low"], v["canny_high"]) == (11, 22) for v in variants)          # one pair for the sweep
    ed.set_canny_density(None)
    assert all("canny_low" not in v for v in ed.edit_sweep(img, "p")[1])


def test_tiles_take_one_pair_from_the_whole_image_and_forward_integers():
    ed = _stub_editor()
    img = Image.new("RGB", (700, 560))
    ed.set_canny_density(0.01)
    out, info = ed.edit(img, "p", tiles=(512, 512), tile_overlap=64, canny_low_threshold=50, canny_high_threshold=150, metrics=True)
    assert ed.asked == [((700, 560), 0.01, 50, 150, (512, 512))]                # one call, on the whole source
    kind, size, kw, density = ed.jobs[-1]
    assert kind == "tiled" and size == (700, 560) and density is None          # the tile jobs get the pair, not the density
    assert (kw["canny_low_threshold"], kw["canny_high_threshold"]) == (33, 66) and all(type(kw[k]) is int for k in ("canny_low_threshold", "canny_high_threshold"))
    assert info == dict(canny_low=33, canny_high=66) and ed.last_canny_thresholds() == [(33, 66)]
    ed.edit_batch([img, img], ["p", "q"], tiles=(512, 512), tile_overlap=64)
    assert len(ed.asked) == 3 and ed.last_canny_thresholds() == [(33, 66), (33, 66)]     # every image of a batch is tiled, and asked, on its own
    ed.set_canny_density(None)
    ed.edit(img, "p", tiles=(512, 512), tile_overlap=64)
    assert len(ed.asked) == 3 and ed.jobs[-1][2]["canny_low_threshold"] == 100          # without a density nothing is asked


def test_region_re_enters_under_the_setting():
    ed = _stub_editor()
    img = Image.new("RGB", (300, 200))
    ed.set_canny_density(0.05)
    out = ed.edit(img, "p", region=(20, 30, 148, 158))
    kind, size, kw, density = ed.jobs[-1]
    assert kind == "single" and size == (128, 128) and density == 0.05 and out.size == (300, 200)      # the crop's own statistics


def test_command_lines():
    """run_single_image.py has the flag; run_batch.py's option set is fixed, so a batch run takes the density from FIE_CANNY_DENSITY."""
    import run_single_image
    one = ["--image", "i.png", "--prompt", "p"]
    assert run_single_image.full_parser().parse_args(one).canny_density is None
    assert run_single_image.full_parser().parse_args(one + ["--canny_density", "0.015"]).canny_density == 0.015


def test_run_batch_writes_each_images_pair(tmp_path):
    """With a density set on the editor every row of --results_json's rows carries the pair its image got; without one no row has the keys."""
    import run_batch

    class Editor:
        def __init__(self, canny_density):
            self.canny_density, self.n = canny_density, 0

        def edit(self, image, prompt, **kw):
            assert "canny_density" not in kw
            self.n += 1
            return Image.new("RGB", (8, 8))

        def last_canny_thresholds(self):
            return [(10 * self.n, 20 * self.n)]

        def clear_memory(self):
            pass

    src = tmp_path / "src"
    src.mkdir()
    entries = []
    for i in range(2):
        Image.new("RGB", (16, 16), (i, i, i)).save(src / f"{i}.png")
        entries.append((i, str(i), {"image_path": f"{i}.png", "editing_prompt": "p"}))
    args = run_batch.full_parser().parse_args(["--source_dir", str(src), "--output_dir", str(tmp_path / "o")])
    res = run_batch.process_shard(Editor(0.02), entries, args, str(tmp_path / "o" / "e"), str(tmp_path / "o" / "c"))
    assert res["processed"] == 2 and [(r["canny_low"], r["canny_high"]) for r in res["rows"]] == [(10, 20), (20, 40)]
    args = run_batch.full_parser().parse_args(["--source_dir", str(src), "--output_dir", str(tmp_path / "p")])
    res = run_batch.process_shard(Editor(None), entries, args, str(tmp_path / "p" / "e"), str(tmp_path / "p" / "c"))
    assert res["processed"] == 2 and all("canny_low" not in r for r in res["rows"])


# ---------------------------------------------------------------- 6. the ABI
def test_header_declares_and_library_exports_the_entries(lib):
    with open(os.path.join(ROOT, "include", "fie.h")) as fh:
        text = fh.read()
    for name in NEW_ENTRIES:
        assert re.search(r"\b%s\s*\(" % name, text), name
        assert name in hip.SIGNATURES and hasattr(lib, name), name
    assert hip.header.FUNCTIONS["fie_canny_auto_workspace_bytes"][0] is hip.ctypes.c_int64
    assert hip.header.FUNCTIONS["fie_canny_rgb_device_begin_auto_u8"][1][4] is hip.ctypes.c_int64          # the budget
