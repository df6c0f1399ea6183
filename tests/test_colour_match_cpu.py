"""Colour match, the definition (no GPU): `fie_amd/colour.py` -- the statistics against a plain Python loop, the region
threshold, the properties the definition promises (identity, monotone LUTs, the flat edit, the gain clamps, the widths at the largest image), the
range of the amount, and a synthetic check of purpose."""
import numpy as np
import pytest

import fie_amd  # noqa: F401
from fie_amd import colour

import colour_match_oracle as co

IDENT = np.tile(np.arange(256, dtype=np.uint8), (3, 1))


def _lut(e, s, l, a):
    """lut_numpy, with what holds for every LUT: shape, monotone, and match_numpy is the LUT applied."""
    lut, rep = colour.lut_numpy(e, s, l, a)
    assert lut.dtype == np.uint8 and lut.shape == (3, 256) and (np.diff(lut.astype(int), axis=1) >= 0).all()
    assert all(512 <= g <= 2048 for g in rep["gain"]) and rep["shift"] == [int(lut[c, 128]) - 128 for c in range(3)]
    out = colour.match_numpy(e, s, l, a)
    assert out.dtype == np.uint8 and all(np.array_equal(out[..., c], lut[c][e[..., c]]) for c in range(3))
    words = [int(rep["region"] == "background")] + rep["gain"] + rep["shift"] + [rep["n"]]
    assert colour.report_dict(words) == dict(colour_gain=[g / 1024 for g in rep["gain"]], colour_shift=rep["shift"], colour_region=rep["region"])
    return lut, rep


# ---------------------------------------------------------------------------------------------------------------- 1. statistics and LUT
@pytest.mark.parametrize("masked", [False, True], ids=["nomask", "mask"])
@pytest.mark.parametrize("size", co.SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_statistics_are_the_plain_sums(size, masked):
    e, s, l = co.case(*size, seed=size[0] * 1000 + size[1])
    st = colour.stats_numpy(e, s, l if masked else None)
    want = [0] * 26
    for y in range(size[0]):
        for x in range(size[1]):
            o = 13 if masked and l[y, x] >= 128 else 0
            want[o] += 1
            for c in range(3):
                ev, sv = int(e[y, x, c]), int(s[y, x, c])
                want[o + 1 + c] += ev; want[o + 4 + c] += ev * ev; want[o + 7 + c] += sv; want[o + 10 + c] += sv * sv
    assert st == want and all(isinstance(v, int) for v in st)


@pytest.mark.parametrize("a", co.AMOUNTS)
@pytest.mark.parametrize("masked", [False, True], ids=["nomask", "mask"])
@pytest.mark.parametrize("size", co.SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_lut_on_the_seeded_cases(size, masked, a):
    e, s, l = co.case(*size, seed=size[0] * 1000 + size[1])
    lut, rep = _lut(e, s, l if masked else None, a)
    if a == 256 and size[0] * size[1] >= 64 * 64:                                      # the cast of the case is 0.8x / 1.1x / 1.0x: the gains undo it
        assert abs(rep["gain"][0] / 1024 - 1 / 0.8) < 0.05 and abs(rep["gain"][1] / 1024 - 1 / 1.1) < 0.05 and abs(rep["gain"][2] / 1024 - 1) < 0.05
    if a == 1:                                                                         # 1 / 256 of the way: no level moves by more than one
        assert np.abs(lut.astype(int) - IDENT).max() <= 1


def test_means_agree_after_the_match():
    rng = np.random.default_rng(9)
    e, s = rng.integers(0, 256, (40, 56, 3), dtype=np.uint8), rng.integers(32, 224, (40, 56, 3), dtype=np.uint8)
    _, rep = _lut(e, s, None, 256)
    assert all(700 < g < 840 for g in rep["gain"])                                     # 0.75 of the contrast: inside the clamp, nothing clips
    out = colour.match_numpy(e, s, None, 256)
    for c in range(3):
        assert abs(float(out[..., c].mean()) - float(s[..., c].mean())) < 1.0
        assert abs(float(out[..., c].std()) - float(s[..., c].std())) < 1.0


# ---------------------------------------------------------------------------------------------------------------- 2. the region threshold
def test_region_threshold():
    """64 x 64: ceil(4096 / 16) = 256 background pixels are enough, 255 are not."""
    e, s, _ = co.case(64, 64, seed=1)
    lut_few, rep_few = _lut(e, s, co.mask_with_background(64, 64, 255), 256)
    lut_enough, rep_enough = _lut(e, s, co.mask_with_background(64, 64, 256), 256)
    assert rep_few["region"] == "image" and rep_few["n"] == 4096
    assert rep_enough["region"] == "background" and rep_enough["n"] == 256
    assert np.array_equal(lut_few, colour.lut_numpy(e, s, None, 256)[0])              # the fallback is the whole image's LUT
    assert not np.array_equal(lut_enough, lut_few)
    for l, region in ((np.full((64, 64), 255, np.uint8), "image"), (np.zeros((64, 64), np.uint8), "background"), (np.full((64, 64), 127, np.uint8), "background"),
                      (np.full((64, 64), 128, np.uint8), "image")):
        assert _lut(e, s, l, 256)[1]["region"] == region


# ---------------------------------------------------------------------------------------------------------------- 3. properties
@pytest.mark.parametrize("a", co.AMOUNTS)
def test_identity_when_edit_equals_source_on_the_region(a):
    e, s, l = co.case(48, 72, seed=2)
    lut, rep = _lut(s, s, None, a)
    assert np.array_equal(lut, IDENT) and rep["gain"] == [1024] * 3 and rep["shift"] == [0] * 3
    mixed = np.where((l >= 128)[..., None], e, s)                                      # differs inside the mask only
    lut, rep = _lut(mixed, s, l, a)
    assert rep["region"] == "background" and np.array_equal(lut, IDENT)
    assert not np.array_equal(_lut(mixed, s, None, a)[0], IDENT) or a == 1


def test_flat_edit_has_gain_one():
    rng = np.random.default_rng(3)
    s = rng.integers(0, 256, (20, 30, 3), dtype=np.uint8)
    e = np.empty_like(s)
    e[:] = (10, 128, 250)
    lut, rep = _lut(e, s, None, 256)
    assert rep["gain"] == [1024] * 3
    for c, v in enumerate((10, 128, 250)):                                             # the flat level moves to the source's mean, rounded
        n, ss = 600, int(s[..., c].astype(np.int64).sum())
        assert int(lut[c, v]) == min(max((1024 * ss + 512 * n) // (1024 * n), 0), 255)
    assert _lut(np.zeros_like(s), np.zeros_like(s), None, 256)[1]["gain"] == [1024] * 3


def test_gain_clamps():
    rng = np.random.default_rng(4)
    s = rng.integers(64, 192, (32, 32, 3), dtype=np.uint8)
    assert _lut(co.cast(s, 0.25, 96.0), s, None, 256)[1]["gain"] == [2048] * 3         # a quarter of the contrast: the map wants 4x
    low = rng.integers(112, 144, (32, 32, 3), dtype=np.uint8)
    assert _lut(co.cast(low, 4.0, -384.0), low, None, 256)[1]["gain"] == [512] * 3     # four-fold contrast: the map wants 0.25x
    assert all(512 <= g <= 540 for g in _lut(co.cast(low, 2.0, -128.0), low, None, 256)[1]["gain"])
    assert colour.gain_q10(100, 0, 100, 0, 100) == 1024 and colour.gain_q10(100, 0, 100, 0, 400) == 2048 and colour.gain_q10(100, 0, 400, 0, 100) == 512
    assert colour.gain_q10(100, 0, 400, 0, 900) == 1536


def test_widths_at_the_largest_image():
    """2^22 pixels of 255 against 0: every sum at its largest; n Qe = 2^44 * 65025 < 2^61, so the definition fits 64-bit integers."""
    e, s = np.full((2048, 2048, 3), 255, np.uint8), np.zeros((2048, 2048, 3), np.uint8)
    st = colour.stats_numpy(e, s)
    assert st[0] == 1 << 22 and st[1:4] == [255 << 22] * 3 and st[4:7] == [65025 << 22] * 3 and st[7:13] == [0] * 6 and st[13:] == [0] * 13
    assert st[0] * st[4] < 1 << 61 and 2048 * 2048 * ((st[0] * st[4]) // st[0]) < 1 << 61 and 2048 * (255 * st[0]) + 1024 * st[1] + 512 * st[0] < 1 << 61
    lut, rep = colour.lut_numpy(e, s, None, 256)
    assert rep["gain"] == [1024] * 3 and rep["n"] == 1 << 22 and rep["shift"] == [-128] * 3 and int(lut.max()) == 0
    lut, rep = colour.lut_numpy(s, e, None, 128)
    assert int(lut[1, 0]) == 128 and rep["shift"] == [64] * 3
    for big in ((2049, 2048), (1, (1 << 22) + 1)):
        with pytest.raises(ValueError, match="2\\^22"):
            colour.lut_numpy(np.zeros(big + (3,), np.uint8), np.zeros(big + (3,), np.uint8))


def test_purpose_a_known_cast_comes_back():
    """Disks on a gradient under a known per-channel cast, outside and inside a mask: the matched image is closer to the uncast picture."""
    src = co.disks_on_gradient(96)
    e = co.cast(src, (0.8, 1.1, 1.0), (30, -10, 12))
    l = np.zeros((96, 96), np.uint8)
    l[24:72, 30:80] = 255
    for mask in (None, l):
        got = colour.match_numpy(e, src, mask)
        before, after = np.abs(e.astype(int) - src).mean(), np.abs(got.astype(int) - src).mean()
        print(f"purpose, mask={mask is not None}: mean absolute error to the uncast image {before:.3f} -> {after:.3f}")
        assert after < before


# ---------------------------------------------------------------------------------------------------------------- 4. arguments
def test_check_ranges():
    assert colour.check(None) is None and colour.check(1) == 1.0 and colour.check(0.5) == 0.5
    assert colour.amount_q8(1.0) == 256 and colour.amount_q8(0.5) == 128 and colour.amount_q8(0.001) == 1 and colour.amount_q8(1 / 256) == 1
    for bad in (0, 0.0, -0.1, 1.01, 2, True, "1", float("nan"), [1.0]):
        with pytest.raises(ValueError, match="colour_match"):
            colour.check(bad)
    z = np.zeros((2, 2, 3), np.uint8)
    for bad in (0, 257, 1.0, True):
        with pytest.raises(ValueError):
            colour.lut_numpy(z, z, None, bad)
    for bad in (lambda: colour.stats_numpy(z, np.zeros((2, 3, 3), np.uint8)), lambda: colour.stats_numpy(z, z, np.zeros((2, 3), np.uint8)),
                lambda: colour.stats_numpy(z.astype(np.int32), z), lambda: colour.stats_numpy(z[..., :2], z[..., :2])):
        with pytest.raises(ValueError):
            bad()
