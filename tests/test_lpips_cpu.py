"""LPIPS, the device-free half: the input table, the map sizes, the two directory forms and their errors, the directory
lookup, the exported symbols, the CPU calculator, the command-line plumbing and the oracle's own controls (tests/lpips_oracle.py)."""
import csv
import json

import numpy as np
import pytest
import torch
import torch.nn.functional as F
from PIL import Image

import lpips_oracle as lo

import fie_amd  # noqa: F401,E402
from fie_amd import lpips as hlpips


def test_input_lut_is_the_reference_arithmetic():
    """All 768 entries, bit for bit: the bytes as a [1, 3, 16, 16] image through `np.array(img).astype(float32) / 255`, `* 2 - 1` and the scaling
    layer's `(x - shift) / scale` with its [1, 3, 1, 1] buffers."""
    img = np.repeat(np.arange(256, dtype=np.uint8).reshape(16, 16, 1), 3, axis=2)
    x = torch.from_numpy(img.astype(np.float32) / 255.0).permute(2, 0, 1).unsqueeze(0)
    x = x * 2 - 1
    shift = torch.Tensor([-.030, -.088, -.188])[None, :, None, None]
    scale = torch.Tensor([.458, .448, .450])[None, :, None, None]
    want = ((x - shift) / scale)[0].reshape(3, 256)
    got = hlpips.input_lut()
    assert got.dtype == torch.float32 and got.shape == (3, 256) and got.is_contiguous()
    assert torch.equal(got.view(torch.int32), want.contiguous().view(torch.int32))
    assert torch.equal(got, lo.lut(torch.float32)) and (got.double() - lo.lut(torch.float64)).abs().max() < 1e-6


def test_feature_sizes_match_torch():
    """Every h, w in 32 .. 80 against the shapes torch gives (a one-channel stand-in: the sizes do not depend on the channels)."""
    k = torch.zeros(1, 1, 3, 3)
    for h in range(32, 81):
        for w in range(32, 81):
            x = F.conv2d(torch.zeros(1, 1, h, w), k, stride=2)
            want = [tuple(x.shape[2:])]
            for _ in range(3):
                x = F.max_pool2d(x, 3, 2, ceil_mode=True)
                want.append(tuple(x.shape[2:]))
            assert hlpips.feature_sizes(h, w) == [want[0], want[1], want[2], want[3], want[3], want[3], want[3]], (h, w)
    assert hlpips.feature_sizes(512, 512) == [(255, 255), (127, 127), (63, 63)] + [(31, 31)] * 4
    assert hlpips.feature_sizes(45, 67) == [(22, 33), (11, 16), (5, 8)] + [(2, 4)] * 4
    for bad in ((31, 64), (64, 31)):
        with pytest.raises(ValueError, match="32 x 32"):
            hlpips.feature_sizes(*bad)
    assert hlpips.TAP_CHANNELS == lo.CHANNELS and hlpips.TAPS == lo.TAPS and hlpips.FIRE == lo.FIRE and hlpips.POOLS == lo.POOLS


def test_both_directory_forms_load_the_same_tensors(tmp_path):
    a = hlpips.read_dir(lo.write_dir(tmp_path / "st", "safetensors"))
    b = hlpips.read_dir(lo.write_dir(tmp_path / "pth", "pth"))
    sd = lo.weights()
    assert set(a) == set(b) == set(hlpips.expected_shapes()) == set(sd) and len(a) == 2 + 6 * 8 + 7
    assert all(torch.equal(a[k], b[k]) and torch.equal(a[k], sd[k]) and a[k].dtype == torch.float32 for k in a)
    assert not any(k.startswith("classifier") for k in b)
    with pytest.raises(FileNotFoundError, match="model.safetensors"):
        hlpips.read_dir(str(tmp_path))


def test_missing_key_and_wrong_shape():
    sd = dict(lo.weights())
    for key in ("features.7.expand3x3.bias", "lin4.model.1.weight", "features.0.weight"):
        with pytest.raises(KeyError, match=key.replace(".", r"\.")):
            hlpips.check_tensors({k: v for k, v in sd.items() if k != key})
    bad = dict(sd)
    bad["features.9.squeeze.weight"] = torch.zeros(48, 128, 1, 1)
    with pytest.raises(ValueError, match=r"features\.9\.squeeze\.weight.*\(48, 128, 1, 1\).*\(48, 256, 1, 1\)"):
        hlpips.check_tensors(bad)
    bad = dict(sd)
    bad["lin0.model.1.weight"] = torch.zeros(64)
    with pytest.raises(ValueError, match=r"lin0\.model\.1\.weight.*\(64,\).*\(1, 64, 1, 1\)"):
        hlpips.check_tensors(bad)


def test_resolve_dir_precedence(monkeypatch, tmp_path):
    monkeypatch.delenv("FIE_LPIPS_DIR", raising=False)
    monkeypatch.delenv("FIE_WEIGHTS_DIR", raising=False)
    assert hlpips.resolve_dir(None) is None and hlpips.resolve_dir("x") == "x"
    monkeypatch.setenv("FIE_WEIGHTS_DIR", str(tmp_path))
    assert hlpips.resolve_dir(None) is None
    (tmp_path / "lpips").mkdir()
    assert hlpips.resolve_dir(None) == str(tmp_path / "lpips")
    monkeypatch.setenv("FIE_LPIPS_DIR", "/somewhere")
    assert hlpips.resolve_dir(None) == "/somewhere" and hlpips.resolve_dir("x") == "x"


def test_library_exports_the_new_symbols():
    from fie_amd import header, hip
    names = ("fie_lpips_stem_u8_f32", "fie_maxpool3s2_nhwc_f32", "fie_lpips_layer_workspace_bytes", "fie_lpips_layer_f32")
    lib = hip.lib()
    assert all(n in header.FUNCTIONS and hasattr(lib, n) for n in names)
    assert hip.ACT_RELU == 5 and header.DEFINES["ACT_RELU"] == 5
    assert lib.fie_lpips_layer_workspace_bytes(3, 65025) == 3 * 1017 * 8 and lib.fie_lpips_layer_workspace_bytes(0, 5) == -1
    assert hlpips.total([0.1, 0.2, 0.3]) == (0.1 + 0.2) + 0.3


def test_cpu_calculator_gives_none(monkeypatch, tmp_path):
    from src.metrics import MetricsCalculator
    monkeypatch.delenv("FIE_LPIPS_DIR", raising=False)
    monkeypatch.delenv("FIE_WEIGHTS_DIR", raising=False)
    d = lo.write_dir(tmp_path / "w", "safetensors")
    calc = MetricsCalculator("cpu", lpips_dir=d)                                 # the CPU calculator never loads one
    ims = lo.images("small")
    a, b = Image.fromarray(ims["a"]), Image.fromarray(ims["b"])
    assert calc.calculate_lpips(a, b) is None and calc.calculate_lpipses([a, b], [b, a]) == [None, None]
    m = calc.calculate_all_metrics(a, b, "p", mask=np.zeros((45, 67), np.uint8))
    assert m["lpips"] is None and list(m) == ["ssim", "lpips", "clip_score", "psnr", "mse", "dino_distance", "bg_ssim", "bg_psnr", "bg_mse"]
    with pytest.raises(ValueError):
        calc.calculate_lpipses([a], [a, b])


class _StubLpips:
    """Stands in for an LpipsScorer on the CPU calculator: evaluate.py only asks the calculator."""


def test_evaluate_fills_the_columns(tmp_path, monkeypatch):
    import evaluate
    import run_batch
    import run_single_image
    from src.metrics import MetricsCalculator
    monkeypatch.delenv("FIE_LPIPS_DIR", raising=False)
    monkeypatch.delenv("FIE_WEIGHTS_DIR", raising=False)
    flags = lambda p: {s for a in p._actions for s in a.option_strings}
    assert flags(evaluate.add_lpips_args(evaluate.build_parser())) - flags(evaluate.build_parser()) == {"--lpips_dir"}
    assert flags(run_batch.add_lpips_args(run_batch.build_parser())) - flags(run_batch.build_parser()) == {"--lpips_dir"}
    assert "--lpips_dir" in flags(run_single_image.build_parser())
    assert run_batch.METRIC_KEYS[-2:] == ("lpips", "bg_lpips")
    (tmp_path / "src" / "0_x").mkdir(parents=True)
    (tmp_path / "out" / "0_x").mkdir(parents=True)
    ims = lo.images("small")
    for name, arr in (("a.png", ims["a"]), ("b.png", ims["c"])):
        Image.fromarray(arr).save(tmp_path / "src" / "0_x" / name)
        Image.fromarray(arr[::-1].copy()).save(tmp_path / "out" / "0_x" / name)
    rle = [0, 512 * 100, 512 * 50, 512 * 362]                                   # PIE-Bench run lengths: rows 100 .. 149 edited
    json.dump({f"00{i}": {"image_path": f"0_x/{n}", "editing_prompt": "p", "editing_type_id": "0", "mask": rle} for i, n in enumerate(("a.png", "b.png"))},
              open(tmp_path / "map.json", "w"))
    seen = []

    def fake_lpipses(self, sources, editeds, masks=None):
        seen.append((len(sources), None if masks is None else [m is not None for m in masks]))
        return [dict({"lpips": 0.25 + 0.5 * i}, **({"bg_lpips": 0.125} if masks is not None and masks[i] is not None else {})) for i in range(len(sources))]

    real_init = MetricsCalculator.__init__

    def init(self, device="cuda", **kw):
        real_init(self, device, **kw)
        seen.append(kw.get("lpips_dir"))
        self._lpips = _StubLpips()

    monkeypatch.setattr(MetricsCalculator, "__init__", init)
    monkeypatch.setattr(MetricsCalculator, "calculate_lpipses", fake_lpipses)
    base = ["--mapping_file", str(tmp_path / "map.json"), "--source_dir", str(tmp_path / "src"), "--outputs_dir", str(tmp_path / "out"),
            "--summary_file", str(tmp_path / "s.json"), "--device", "cpu", "--lpips_dir", "/some/dir"]
    evaluate.main(base + ["--results_file", str(tmp_path / "m.csv")])
    rows = list(csv.reader(open(tmp_path / "m.csv")))
    assert rows[0] == ["image_id", "image_path", "editing_type_id", "editing_prompt", "ssim", "lpips", "clip_score", "psnr", "mse", "dino_distance"]
    assert [r[5] for r in rows[1:]] == ["0.25", "0.75"]
    assert json.load(open(tmp_path / "s.json"))["overall"]["lpips"]["mean"] == pytest.approx(0.5)
    evaluate.main(base + ["--results_file", str(tmp_path / "m2.csv"), "--use_mask"])
    rows = list(csv.reader(open(tmp_path / "m2.csv")))
    assert rows[0][4:] == ["ssim", "lpips", "clip_score", "psnr", "mse", "dino_distance", "bg_ssim", "bg_psnr", "bg_mse", "bg_lpips"]
    assert [r[5] for r in rows[1:]] == ["0.25", "0.75"] and [r[13] for r in rows[1:]] == ["0.125", "0.125"]
    assert seen == ["/some/dir", (2, None), "/some/dir", (2, [True, True])]


def test_oracle_controls_small():
    """What parity can see, from the oracle alone, at the small case (45 x 67).  With bound(pair) = 4 e s_64(pair), e the oracle's own fp32 error
    against its float64 self over the three pairs -- the bound the GPU tests assert:
      * a-a is exactly 0 and the three scores lie more than 10 bounds apart;
      * floor-mode pooling and a missing scaling layer each move every score by more than 10 bounds."""
    _controls("small", floor=True)


def test_oracle_controls_full():
    """The same at 512 x 512, where no pool window is clipped: floor-mode pooling gives the same bits there, so only the scaling layer is a control."""
    _controls("full", floor=False)
    for p in lo.PAIRS:
        assert lo.layers_of("full", p, "f64", ceil=False) == lo.layers_of("full", p, "f64")
    m = lo.full_mask()
    c = lo.images("full")
    rect = (c["a"] != c["c"]).any(2).astype(np.uint8)
    assert lo.score_of("full", "ac", "f64", mask=rect, key="rect") == 0.0          # masking c's own rectangle leaves nothing: not the mask to test with
    bg = lo.score_of("full", "ac", "f64", mask=m, key="band")
    assert 0 < bg < lo.score_of("full", "ac", "f64") and abs(bg - lo.score_of("full", "ac", "f64")) > 40 * lo.score_error("full") * bg


def _controls(case, floor):
    s64 = {p: lo.score_of(case, p, "f64") for p in lo.PAIRS}
    e = lo.score_error(case)
    bound = {p: 4 * e * s64[p] for p in lo.PAIRS}
    print(f"[lpips control] {case}: s_64 {s64}, own error {e:.3e}, tap errors {[f'{v:.2e}' for v in lo.tap_errors(case)]}")
    assert lo.layers_of(case, "aa", "f64") == [0.0] * 7 and lo.layers_of(case, "aa", "f32") == [0.0] * 7
    assert 0 < e < 1e-5 and all(0 < v < 1e-5 for v in lo.tap_errors(case))
    assert all(v > 0 for p in lo.PAIRS for v in lo.layers_of(case, p, "f64"))                      # no tap is dead
    for p, q in (("ab", "ac"), ("ac", "ad"), ("ab", "ad")):
        assert abs(s64[p] - s64[q]) > 10 * max(bound[p], bound[q])
    variants = [("no scaling layer", dict(scaling=False))] + ([("floor pooling", dict(ceil=False))] if floor else [])
    for what, kw in variants:
        miss = {p: abs(lo.score_of(case, p, "f64", **kw) - s64[p]) / bound[p] for p in lo.PAIRS}
        print(f"[lpips control] {case}: {what} misses by {miss} bounds")
        assert min(miss.values()) > 10
