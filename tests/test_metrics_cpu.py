"""Device-side edit metrics, host half (no GPU): the C ABI carries the op, fie_amd/metrics.py decodes result rows and prepares masks,
MetricsCalculator("cpu") gains the background keys, evaluate.py --use_mask writes the extra columns."""
import json
import math
import os
import re

import numpy as np
import pytest
from PIL import Image

import fie_amd  # noqa: F401
from fie_amd import hip
from fie_amd import mask as hmask
from fie_amd import metrics as hmetrics

import metrics_oracle as mo

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("fie_metrics_workspace_bytes", "fie_metrics_pairs_u8")


def test_metrics_entries_in_header_signatures_and_library():
    hip.build()
    text = open(os.path.join(ROOT, "include", "fie.h")).read()
    declared = set(re.findall(r"\b(fie_[a-z0-9_]+)\s*\(", text))
    lib = hip.lib()
    for name in NEW:
        assert name in declared, f"{name} missing from include/fie.h"
        assert name in hip.SIGNATURES, f"{name} missing from hip.SIGNATURES"
        assert hasattr(lib, name), f"{name} not exported by libfie_hip.so"
    # the workspace query is host code: one 16-byte partial per 32x32 tile, pair and variant; sizes below the window are refused
    assert lib.fie_metrics_workspace_bytes(1, 512, 512) == 2 * 256 * 16
    assert lib.fie_metrics_workspace_bytes(8, 203, 517) == 8 * 2 * 7 * 17 * 16
    assert lib.fie_metrics_workspace_bytes(1, 11, 11) == 32
    assert lib.fie_metrics_workspace_bytes(1, 10, 512) == -1 and lib.fie_metrics_workspace_bytes(0, 512, 512) == -1


def _row(sse, ssim_sum, bg_sse=0, bg_ssim_sum=0.0):
    r = np.zeros(4, np.int64)
    r[0], r[2] = sse, bg_sse
    r.view(np.float64)[1], r.view(np.float64)[3] = ssim_sum, bg_ssim_sum
    return r


def test_result_row_to_dict():
    h = w = 512
    n_ssim = 3 * 502 * 502
    d, = hmetrics.rows_to_dicts(_row(123456789, 0.75 * n_ssim, 1000, 0.5 * n_ssim), h, w)
    assert set(d) == {"ssim", "psnr", "mse"}
    mse = 123456789 / (255.0 ** 2 * 3 * h * w)
    assert d["mse"] == mse and d["psnr"] == 10.0 * math.log10(1.0 / mse) and d["ssim"] == 0.75
    d, = hmetrics.rows_to_dicts(_row(123456789, 0.75 * n_ssim, 1000, 0.5 * n_ssim), h, w, bg=True)
    assert set(d) == {"ssim", "psnr", "mse", "bg_ssim", "bg_psnr", "bg_mse"}
    assert d["bg_mse"] == 1000 / (255.0 ** 2 * 3 * h * w) and d["bg_ssim"] == 0.5
    d, = hmetrics.rows_to_dicts(_row(0, float(n_ssim)), h, w)
    assert d["mse"] == 0.0 and d["psnr"] == float("inf") and d["ssim"] == 1.0
    # the largest SSE a 512x512 pair can have survives the trip exactly; per-pair bg flags
    big = 786432 * 65025
    two = hmetrics.rows_to_dicts(np.stack([_row(big, 0.0), _row(1, 0.0, 1, 0.0)]), h, w, bg=[False, True])
    assert two[0]["mse"] == 1.0 and two[0]["psnr"] == 0.0 and "bg_mse" not in two[0] and "bg_mse" in two[1]
    # 11x11: one window position per channel
    assert hmetrics.rows_to_dicts(_row(0, 3.0), 11, 11)[0]["ssim"] == 1.0


def test_row_formulas_agree_with_the_oracle():
    """From the exact SSE and the float64 SSIM sum of a pair, the decoded metrics are the oracle's."""
    from oracle import metrics as ometrics
    a, b = mo.textured(3, 64, 80), None
    _, a, b = mo.variants(a, 1)[0]
    d, = hmetrics.rows_to_dicts(_row(mo.sse(a, b), mo.ssim64(a, b) * 3 * 54 * 70), 64, 80)
    ia, ib = Image.fromarray(a), Image.fromarray(b)
    assert abs(d["mse"] - ometrics.mse(ia, ib, size=None)) < 1e-8
    assert abs(d["psnr"] - ometrics.psnr(ia, ib, size=None)) < 1e-5
    assert abs(d["ssim"] - mo.ssim64(a, b)) < 1e-12           # the divisor is the cropped map's size (the fp32 oracle's own error is d0's business)


def test_binary_mask_preparation():
    assert hmetrics.TARGET == (512, 512)
    m = np.zeros((512, 512), np.uint8)
    m[100:200, 50:300] = 255
    m[0, 0] = 127
    m[0, 1] = 128
    b = hmetrics.binary_mask(m)
    assert b.dtype == np.uint8 and b.shape == (512, 512) and set(np.unique(b)) == {0, 1}
    assert b[150, 100] == 1 and b[0, 0] == 0 and b[0, 1] == 1 and int(b.sum()) == 100 * 250 + 1
    assert np.array_equal(hmetrics.binary_mask(m > 127), hmetrics.binary_mask(Image.fromarray(np.where(m > 127, 255, 0).astype(np.uint8))))
    # another size: mode L, LANCZOS to 512x512, then >= 128
    big = np.zeros((768, 1024), np.uint8)
    big[:, 512:] = 255
    want = (np.asarray(Image.fromarray(big, "L").resize((512, 512), Image.LANCZOS)) >= 128).astype(np.uint8)
    assert np.array_equal(hmetrics.binary_mask(big), want) and want[:, 300:].all() and not want[:, :200].any()
    with pytest.raises(ValueError):
        hmetrics.binary_mask(big, size=(512, 512))
    # a PIE-Bench run-length mask is 512x512 already
    blob = mo.blob_mask(512, 512, 5)
    dec = hmask.rle_decode(hmask.rle_encode(blob))
    assert np.array_equal(hmetrics.binary_mask(dec), (dec > 0).astype(np.uint8))


def test_cpu_calculator_background_keys():
    from src.metrics import MetricsCalculator
    from oracle import metrics as ometrics
    a = mo.textured(5)
    _, a, b = mo.variants(a, 2)[0]
    mask = mo.blob_mask(512, 512, 9)
    mc = MetricsCalculator(device="cpu")
    ia, ib = Image.fromarray(a), Image.fromarray(b)
    plain = mc.calculate_all_metrics(ia, ib, "x")
    assert list(plain) == ["ssim", "lpips", "clip_score", "psnr", "mse", "dino_distance"]
    assert plain["ssim"] == mc.calculate_ssim(ia, ib) and plain["mse"] == mc.calculate_mse(ia, ib) and plain["psnr"] == mc.calculate_psnr(ia, ib)
    m = mc.calculate_all_metrics(ia, ib, "x", mask=mask)
    assert list(m) == list(plain) + ["bg_ssim", "bg_psnr", "bg_mse"] and all(m[k] == plain[k] for k in plain)
    za, zb = mo.zeroed(a, b, mask)
    assert abs(m["bg_ssim"] - ometrics.ssim(Image.fromarray(za), Image.fromarray(zb))) < 1e-6
    assert abs(m["bg_mse"] - mo.sse(za, zb) / (65025.0 * a.size)) < 1e-9 and m["bg_mse"] < m["mse"]
    rows = mc.calculate_pairs([ia, ia], [ib, ia], [None, mask])
    assert set(rows[0]) == {"ssim", "psnr", "mse"} and rows[0]["ssim"] == plain["ssim"]
    assert rows[1]["psnr"] == float("inf") and rows[1]["bg_mse"] == 0.0 and abs(rows[1]["bg_ssim"] - 1.0) < 1e-6
    with pytest.raises(ValueError):
        mc.calculate_pairs([ia], [ib, ib])


def _tree(tmp_path, with_masks):
    mapping = {}
    for i in range(4):
        rel = f"{i % 2}_cat/{i:012d}.png"
        a = mo.textured(i, 96, 128)
        for root, img in (("src", a), ("out", mo.variants(a, i)[0][2])):
            p = tmp_path / root / rel
            p.parent.mkdir(parents=True, exist_ok=True)
            Image.fromarray(img).save(p)
        mapping[f"{i:012d}"] = {"image_path": rel, "editing_prompt": f"a [thing] {i}", "editing_type_id": str(i % 2)}
        if with_masks:
            mapping[f"{i:012d}"]["mask"] = hmask.rle_encode(mo.blob_mask(512, 512, i))
    (tmp_path / "map.json").write_text(json.dumps(mapping))
    return ["--mapping_file", str(tmp_path / "map.json"), "--source_dir", str(tmp_path / "src"), "--outputs_dir", str(tmp_path / "out"),
            "--results_file", str(tmp_path / "r" / "metrics.csv"), "--summary_file", str(tmp_path / "r" / "summary.json"), "--device", "cpu"]


def test_evaluate_use_mask_columns(tmp_path):
    import csv
    import evaluate
    from src.metrics import MetricsCalculator
    base = "image_id,image_path,editing_type_id,editing_prompt,ssim,lpips,clip_score,psnr,mse,dino_distance"
    argv = _tree(tmp_path, True)
    evaluate.main(argv)
    assert (tmp_path / "r" / "metrics.csv").read_text().splitlines()[0] == base
    s = json.loads((tmp_path / "r" / "summary.json").read_text())
    assert set(s["overall"]) == {"ssim", "lpips", "clip_score", "psnr", "mse", "dino_distance"} and s["total_images"] == 4
    plain_rows = list(csv.DictReader(open(tmp_path / "r" / "metrics.csv")))
    evaluate.main(argv + ["--use_mask"])
    assert (tmp_path / "r" / "metrics.csv").read_text().splitlines()[0] == base + ",bg_ssim,bg_psnr,bg_mse"
    rows = list(csv.DictReader(open(tmp_path / "r" / "metrics.csv")))
    assert len(rows) == 4 and all(float(r["bg_mse"]) < float(r["mse"]) and 0 < float(r["bg_ssim"]) <= 1 for r in rows)
    assert [(r["ssim"], r["psnr"], r["mse"]) for r in rows] == [(r["ssim"], r["psnr"], r["mse"]) for r in plain_rows]
    s = json.loads((tmp_path / "r" / "summary.json").read_text())
    assert set(s["overall"]) == {"ssim", "lpips", "clip_score", "psnr", "mse", "dino_distance", "bg_ssim", "bg_psnr", "bg_mse"}
    assert set(s["overall"]["bg_ssim"]) == {"mean", "std", "median"} and set(s["by_category"]["0"]["bg_psnr"]) == {"mean", "std"}
    # the row of item 0 is the calculator's on that pair and its decoded mask (the decoder sets the 1-pixel border)
    rel = rows[0]["image_path"]
    want = MetricsCalculator("cpu").calculate_all_metrics(Image.open(tmp_path / "src" / rel).convert("RGB"), Image.open(tmp_path / "out" / rel).convert("RGB"),
                                                          "", mask=hmask.rle_decode(hmask.rle_encode(mo.blob_mask(512, 512, 0))))
    assert float(rows[0]["bg_ssim"]) == want["bg_ssim"] and float(rows[0]["mse"]) == want["mse"]


def test_evaluate_use_mask_needs_masks(tmp_path, capsys):
    import evaluate
    evaluate.main(_tree(tmp_path, False) + ["--use_mask"])
    assert "has no `mask`" in capsys.readouterr().out and not (tmp_path / "r" / "metrics.csv").exists()


def test_cli_flags_are_additive():
    import evaluate
    import run_batch
    flags = lambda p: {a.option_strings[0] for a in p._actions if a.option_strings}
    assert flags(evaluate.add_mask_args(evaluate.build_parser())) - flags(evaluate.build_parser()) == {"--use_mask"}
    assert flags(run_batch.add_metrics_args(run_batch.build_parser())) - flags(run_batch.build_parser()) == {"--metrics"}
    (act,) = [a for a in run_batch.add_metrics_args(run_batch.build_parser())._actions if a.option_strings == ["--metrics"]]
    assert "BEFORE JPEG" in act.help


def test_d0_of_the_pair_set_is_what_the_gpu_bound_rests_on():
    """The SSIM tolerance of tests/test_metrics_gpu.py is 4 x d0, d0 = max |fp32 oracle - float64 restatement| over the whole pair set.  It is a
    property of the reference arithmetic alone and is computed, not chosen; this test only shows it is a sane yardstick (non-zero, far below
    the differences between the metrics of any two of the pairs)."""
    d0 = mo.d0(mo.pair_set())
    print(f"d0 = {d0:.3e}")
    assert 1e-7 < d0 < 1e-4
