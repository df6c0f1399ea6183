"""Device-side edit metrics on the MI355X (csrc/metrics.hip through ctx.metrics_pairs, MetricsCalculator("cuda"), FastEditor.edit(metrics=True)).

Yardsticks (tests/metrics_oracle.py): the SSE must equal numpy's integer sum exactly; the SSIM must lie within 4 x d0 of the float64
restatement, d0 = max |fp32 oracle - float64 restatement| over the whole pair set (what the reference definition itself leaves undetermined in
fp32; one factor of two for the second separable pass's rounding, one for summation order).  d0 is computed here, never chosen."""
import numpy as np
import pytest
import torch
from PIL import Image

import metrics_oracle as mo

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def pairs():
    return mo.pair_set()


@pytest.fixture(scope="module")
def tol(pairs):
    d0 = mo.d0(pairs)
    print(f"\n[metrics] d0 = {d0:.3e}, SSIM tolerance 4 x d0 = {4 * d0:.3e}")
    assert d0 > 0
    return 4 * d0


def _dev(fie, arrs):
    return torch.from_numpy(np.stack(arrs)).to(fie.device)


def _score(fie, a_list, b_list, masks=None):
    """-> (int64 [n, 4] rows on the host, [dict])"""
    from fie_amd import metrics as hmetrics
    rows = fie.metrics_pairs(_dev(fie, a_list), _dev(fie, b_list), None if masks is None else _dev(fie, masks)).cpu().numpy()
    h, w = a_list[0].shape[:2]
    return rows, hmetrics.rows_to_dicts(rows, h, w, masks is not None)


def _by_size(pairs):
    out = {}
    for name, a, b in pairs:
        out.setdefault(a.shape[:2], []).append((name, a, b))
    return out


def _masks(h, w):
    from fie_amd import mask as hmask
    half = np.zeros((h, w), np.uint8)
    half[:, w // 2:] = 255
    blob = mo.blob_mask(h, w, h + w)
    rle = hmask.rle_decode(hmask.rle_encode(blob), (h, w))          # PIE-Bench's code: the decoder also sets the 1-pixel border
    return {"half_plane": half, "run_length": rle}


@pytest.mark.parametrize("n", [1, 3, 8])
def test_sse_exact_and_ssim_within_the_oracle_bound(fie, pairs, tol, n):
    """Rules 4 and 5 on every pair of the set, in launches of n pairs (the set's pairs of one size, n at a time, the last launch padded
    by wrapping round), without a mask and with the half-plane and run-length masks."""
    worst = 0.0
    for (h, w), group in _by_size(pairs).items():
        masks = _masks(h, w)
        for start in range(0, len(group), n):
            chunk = [group[(start + i) % len(group)] for i in range(n)]
            a_list, b_list = [c[1] for c in chunk], [c[2] for c in chunk]
            rows0, plain = _score(fie, a_list, b_list)
            for i, ((name, a, b), d) in enumerate(zip(chunk, plain)):
                ref = mo.ssim64(a, b)
                err = abs(d["ssim"] - ref)
                worst = max(worst, err)
                print(f"[metrics] n={n} {name}: ssim {d['ssim']:.9f} ref {ref:.9f} err {err:.2e}")
                assert int(rows0[i, 0]) == mo.sse(a, b) and d["mse"] == mo.sse(a, b) / (65025.0 * a.size), name
                assert err <= tol, (name, d["ssim"], ref, err, tol)
                if mo.sse(a, b) == 0:
                    assert d["psnr"] == float("inf")
            names = list(masks)
            for shift in range(len(names)):                       # pair i of a launch takes mask (i + shift): different masks within one launch
                used = [names[(i + shift) % len(names)] for i in range(n)]
                rows, got = _score(fie, a_list, b_list, [masks[u] for u in used])
                for i, ((name, a, b), d) in enumerate(zip(chunk, got)):
                    mname, m = used[i], masks[used[i]]
                    za, zb = mo.zeroed(a, b, m)
                    ref = mo.ssim64(za, zb)
                    err = abs(d["bg_ssim"] - ref)
                    worst = max(worst, err)
                    print(f"[metrics] n={n} {name} bg({mname}): ssim {d['bg_ssim']:.9f} ref {ref:.9f} err {err:.2e}")
                    assert int(rows[i, 0]) == mo.sse(a, b) and int(rows[i, 2]) == mo.sse(za, zb), (name, mname)
                    assert d["ssim"] == plain[i]["ssim"] and err <= tol, (name, mname, d["bg_ssim"], ref, err, tol)
    print(f"[metrics] n={n}: largest device SSIM error {worst:.3e} (bound {tol:.3e})")


def test_constant_images_one_grey_level_apart(fie):
    """E[xx] - mu^2 cancels on constant images: the fp32 oracle itself is off by 6.5e-5 here and a plain separable fp32 form by more, so this
    pair is outside the bounded set; the value must be finite and in [0, 1], its error is recorded."""
    a, b = np.full((512, 512, 3), 200, np.uint8), np.full((512, 512, 3), 201, np.uint8)
    rows, (d,) = _score(fie, [a], [b])
    ref = mo.ssim64(a, b)
    print(f"[metrics] constant 200 vs 201: device {d['ssim']:.9f} float64 {ref:.9f} err {abs(d['ssim'] - ref):.2e}; fp32 oracle err {abs(mo.ssim32(a, b) - ref):.2e}")
    assert int(rows[0, 0]) == a.size and np.isfinite(d["ssim"]) and 0.0 <= d["ssim"] <= 1.0


def test_determinism_across_calls_and_batch_positions(fie, pairs):
    group = _by_size(pairs)[(512, 512)]
    a_list, b_list = [g[1] for g in group], [g[2] for g in group]
    mask = _masks(512, 512)["run_length"]
    a8 = [a_list[i % len(group)] for i in range(8)]
    b8 = [b_list[(i + 1) % len(group)] for i in range(8)]
    da, db, dm = _dev(fie, a8), _dev(fie, b8), _dev(fie, [mask] * 8)
    r1 = fie.metrics_pairs(da, db, dm).cpu()
    r2 = fie.metrics_pairs(da, db, dm).cpu()
    assert torch.equal(r1, r2)
    alone = fie.metrics_pairs(da[5], db[5], dm[5]).cpu()
    assert alone.shape == (1, 4) and torch.equal(alone[0], r1[5])
    assert torch.equal(fie.metrics_pairs(da[5:6], db[5:6]).cpu()[0, :2], r1[5, :2])


def test_background_limits(fie, pairs, tol):
    from fie_amd import metrics as hmetrics
    name, a, b = _by_size(pairs)[(512, 512)][0]
    zeros, ones = np.zeros((512, 512), np.uint8), np.ones((512, 512), np.uint8)
    rows, _ = _score(fie, [a, a], [b, b], [zeros, ones])
    assert rows[0, 2] == rows[0, 0] and rows[0, 3] == rows[0, 1]            # nothing edited: the background pair IS the pair, bit for bit
    assert rows[1, 0] == rows[0, 0] and rows[1, 1] == rows[0, 1]
    d = hmetrics.rows_to_dicts(rows, 512, 512, True)[1]
    assert int(rows[1, 2]) == 0 and d["bg_psnr"] == float("inf") and abs(d["bg_ssim"] - 1.0) <= tol
    plain, _ = _score(fie, [a], [b])
    assert plain[0, 0] == rows[0, 0] and plain[0, 1] == rows[0, 1] and plain[0, 2] == 0 and plain[0, 3] == 0


def test_argument_checks(fie):
    from fie_amd import hip
    small = torch.zeros((1, 10, 64, 3), device=fie.device, dtype=torch.uint8)
    with pytest.raises(hip.FieError):
        fie.metrics_pairs(small, small)
    a = torch.zeros((1, 16, 16, 3), device=fie.device, dtype=torch.uint8)
    with pytest.raises(ValueError):
        fie.metrics_pairs(a, a.float())
    with pytest.raises(ValueError):
        fie.metrics_pairs(a, a, torch.zeros((1, 16, 15), device=fie.device, dtype=torch.uint8))
    ws = torch.zeros(4, device=fie.device, dtype=torch.int64)
    out = torch.zeros((1, 4), device=fie.device, dtype=torch.int64)
    fie.sync_stream()
    lib = hip.lib()
    assert lib.fie_metrics_pairs_u8(fie.h, a.data_ptr(), a.data_ptr(), None, 1, 16, 16, out.data_ptr(), ws.data_ptr(), 8) != 0       # short workspace
    assert lib.fie_metrics_pairs_u8(fie.h, a.data_ptr(), None, None, 1, 16, 16, out.data_ptr(), ws.data_ptr(), 32) != 0
    assert lib.fie_metrics_pairs_u8(fie.h, a.data_ptr(), a.data_ptr(), None, 1, 16, 16, out.data_ptr(), ws.data_ptr(), 32) == 0
    torch.cuda.synchronize()
    assert out.cpu()[0, 0] == 0


@pytest.mark.parametrize("size", [(512, 512), (1024, 768)])
def test_calculator_cuda_against_cpu(fie, tol, size):
    from src.metrics import MetricsCalculator
    w, h = size
    a = mo.textured(21, h, w)
    _, a, b = mo.variants(a, 3)[0]
    ia, ib = Image.fromarray(a), Image.fromarray(b)
    mask = mo.blob_mask(h, w, 4)
    gpu, cpu = MetricsCalculator("cuda"), MetricsCalculator("cpu")
    g, c = gpu.calculate_all_metrics(ia, ib, "p", mask=mask), cpu.calculate_all_metrics(ia, ib, "p", mask=mask)
    assert list(g) == list(c)
    ra, rb = np.asarray(ia.resize((512, 512), Image.LANCZOS)), np.asarray(ib.resize((512, 512), Image.LANCZOS))
    assert g["mse"] == mo.sse(ra, rb) / (65025.0 * ra.size)                 # the device LANCZOS is Pillow's, the SSE exact
    # the issue asks "MSE equal to float64 rounding" between the two calculators; the pinned CPU path averages in fp32 (a relative 1e-6 of fp32
    # rounding and summation), so float64 equality is asserted against numpy's integer SSE above and the CPU comparison is at fp32 precision
    for k in ("mse", "bg_mse"):
        assert abs(g[k] - c[k]) <= 1e-6 * c[k] + 1e-12, (k, g[k], c[k])
    for k in ("psnr", "bg_psnr"):
        assert abs(g[k] - c[k]) <= 1e-4, (k, g[k], c[k])
    for k in ("ssim", "bg_ssim"):
        print(f"[metrics] calculator {size} {k}: cuda {g[k]:.9f} cpu {c[k]:.9f}")
        assert abs(g[k] - c[k]) <= tol, (k, g[k], c[k])
    assert g["lpips"] is None and g["clip_score"] is None and g["dino_distance"] is None
    assert gpu.calculate_ssim(ia, ib) == g["ssim"] and gpu.calculate_mse(ia, ib) == g["mse"] and gpu.calculate_psnr(ia, ib) == g["psnr"]
    many = gpu.calculate_pairs([ia, ib, ia], [ib, ia, ia], [None, mask, None])
    assert many[0] == {k: g[k] for k in ("ssim", "psnr", "mse")} and many[1]["bg_mse"] == g["bg_mse"] and many[2]["psnr"] == float("inf")


@pytest.fixture(scope="module")
def editor(fie):
    from src.pipeline import FastEditor
    return FastEditor(model_name="tiny", enable_cpu_offload=False)


def _close(m, want, tol, keys):
    for k in keys:
        if k.endswith("mse"):
            assert abs(m[k] - want[k]) <= 1e-6 * want[k] + 1e-12, (k, m[k], want[k])
        elif k.endswith("psnr"):
            assert abs(m[k] - want[k]) <= 1e-4, (k, m[k], want[k])
        else:
            assert abs(m[k] - want[k]) <= tol, (k, m[k], want[k])


def test_edit_with_inline_metrics(editor, tol):
    from src.metrics import MetricsCalculator
    img = Image.fromarray(mo.textured(31, 384, 640))
    prompt = "a [red] kite"
    plain = editor.edit(img, prompt, seed=42)
    image, m = editor.edit(img, prompt, seed=42, metrics=True)
    assert isinstance(plain, Image.Image) and np.array_equal(np.asarray(image), np.asarray(plain))
    assert set(m) == {"ssim", "psnr", "mse"}
    ra, rb = np.asarray(img.resize((512, 512), Image.LANCZOS)), np.asarray(image.resize((512, 512), Image.LANCZOS))
    assert m["mse"] == mo.sse(ra, rb) / (65025.0 * ra.size)
    _close(m, MetricsCalculator("cpu").calculate_all_metrics(img, image, prompt), tol, ("ssim", "psnr", "mse"))
    again = editor.edit(img, prompt, seed=42, metrics=True)[1]
    assert again == m


def test_masked_edit_with_inline_background_metrics(editor, fie, tol):
    from src.metrics import MetricsCalculator
    src = mo.textured(33, 1024, 1024)
    img = Image.fromarray(src)
    mask = np.zeros((1024, 1024), np.uint8)
    mask[200:700, 300:900] = 255
    kw = dict(seed=42, mask=mask, paste_back=True, mask_blur=0)
    image, m = editor.edit(img, "a [green] door", metrics=True, **kw)
    assert np.array_equal(np.asarray(image), np.asarray(editor.edit(img, "a [green] door", **kw)))
    assert set(m) == {"ssim", "psnr", "mse", "bg_ssim", "bg_psnr", "bg_mse"}
    want = MetricsCalculator("cpu").calculate_all_metrics(img, image, "a [green] door", mask=mask)
    _close(m, want, tol, ("ssim", "psnr", "mse", "bg_ssim", "bg_psnr", "bg_mse"))
    assert m["bg_mse"] < m["mse"]
    # the exact case: at the edit size (no resize) the background of a pasted-back edit is the source, byte for byte
    out = np.asarray(image)
    rows = fie.metrics_pairs(torch.from_numpy(src).to(fie.device), torch.from_numpy(out.copy()).to(fie.device),
                             torch.from_numpy((mask >= 128).astype(np.uint8)).to(fie.device)).cpu().numpy()
    assert int(rows[0, 2]) == 0 and int(rows[0, 0]) == mo.sse(src, out) and int(rows[0, 0]) > 0


def test_edit_batch_with_inline_metrics(editor, tol):
    from src.metrics import MetricsCalculator
    imgs = [Image.fromarray(mo.textured(40 + i, 256, 256)) for i in range(3)]
    prompts = [f"a [toy] number {i}" for i in range(3)]
    mask = np.zeros((256, 256), np.uint8)
    mask[64:192, 32:160] = 255
    masks = [mask, None, Image.fromarray(mask.T.copy())]
    outs, ms = editor.edit_batch(imgs, prompts, seed=7, strength=0.5, masks=masks, metrics=True)
    assert len(outs) == len(ms) == 3 and isinstance(editor.edit_batch(imgs, prompts, seed=7, strength=0.5, masks=masks), list)
    cpu = MetricsCalculator("cpu")
    for im, out, p, mk, m in zip(imgs, outs, prompts, masks, ms):
        want = cpu.calculate_all_metrics(im, out, p, mask=mk)
        keys = ("ssim", "psnr", "mse") + (("bg_ssim", "bg_psnr", "bg_mse") if mk is not None else ())
        assert set(m) == set(keys)
        _close(m, want, tol, keys)
    outs2, ms2 = editor.edit_batch(imgs, prompts, seed=7, strength=0.5, metrics=True)
    assert all(set(m) == {"ssim", "psnr", "mse"} for m in ms2)


def test_run_batch_metrics_rows(editor, tmp_path):
    import json
    import run_batch
    from tools import make_synthetic_piebench as msp
    data = tmp_path / "pie"
    msp.main(["--out", str(data), "--num", "2", "--with_masks"])
    mapping = json.load(open(data / "mapping_file.json"))
    entries = [(i, k, e) for i, (k, e) in enumerate(mapping.items())]
    out = tmp_path / "out"
    parser = run_batch.add_metrics_args(run_batch.add_mask_args(run_batch.build_parser()))
    args = parser.parse_args(["--source_dir", str(data / "annotation_images"), "--output_dir", str(out), "--seed", "42", "--strength", "0.5",
                              "--use_mask", "--metrics"])
    r = run_batch.process_shard(editor, entries, args, str(out / "e"), str(out / "c"))
    assert r["processed"] == 2 and r["failed"] == 0
    for row in r["rows"]:
        assert {"ssim", "psnr", "mse", "bg_ssim", "bg_psnr", "bg_mse"} <= set(row) and 0 < row["ssim"] <= 1 and row["bg_mse"] < row["mse"]
    json.dumps(r)
