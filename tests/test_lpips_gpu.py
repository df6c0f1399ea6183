"""LPIPS on the MI355X (csrc/lpips.hip, FIE_ACT_RELU in csrc/f32.hip, fie_amd/lpips.py, MetricsCalculator, FastEditor) against the CPU oracle of
tests/lpips_oracle.py (SqueezeNet 1.1's features and the LPIPS head in plain torch, as DESIGN.md section 19 defines the number).

Every bound comes from the oracle alone and is computed at run time: 4 x the oracle's own fp32 error against its float64 self (the factor allows
for another summation order and tile shape; the margin of DESIGN.md section 10).  For a score the own error is the worst over the case's three
pairs.  DESIGN.md section 19 records the device errors measured beside them."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F
from PIL import Image

import dino_oracle as do
import lpips_oracle as lo
from isolation import guarded

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctxs(fie):
    from fie_amd import hip
    return {"f16": fie, "f32": hip.context(0, torch.float32)}


@pytest.fixture(scope="module")
def wdir(tmp_path_factory):
    return lo.write_dir(tmp_path_factory.mktemp("lpips_st"), "safetensors")


@pytest.fixture(scope="module")
def scorers(ctxs, wdir, tmp_path_factory):
    from fie_amd import lpips as hlpips
    # the fp32 context's scorer from the other directory form: the two must agree bit for bit anyway
    return {"f16": hlpips.load(wdir, ctxs["f16"]), "f32": hlpips.load(lo.write_dir(tmp_path_factory.mktemp("lpips_pth"), "pth"), ctxs["f32"])}


def _dev(ctx, arr):
    return torch.from_numpy(np.ascontiguousarray(arr)).to(ctx.device)


def _bits(t):
    return t.contiguous().view(torch.int32 if t.element_size() == 4 else torch.int64)


# ---------------------------------------------------------------------------------------------------------------------- ops
@pytest.mark.parametrize("shape", [(2, 22, 33, 64), (1, 5, 8, 256), (1, 2, 4, 384)])
def test_maxpool_bit_equal_to_torch(fie, shape):
    """Even and odd edges, clipped and unclipped last windows, an input smaller than the window; negative values, so a window that started from 0
    instead of -inf would show."""
    g = torch.Generator().manual_seed(sum(shape))
    x = torch.randn(shape, generator=g) - 1.5
    want = F.max_pool2d(x.permute(0, 3, 1, 2), 3, 2, ceil_mode=True).permute(0, 2, 3, 1).contiguous()
    assert bool((want < 0).any())
    out, guard = guarded(tuple(want.shape), dtype=torch.float32, device=fie.device, flat=True)
    got = fie.maxpool3s2(x.to(fie.device), out=out)
    torch.cuda.synchronize()
    guard.check("maxpool3s2")
    assert got.shape == want.shape and torch.equal(_bits(got.cpu()), _bits(want))
    assert torch.equal(_bits(fie.maxpool3s2(x.to(fie.device)).cpu()), _bits(want))
    with pytest.raises(ValueError):
        fie.maxpool3s2(x[..., :6].contiguous().to(fie.device))


def test_relu_epilogue_in_the_fp32_entries(ctxs):
    """FIE_ACT_RELU in fie_gemm_f32 / fie_conv3x3_nhwc_f32 is max(., 0) of the FIE_ACT_NONE result, from a context of either dtype; the f16 entry
    still refuses the code."""
    from fie_amd import hip
    g = torch.Generator().manual_seed(3)
    for ctx in ctxs.values():
        dev = ctx.device
        a, w, b = torch.randn(150, 70, generator=g).to(dev), torch.randn(90, 70, generator=g).to(dev), torch.randn(90, generator=g).to(dev)
        none = ctx.gemm_f32(a, w, 90, bias=b)
        relu = ctx.gemm_f32(a, w, 90, bias=b, act=hip.ACT_RELU)
        assert none.dtype == torch.float32 and bool((none < 0).any()) and torch.equal(relu, none.clamp_min(0))
        ref = (a.double() @ w.double().T + b.double()).cpu()
        assert do.rel_err(none.cpu(), ref) < 1e-5
        x, wc, bc = torch.randn(2, 9, 11, 16, generator=g).to(dev), torch.randn(24, 144, generator=g).to(dev), torch.randn(24, generator=g).to(dev)
        wide = [torch.zeros(2, 9, 11, 40, device=dev) for _ in range(2)]
        ctx.conv3x3_f32(x, wc, 24, wide[0][..., 16:], bias=bc)
        ctx.conv3x3_f32(x, wc, 24, wide[1][..., 16:], bias=bc, act=hip.ACT_RELU)
        assert bool((wide[0] < 0).any()) and torch.equal(wide[1], wide[0].clamp_min(0)) and not bool(wide[1][..., :16].any())
        refc = F.conv2d(x.permute(0, 3, 1, 2).double().cpu(), wc.view(24, 3, 3, 16).permute(0, 3, 1, 2).double().cpu(), bc.double().cpu(), padding=1)
        assert do.rel_err(wide[0][..., 16:].permute(0, 3, 1, 2).cpu(), refc) < 1e-5
    f16 = ctxs["f16"]
    a16 = torch.randn(128, 64, generator=g).half().to(f16.device)
    wp = f16.pack_linear(torch.randn(128, 64, generator=g).half())
    with pytest.raises(hip.FieError, match="act"):
        f16.gemm(a16, wp, 128, act=hip.ACT_RELU)
    assert f16.gemm(a16, wp, 128).shape == (128, 128)


@pytest.mark.parametrize("masked", [False, True])
def test_stem_against_torch(fie, masked):
    """Small case, n = 3: every output within 4 d0 of relu(F.conv2d) in float64 on the scaled image, d0 = the same in fp32 against float64."""
    from fie_amd import lpips as hlpips
    ims = lo.images("small")
    arrs = [ims[n] for n in ("a", "c", "d")]
    g = np.random.default_rng(5)
    masks = [(g.random((45, 67)) < 0.3).astype(np.uint8) * v for v in (1, 255, 7)] if masked else [None] * 3
    sd = lo.weights()

    def ref(dtype):
        z = torch.cat([lo.scaled(a, dtype, m) for a, m in zip(arrs, masks)])
        return F.relu(F.conv2d(z, sd["features.0.weight"].to(dtype), sd["features.0.bias"].to(dtype), stride=2)).permute(0, 2, 3, 1)
    r64 = ref(torch.float64)
    d0 = (ref(torch.float32).double() - r64).abs().max().item()
    w = sd["features.0.weight"].permute(2, 3, 1, 0).reshape(27, 64).contiguous().to(fie.device)
    out, guard = guarded((3, 22, 33, 64), dtype=torch.float32, device=fie.device, flat=True)
    got = fie.lpips_stem(_dev(fie, np.stack(arrs)), hlpips.input_lut().to(fie.device), w, sd["features.0.bias"].to(fie.device),
                         mask=_dev(fie, np.stack(masks)) if masked else None, out=out)
    torch.cuda.synchronize()
    guard.check("lpips_stem")
    err = (got.cpu().double() - r64).abs().max().item()
    print(f"[lpips] stem masked={masked}: device error {err:.3e} against float64, d0 {d0:.3e} (bound 4 d0 = {4 * d0:.3e})")
    assert got.shape == r64.shape and err <= 4 * d0
    assert 0.3 < (got > 0).float().mean().item() < 0.7
    if masked:                                                           # the control: the mask matters at this bound
        assert (fie.lpips_stem(_dev(fie, np.stack(arrs)), hlpips.input_lut().to(fie.device), w, sd["features.0.bias"].to(fie.device)).cpu().double()
                - r64).abs().max().item() > 40 * d0


@pytest.mark.parametrize("hw", [8, 176, 3969])
@pytest.mark.parametrize("c", [64, 384, 512])
def test_layer_op(fie, c, hw):
    """One tap on given features against float64 torch.  Bound: 4 x the fp32 torch restatement's error, relative, the worst over the three pairs.
    Then the four properties: equal bits from two runs, from P = 1 and from another position; an identical pair exactly 0; all-zero pixels 0."""
    g = torch.Generator().manual_seed(c * 10000 + hw)
    base = torch.relu(torch.randn(hw, c, generator=g))
    mk = lambda s: torch.relu(base + s * torch.randn(hw, c, generator=g))
    fa = torch.stack([base, mk(0.2), 5.0 * mk(1.0)])
    fb = torch.stack([mk(0.05), mk(0.5), mk(2.0)])
    fa[1, 3] = 0                                                         # a zero pixel on one side
    fa[2, hw - 1] = 0
    fb[2, hw - 1] = 0                                                    # ... and on both
    w = torch.rand(c, generator=g) * 2.0 / c
    ref = lambda dt: [lo.layer_value(fa[i].T.reshape(c, hw, 1).to(dt), fb[i].T.reshape(c, hw, 1).to(dt), w).item() for i in range(3)]
    want, r32 = ref(torch.float64), ref(torch.float32)
    e = max(abs(a - b) / b for a, b in zip(r32, want))
    da, db, dw = fa.to(fie.device), fb.to(fie.device), w.to(fie.device)
    got = fie.lpips_layer(da, db, dw).cpu()
    assert got.dtype == torch.float64 and got.shape == (3,) and bool(torch.isfinite(got).all())
    for i in range(3):
        print(f"[lpips] layer C={c} HW={hw} pair {i}: device {got[i].item():.9e} float64 {want[i]:.9e} error {abs(got[i].item() - want[i]) / want[i]:.3e} "
              f"(own error {e:.3e}, bound {4 * e:.3e})")
    assert all(abs(got[i].item() - want[i]) <= 4 * e * want[i] for i in range(3))
    assert torch.equal(_bits(fie.lpips_layer(da, db, dw).cpu()), _bits(got))
    col = torch.full((3, 7), -1.0, device=fie.device, dtype=torch.float64)
    fie.lpips_layer(da, db, dw, out=col[:, 4])                           # a column of a wider result: ld_out = 7
    assert torch.equal(_bits(col[:, 4].cpu()), _bits(got)) and bool((col[:, :4] == -1).all()) and bool((col[:, 5:] == -1).all())
    for i in range(3):
        one = fie.lpips_layer(da[i:i + 1], db[i:i + 1], dw).cpu()
        order = [(i + 1) % 3, (i + 2) % 3, i]
        moved = fie.lpips_layer(da[order].contiguous(), db[order].contiguous(), dw).cpu()
        assert torch.equal(_bits(one[0:1]), _bits(got[i:i + 1])) and torch.equal(_bits(moved[2:3]), _bits(got[i:i + 1]))
    assert fie.lpips_layer(da, da.clone(), dw).cpu().tolist() == [0.0, 0.0, 0.0]
    zero = torch.zeros(1, hw, c, device=fie.device)
    assert fie.lpips_layer(zero, zero.clone(), dw).cpu().tolist() == [0.0]
    with pytest.raises(ValueError):
        fie.lpips_layer(da[..., :48].contiguous(), db[..., :48].contiguous(), dw[:48].contiguous())


# ---------------------------------------------------------------------------------------------------------------------- scorer
def test_scorer_small_case(scorers):
    """45 x 67: every pool clips a window on one axis and not on the other.  Each tap (relative max-abs error) and each score within 4 x the oracle's
    own error; a-a exactly 0; the fp16 and the fp32 context give the same bits (there is one fp32 path)."""
    ims = lo.images("small")
    sc = scorers["f16"]
    dev = {n: _dev(sc.ctx, v) for n, v in ims.items()}
    own = lo.tap_errors("small")
    for k, f in enumerate(sc.taps(torch.stack([dev[n] for n in do.NAMES]))):
        f = f.cpu().permute(0, 3, 1, 2)
        errs = [do.rel_err(f[i:i + 1], lo.taps_of("small", n, "f64")[k]) for i, n in enumerate(do.NAMES)]
        print(f"[lpips] small tap {k} {tuple(f.shape)}: relative max-abs error {max(errs):.3e} (oracle's own {own[k]:.3e}, bound {4 * own[k]:.3e})")
        assert tuple(f.shape[1:]) == (lo.CHANNELS[k],) + tuple(lo.taps_of("small", "a", "f64")[k].shape[2:]) and max(errs) <= 4 * own[k]
    rows = {p: s.scores([dev["a"]] * 4, [dev["b"], dev["c"], dev["d"], dev["a"]]).cpu() for p, s in scorers.items()}
    assert rows["f16"].shape == (4, 7) and rows["f16"].dtype == torch.float64 and torch.equal(_bits(rows["f16"]), _bits(rows["f32"]))
    from fie_amd import lpips as hlpips
    e = lo.score_error("small")
    for p, row in zip(lo.PAIRS, rows["f16"]):
        got, want = hlpips.total(row.tolist()), lo.score_of("small", p, "f64")
        print(f"[lpips] small score {p}: device {got:.9e} float64 {want:.9e} error {abs(got - want) / want:.3e} (own error {e:.3e}, bound {4 * e:.3e})")
        assert abs(got - want) <= 4 * e * want
    assert rows["f16"][3].tolist() == [0.0] * 7
    with pytest.raises(ValueError, match="32 x 32"):
        sc.scores([dev["a"][:31]], [dev["b"][:31]])


def test_scorer_full_case(scorers):
    """512 x 512: score and background score (a band that is not image c's rectangle) of the three pairs in one call."""
    from fie_amd import lpips as hlpips
    sc = scorers["f16"]
    dev = {n: _dev(sc.ctx, v) for n, v in lo.images("full").items()}
    band = lo.full_mask()
    mk = _dev(sc.ctx, band)
    rows = sc.scores([dev["a"]] * 3, [dev["b"], dev["c"], dev["d"]], [mk, mk, mk]).cpu()
    assert rows.shape == (3, 14) and bool(torch.isfinite(rows).all())
    for what, cols, kw in (("score", slice(0, 7), {}), ("bg score", slice(7, 14), dict(mask=band, key="band"))):
        e = max(abs(lo.score_of("full", p, "f32", **kw) - lo.score_of("full", p, "f64", **kw)) / lo.score_of("full", p, "f64", **kw) for p in lo.PAIRS)
        for p, row in zip(lo.PAIRS, rows):
            got, want = hlpips.total(row[cols].tolist()), lo.score_of("full", p, "f64", **kw)
            print(f"[lpips] full {what} {p}: device {got:.9e} float64 {want:.9e} error {abs(got - want) / want:.3e} (own error {e:.3e}, bound {4 * e:.3e})")
            assert abs(got - want) <= 4 * e * want
    part = sc.scores([dev["a"]] * 2, [dev["c"], dev["d"]], [None, mk]).cpu()       # a mask for one pair only: NaN where none was given
    assert torch.equal(_bits(part[:, :7]), _bits(rows[1:, :7])) and torch.equal(_bits(part[1, 7:]), _bits(rows[2, 7:])) and bool(torch.isnan(part[0, 7:]).all())


# ---------------------------------------------------------------------------------------------------------------------- calculator
def test_calculator_batching_and_resize(fie, wdir, monkeypatch):
    """calculate_lpipses over a list (more pairs than one pass of the tower holds) equals one call each, bit for bit; a 300 x 200 input equals
    the oracle on Pillow's LANCZOS resize."""
    from src.metrics import MetricsCalculator
    monkeypatch.delenv("FIE_LPIPS_DIR", raising=False)
    monkeypatch.delenv("FIE_WEIGHTS_DIR", raising=False)
    calc = MetricsCalculator("cuda", lpips_dir=wdir)
    pil = {n: Image.fromarray(v) for n, v in lo.images("full").items()}
    band = lo.full_mask()
    small = {n: Image.fromarray(np.ascontiguousarray(do.images(300)[n][:200])) for n in ("a", "d")}
    assert small["a"].size == (300, 200)
    srcs = [pil["a"], pil["a"], pil["a"], small["a"], pil["b"], pil["c"], pil["d"], pil["d"], pil["b"], pil["a"]]
    edts = [pil["b"], pil["c"], pil["d"], small["d"], pil["c"], pil["d"], pil["a"], pil["b"], pil["a"], pil["a"]]
    masks = [None, band, None, None, Image.fromarray(band), None, None, band, None, band]
    many = calc.calculate_lpipses(srcs, edts, masks)
    single = [calc.calculate_lpipses([s], [e], [m])[0] for s, e, m in zip(srcs, edts, masks)]
    assert many == single and [set(m) for m in many] == [{"lpips", "bg_lpips"} if m is not None else {"lpips"} for m in masks]
    assert many[9] == {"lpips": 0.0, "bg_lpips": 0.0} and calc.calculate_lpips(pil["a"], pil["c"]) == many[1]["lpips"]
    e = lo.score_error("full")
    for i, p in enumerate(lo.PAIRS):
        assert abs(many[i]["lpips"] - lo.score_of("full", p, "f64")) <= 4 * e * lo.score_of("full", p, "f64")
    s = {}
    for prec, dt in lo.DTYPES.items():
        with torch.no_grad():
            ta, tb = (lo.tower(lo.scaled(np.asarray(small[n].resize((512, 512), Image.LANCZOS)), dt), dt) for n in ("a", "d"))
        s[prec] = lo.total(lo.layers(ta, tb))
    e = max(e, abs(s["f32"] - s["f64"]) / s["f64"])
    print(f"[lpips] 300 x 200 pair: device {many[3]['lpips']:.9e} float64 {s['f64']:.9e} error {abs(many[3]['lpips'] - s['f64']) / s['f64']:.3e} (bound {4 * e:.3e})")
    assert abs(many[3]["lpips"] - s["f64"]) <= 4 * e * s["f64"]
    allm = calc.calculate_all_metrics(pil["a"], pil["c"], "p", mask=band)
    assert list(allm) == ["ssim", "lpips", "clip_score", "psnr", "mse", "dino_distance", "bg_ssim", "bg_psnr", "bg_mse", "bg_lpips"]
    assert allm["lpips"] == many[1]["lpips"] and allm["bg_lpips"] == many[1]["bg_lpips"]
    none = MetricsCalculator("cuda")
    assert none.calculate_lpips(pil["a"], pil["b"]) is None and none.calculate_lpipses([pil["a"]], [pil["b"]]) == [None]
    assert none.calculate_all_metrics(pil["a"], pil["c"], "p")["lpips"] is None


# ---------------------------------------------------------------------------------------------------------------------- in the edit
@pytest.fixture(scope="module")
def editors(fie, wdir):
    from src.pipeline import FastEditor
    return FastEditor(model_name="tiny", enable_cpu_offload=False), FastEditor(model_name="tiny", enable_cpu_offload=False, lpips_dir=wdir)


def test_edit_with_inline_lpips(editors, wdir):
    """edit(metrics=True) with the directory: the same image bytes and the same other keys as without it; lpips / bg_lpips are exactly what the
    calculator gives on (source, returned image)."""
    from src.metrics import MetricsCalculator
    plain_ed, ed = editors
    calc = MetricsCalculator("cuda", lpips_dir=wdir)
    img = Image.fromarray(do.images(256)["c"])
    mask = np.zeros((256, 256), np.uint8)
    mask[40:150, 60:200] = 255
    for kw, keys in ((dict(), ["ssim", "psnr", "mse"]), (dict(mask=mask, paste_back=True, mask_blur=0), ["ssim", "psnr", "mse", "bg_ssim", "bg_psnr", "bg_mse"])):
        base, base_m = plain_ed.edit(img, "a red kite", seed=42, metrics=True, **kw)
        out, m = ed.edit(img, "a red kite", seed=42, metrics=True, **kw)
        extra = ["lpips", "bg_lpips"] if kw else ["lpips"]
        assert list(base_m) == keys and list(m) == keys + extra
        assert np.array_equal(np.asarray(out), np.asarray(base)) and all(m[k] == base_m[k] for k in base_m)
        plain = ed.edit(img, "a red kite", seed=42, **kw)
        assert isinstance(plain, Image.Image) and np.array_equal(np.asarray(plain), np.asarray(base))
        want = calc.calculate_lpipses([img], [out], [mask] if kw else None)[0]
        print(f"[lpips] inline {sorted(kw)}: {[m[k] for k in extra]!r} vs calculator on the returned image {want!r}")
        assert {k: m[k] for k in extra} == want and all(v > 0 for v in want.values())
    outs, ms = ed.edit_batch([img, img], ["a red kite", "an orange cat"], seed=7, strength=0.5, masks=[mask, None], metrics=True)
    want = calc.calculate_lpipses([img, img], outs, [mask, None])
    assert [{k: m[k] for k in m if "lpips" in k} for m in ms] == want and set(want[0]) == {"lpips", "bg_lpips"} and set(want[1]) == {"lpips"}
