"""The checkers of tests/test_launch_table_gpu.py (tests/launch_check.py) on crafted outputs, and the product-problem fixture it reads.

Every crafted defect below is one a tile could plausibly have: the checkers must flag each while passing a correct fp32-accumulating result."""
import json
import math
import os

import torch

import launch_check as lc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "launch_problems.json")
C_FP32 = 8.0          # tests/test_launch_table_gpu.py: C_FP32


def _int_problem(M=64, N=48, K=1280, seed=0):
    g = torch.Generator().manual_seed(seed)
    a = torch.randint(-2, 3, (M, K), generator=g).double()
    w = torch.randint(-2, 3, (N, K), generator=g).double()
    bias = torch.randint(-4, 5, (N,), generator=g).double()
    return a, w, bias


def _real_problem(M=32, N=32, K=5120, seed=1):
    g = torch.Generator().manual_seed(seed)
    a = (torch.randn(M, K, generator=g) + 0.25).half().double()
    w = ((torch.randn(N, K, generator=g) + 0.25) / math.sqrt(K)).half().double()
    return a, w


def test_exact_check_passes_the_single_rounded_result_and_flags_one_ulp():
    a, w, bias = _int_problem()
    ref = a @ w.t() + bias
    out = ref.half()
    assert lc.exact_mismatches(out, ref)[0] == 0
    bad = out.clone()
    bad.view(torch.int16)[5, 7] += 1                       # one ulp up at one element
    n, where = lc.exact_mismatches(bad, ref)
    assert n == 1 and where == [(5, 7)]


def test_exact_check_flags_a_fragment_missing_one_k_step():
    a, w, bias = _int_problem()
    ref = a @ w.t() + bias
    bad = ref.clone()
    # one 16x1 fragment (rows 16..31 of column 9) without the contribution of the K-step k = 640..703
    bad[16:32, 9] -= a[16:32, 640:704] @ w[9, 640:704]
    n, _ = lc.exact_mismatches(bad.half(), ref)
    assert n >= 12, n                                      # (a K-step's sum over 64 terms of {-2..2} products is rarely zero)


def test_exact_check_flags_a_column_without_bias_and_swapped_rows():
    a, w, bias = _int_problem()
    bias[3] = 3.0
    ref = a @ w.t() + bias
    nob = ref.clone()
    nob[:, 3] -= bias[3]
    assert lc.exact_mismatches(nob.half(), ref)[0] == ref.shape[0]
    sw = ref.clone()
    sw[[10, 11]] = sw[[11, 10]]
    assert lc.exact_mismatches(sw.half(), ref)[0] > 0


def test_precision_check_passes_fp32_accumulation_and_flags_the_defects():
    a, w = _real_problem()
    K = a.shape[1]
    ref, absref = a @ w.t(), a.abs() @ w.abs().t()
    good = (a.float() @ w.float().t()).half()              # fp32 accumulation, one rounding to f16
    r_good = lc.precision_ratio(good, ref, absref, K)
    assert r_good <= C_FP32, r_good
    # the one-ulp, missing-K-step, missing-bias and swapped-row defects are also far outside the real-data bound
    # (a one-ulp change is pass 1's to catch: next to a rounding midpoint it stays within 0.5 ulp + a hair of the reference; here it is made
    # where the correct output sits closest to the reference)
    bad = good.clone()
    i = int(((good.double() - ref).abs() / lc.ulp16(ref)).argmin())
    bad.view(-1).view(torch.int16)[i] += 1
    assert lc.precision_ratio(bad, ref, absref, K) > C_FP32
    miss = ref.clone()
    miss[16:32, 9] -= a[16:32, 640:704] @ w[9, 640:704]
    assert lc.precision_mismatches(miss.half(), ref, absref, K, C_FP32)[0] >= 8
    sw = good.clone()
    sw[[10, 11]] = sw[[11, 10]]
    assert lc.precision_ratio(sw, ref, absref, K) > C_FP32


def test_precision_check_flags_fp16_accumulation():
    """Where fp16 accumulation lands on the ratio scale: an output summed over K = 5120 in 16-wide fp32 MFMA steps whose running sum is
    rounded to f16 after each step (320 roundings) reaches a worst ratio of ~200; per-term f16 rounding only goes higher.  C_FP32 stays
    far below that point."""
    a, w = _real_problem(M=16, N=16)
    K = a.shape[1]
    ref, absref = a @ w.t(), a.abs() @ w.abs().t()
    acc = torch.zeros(16, 16, dtype=torch.float16)
    ah, wh = a.half(), w.half()
    for k0 in range(0, K, 16):                              # f16 running sum (MFMA-shaped 16-wide steps, each rounded to f16)
        acc = (acc.float() + ah[:, k0:k0 + 16].float() @ wh[:, k0:k0 + 16].float().t()).half()
    r = lc.precision_ratio(acc, ref, absref, K)
    print(f"fp16 accumulation over K={K}: worst ratio {r:.0f} (C_FP32 = {C_FP32})")
    assert r > 10 * C_FP32, r


def test_ulp_and_f8_checks():
    ref = torch.tensor([[1.0, 100.0, -3.0, 0.0]], dtype=torch.float64)
    out = ref.half()
    out.view(torch.int16)[0, 1] += 1
    assert lc.ulp_mismatches(out, ref, 1)[0] == 0
    out.view(torch.int16)[0, 1] += 1
    assert lc.ulp_mismatches(out, ref, 1)[0] == 1
    f8 = ref.float().to(torch.float8_e4m3fn).view(torch.uint8)
    assert lc.f8_mismatches(f8, ref)[0] == 0
    f8[0, 2] += 2                                          # two e4m3 steps
    assert lc.f8_mismatches(f8, ref)[0] == 1


def test_conv_reference_matches_torch_conv():
    """The nine-shifted-GEMM float64 conv (no im2col) against torch's conv2d, for both paddings, stride 2 and the 2x up-sampling."""
    g = torch.Generator().manual_seed(3)
    for stride, pad_mode, ups in ((1, 0, 0), (2, 1, 0), (1, 0, 1), (2, 0, 0)):
        x = torch.randn(2, 6, 10, 8, generator=g, dtype=torch.float64)
        w = torch.randn(5, 8, 3, 3, generator=g, dtype=torch.float64)
        xi = x.repeat_interleave(2, 1).repeat_interleave(2, 2) if ups else x
        H, W = xi.shape[1:3]
        pads = 2 if pad_mode == 0 else 1
        geo = {"stride": stride, "pt": 1 if pad_mode == 0 else 0, "OH": (H + pads - 3) // stride + 1, "OW": (W + pads - 3) // stride + 1}
        taps = [(t // 3, t % 3, w[:, :, t // 3, t % 3]) for t in range(9)]
        got = lc.conv_taps64(xi, taps, geo).view(2, geo["OH"], geo["OW"], 5)
        xc = xi.permute(0, 3, 1, 2)
        xc = torch.nn.functional.pad(xc, (1, 1, 1, 1) if pad_mode == 0 else (0, 1, 0, 1))
        want = torch.nn.functional.conv2d(xc, w, stride=stride).permute(0, 2, 3, 1)
        assert got.shape == want.shape and torch.allclose(got, want, atol=1e-10), (stride, pad_mode, ups)


def test_launch_problems_fixture_well_formed():
    doc = json.load(open(FIXTURE))
    probs = doc["problems"]
    fields = doc["fields"]
    assert set(doc["configs"]) == {"ssd1b_cn", "sdxl_b8", "sdxl_w8", "sdxl_w8a8"}
    seen = set()
    for p in probs:
        for f in fields + ["key", "rule", "in_scope", "configs", "cands_recorded"]:
            assert f in p, (f, p)
        assert p["kind"] in ("gemm", "conv") and p["M"] > 0 and p["N"] > 0 and p["K"] > 0 and 0 < p["K1"] <= p["K"]
        assert p["configs"] and all(n in doc["configs"] and c > 0 for n, c in p["configs"].items())
        assert p["in_scope"] == (not p["ln"] and not p["gna"])
        assert p["in_scope"] == (p["cands_recorded"] is not None)
        assert p["w8"] in (0, 1, 2) and 0 <= p["act"] <= 4 and p["scale"] > 0
        if p["kind"] == "conv":
            assert p["b"] >= 1 and p["Cin"] % 8 == 0 and p["stride"] in (1, 2) and p["pad"] in (0, 1)
            assert p["K"] == (4 if p["parity"] else 9) * p["Cin"] + p["C2"] + p["C3"]
        ident = tuple(p[f] for f in fields)
        assert ident not in seen, f"duplicate record {p['key']}"
        seen.add(ident)
    for name in doc["configs"]:
        assert any(name in p["configs"] for p in probs), name
    # FF1 (M 2048 x N 10240 x K 1280, GEGLU) and the VAE's 1024^2 x 128-channel convs are there
    assert any(p["kind"] == "gemm" and (p["M"], p["N"], p["K"], p["act"]) == (2048, 10240, 1280, 4) for p in probs)
    assert any(p["kind"] == "conv" and (p["H"], p["W"], p["Cin"], p["N"]) == (1024, 1024, 128, 128) for p in probs)
    # the thin-conv rule (77) and the halo conv (72) appear where the product launches them
    assert any(p["rule"] == 77 for p in probs) and any(p["rule"] == 72 for p in probs)
