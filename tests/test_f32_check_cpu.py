"""The checkers and cases of tests/test_f32_contract_gpu.py (tests/f32_check.py) on CPU models of csrc/f32.hip with one defect each.

For every defect the new cases must flag it, at the shapes the GPU test runs; what tests/test_fp32_gpu.py asserts (max |out - ref| / max |ref| < 2e-5 on
its own N(0, 1) inputs) is evaluated next to it.  OLD_METRIC_MISSES lists exactly the defects that metric passes, and they are the ones its inputs
never reach: the A-concat seam, the row-bias row decode, a GEGLU pair stored past N (it looks at no neighbour) and the tap decode with the padded Cin
(its convs have Cin % 8 == 0).  The others it does see: a dropped K tail 0.32, swapped or lost GEGLU pairs, a wrong causal limit, batch stride or
[K][N] staging 1 and more (through its attention test, the old suite's only [K][N] calls), and the arithmetic ones too -- 10-bit operands 6.3e-4, bf16
5.6e-3, an f16 accumulator 8.4e-3 against its 2e-5.  What it cannot do is say where, or hold the path tighter than 2e-5 of a maximum: the new bound is
2^-24-sized per element, and the reduced-precision models land 3 664 x (TF32-like operands) to 25 928 x (bf16) above C_F32."""
import pytest
import torch

import attn_norm_check as an
import f32_check as fc
from test_f32_contract_gpu import B, C_ACT32, C_ATTN32, C_F32, C_SM, CONCAT, CONVS, GEGLU_SHAPES, H, KN_SHAPES, TRIPLES

OLD_BOUND = 2e-5                      # tests/test_fp32_gpu.py
OLD_METRIC_MISSES = {"concat_seam", "rowbias_div", "geglu_pair_past_n", "tap_padded_cin"}
DEV = torch.device("cpu")


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _flags(buf, case, h, habs, c_f32, c_act):
    """True when a checker of the GPU test flags the model's output buffer ([M, Nout + 1]: the last column is padding)."""
    out, pad = buf[:, :-1], buf[:, -1]
    if not bool((pad == fc.PREFILL).all()):
        return True
    act = case["act"]
    if case["integer"]:
        if act in (fc.ACT_NONE, fc.ACT_RELU):
            return fc.exact32_mismatches(out, fc.finish64(h, habs, case)[0])[0] > 0
        return fc.act32_mismatches(out, h, act, c_act, case["scale"], case["residual"])[0] > 0
    ref, budget = fc.finish64(h, habs, case)
    return fc.mismatches32(out, ref, budget, case["K"], c_f32, case["residual"])[0] > 0


def _gemm_cases():
    """name -> (case, w_kn): instances of every GEMM family of the GPU test, integer and real."""
    cases = {}
    for integer in (True, False):
        t = "int" if integer else "real"
        for i, (M, N, K) in enumerate(TRIPLES):
            if K in (5, 17, 33, 200) or (M, N) == (65, 65):
                cases[f"{t} {M}x{N}x{K} relu rowbias"] = (fc.gemm_case(M, N, K, _gen(i), integer, bias=True, rpb=7, residual=True, scale=0.5, act=fc.ACT_RELU), False)
                cases[f"{t} {M}x{N}x{K} silu"] = (fc.gemm_case(M, N, K, _gen(100 + i), integer, bias=True, scale=2.0, act=fc.ACT_SILU), False)
        for i, (M, N, K) in enumerate(GEGLU_SHAPES):
            cases[f"{t} geglu {M}x{N}x{K}"] = (fc.gemm_case(M, N, K, _gen(200 + i), integer, bias=True, act=fc.ACT_GEGLU), False)
        for i, (k1, k2) in enumerate(CONCAT):
            cases[f"{t} concat {k1}+{k2}"] = (fc.gemm_case(65, 64, k1 + k2, _gen(300 + i), integer, K1=k1), False)
        for i, (M, N, K) in enumerate(KN_SHAPES):
            cases[f"{t} kn {M}x{N}x{K}"] = (fc.gemm_case(M, N, K, _gen(400 + i), integer), True)
    return cases


def _conv_cases():
    cases = {}
    for integer in (True, False):
        for i, (hh, ww, cin, cout, stride, pad_mode, ups, raw, bias, rowbias, res, _, scale, act) in enumerate(CONVS):
            cases[f"{'int' if integer else 'real'} conv {i} {hh}x{ww} Cin={cin} raw={raw}"] = (
                fc.conv_case(B, hh, ww, cin, cout, _gen(500 + i), integer, stride=stride, pad_mode=pad_mode, ups=ups, bias=bias, rowbias=rowbias,
                             residual=res, scale=scale, act=act), raw)
    return cases


@pytest.fixture(scope="module")
def gemm_cases():
    return _gemm_cases()


@pytest.fixture(scope="module")
def conv_cases():
    return _conv_cases()


def _flagged_gemm(cases, defect, c_f32, c_act):
    hits = []
    for name, (case, w_kn) in cases.items():
        h, habs = fc.gemm_ref64(case)
        if _flags(fc.gemm_model(case, defect, w_kn), case, h, habs, c_f32, c_act):
            hits.append(name)
    return hits


def _flagged_conv(cases, defect, c_f32, c_act):
    hits = []
    for name, (case, raw) in cases.items():
        if defect == "tap_padded_cin" and not raw:            # packed weights carry the padded Cin in x too: there the decode is right
            continue
        h, habs = fc.conv_ref64(case)
        if _flags(fc.conv_model(case, defect), case, h, habs, c_f32, c_act):
            hits.append(name)
    return hits


# ------------------------------------------------------------------------------------------------------------------ the old metric on the old inputs
def _old_gemm_metric(defect):
    """tests/test_fp32_gpu.py: test_gemm_f32 at (300, 200, 72) and (77, 77, 64): bias, residual, scale 0.5, SiLU, and the GEGLU form."""
    worst = 0.0
    for (m, n, k) in [(300, 200, 72), (77, 77, 64)]:
        g = _gen(m)
        a, w = torch.randn(m, k, generator=g), torch.randn(n, k, generator=g) * k ** -0.5
        base = {"a1": a, "a2": None, "w": w, "M": m, "N": n, "K": k, "K1": k, "bias": torch.randn(n, generator=g), "rowbias": None, "rpb": 0, "integer": False}
        case = dict(base, residual=torch.randn(m, n, generator=g), scale=0.5, act=fc.ACT_SILU)
        ref, _ = fc.finish64(*fc.gemm_ref64(case), case)
        worst = max(worst, fc.old_metric(fc.gemm_model(case, defect)[:, :-1], ref))
        if n % 2 == 0:
            case = dict(base, residual=None, scale=1.0, act=fc.ACT_GEGLU)
            ref, _ = fc.finish64(*fc.gemm_ref64(case), case)
            out = fc.gemm_model(case, defect)[:, :-1]
            worst = max(worst, fc.old_metric(out, ref))
    return worst


def _old_conv_metric(defect):
    """test_conv_f32 at (2, 12, 20, 8 -> 24, stride 2): packed weights, Cin % 8 == 0."""
    case = fc.conv_case(2, 12, 20, 8, 24, _gen(1), False, stride=2, bias=True)
    ref, _ = fc.finish64(*fc.conv_ref64(case), case)
    return fc.old_metric(fc.conv_model(case, defect)[:, :-1], ref)


def _old_attn_metric(defect):
    """test_attention_f32 at (1, 2, 77, 77, 64, causal) and (2, 3, 200, 333, 64)."""
    worst = 0.0
    for (b, hn, tq, tk, causal, seed) in [(1, 2, 77, 77, True, 1), (2, 3, 200, 333, False, 2)]:
        g = _gen(seed)
        q, k, v = (torch.randn(b, hn, t, 64, generator=g) for t in (tq, tk, tk))
        ref = an.attn_ref64(q, k, v, 0.125, causal)
        worst = max(worst, fc.old_metric(fc.attn32_model(q, k, v, 0.125, causal, defect), ref))
    return worst


def _record(kind, defect, old, hits):
    print(f"\n[f32 defect] {kind} {defect}: old metric {old:.2e} (bound {OLD_BOUND}); flagged by {len(hits)} cases, e.g. {hits[:4]}")
    assert hits, f"{defect}: no new case flags it"
    if defect in OLD_METRIC_MISSES:
        assert old < OLD_BOUND, f"{defect}: the old metric already sees it ({old:.2e})"
    else:
        assert old >= OLD_BOUND, f"{defect}: the old metric misses it after all ({old:.2e}): move it into OLD_METRIC_MISSES"


# ------------------------------------------------------------------------------------------------------------------ contraction
def test_the_clean_models_pass_every_contraction_check(gemm_cases, conv_cases):
    assert _flagged_gemm(gemm_cases, None, 0.0, 1.0) == []
    assert _flagged_conv(conv_cases, None, 0.0, 1.0) == []


def test_builders_refuse_inexact_integer_data():
    with pytest.raises(AssertionError):
        fc.gemm_case(1, 1, 1, _gen(0), True, scale=0.3)
    case = fc.gemm_case(3, 2, 5, _gen(0), True, bias=True, rpb=2)
    case["bias"] = case["bias"] + 2.0 ** 24
    assert float(fc.gemm_ref64(case)[1].max()) >= 2.0 ** 24        # what the builder's assertion looks at


@pytest.mark.parametrize("defect", fc.GEMM_DEFECTS)
def test_gemm_defect_is_flagged(gemm_cases, defect):
    old = _old_gemm_metric(defect)
    if defect in fc.ATTN_DEFECTS:                               # the old suite's only [K][N] calls are the P V products of its attention test
        old = max(old, _old_attn_metric(defect))
    _record("gemm", defect, old, _flagged_gemm(gemm_cases, defect, C_F32, C_ACT32))


@pytest.mark.parametrize("defect", fc.CONV_DEFECTS)
def test_conv_defect_is_flagged(conv_cases, defect):
    hits = _flagged_conv(conv_cases, defect, C_F32, C_ACT32)
    old = _old_conv_metric(defect)
    print(f"\n[f32 defect] conv {defect}: old metric {old:.2e} (bound {OLD_BOUND}); flagged by {len(hits)} cases, e.g. {hits[:4]}")
    assert hits, f"{defect}: no new case flags it"
    assert (old < OLD_BOUND) == (defect in OLD_METRIC_MISSES), (defect, old)


def test_reduced_precision_operands_land_100x_above_the_constant(gemm_cases):
    """Operands cut to 10 (TF32-like) or 7 (bf16) mantissa bits and an f16 accumulator, on the real-data cases: the figure the GPU test measures (the
    worst ratio32 over its shapes) lands at least 100 x above C_F32, so no constant of the order measured can absorb such an 'optimisation'; the
    least sensitive single case (one row, K = 200) is printed next to it and is flagged as well."""
    for defect in ("operands_tf32", "operands_bf16", "acc_f16"):
        lowest, highest = (float("inf"), None), (0.0, None)
        for name, (case, w_kn) in gemm_cases.items():
            if case["integer"] or case["act"] != fc.ACT_NONE:
                continue
            h, habs = fc.gemm_ref64(case)
            ref, budget = fc.finish64(h, habs, case)
            r = fc.ratio32(fc.gemm_model(case, defect, w_kn)[:, :-1], ref, budget, case["K"], case["residual"])
            lowest, highest = min(lowest, (r, name)), max(highest, (r, name))
        print(f"\n[f32 defect] {defect}: worst ratio over the real GEMM cases {highest[0]:.0f} = {highest[0] / C_F32:.0f} x C_F32 at {highest[1]}; "
              f"the least sensitive case {lowest[0]:.0f} = {lowest[0] / C_F32:.1f} x C_F32 at {lowest[1]}")
        assert highest[0] >= 100.0 * C_F32 and lowest[0] > C_F32, (defect, lowest, highest)


def test_round_mantissa_and_the_fma_chain():
    x = torch.tensor([1.0 + 2.0 ** -11, 1.0 + 3 * 2.0 ** -11, -(1.0 + 2.0 ** -10 + 2.0 ** -12), 3.0])
    assert fc.round_mantissa(x, 10).tolist() == [1.0, 1.0 + 2.0 ** -9, -(1.0 + 2.0 ** -10), 3.0]                  # ties to even, sign kept
    assert torch.equal(fc.round_mantissa(torch.randn(1000, generator=_gen(3)), 7), torch.randn(1000, generator=_gen(3)).bfloat16().float())
    a, w = torch.randn(50, 200, generator=_gen(4)), torch.randn(30, 200, generator=_gen(5))
    chain = fc.fma_chain32(a, w)
    ref = a.double() @ w.double().t()
    assert bool(((chain.double() - ref).abs() <= 200 * 2.0 ** -24 * (a.double().abs() @ w.double().abs().t())).all())       # a chain: inside K 2^-24 |a||w| ...
    assert fc.exact32_mismatches(chain, ref)[0] > 0                                 # ... and not the sum rounded once
    ai, wi = torch.randint(-2, 3, (50, 200), generator=_gen(6)).float(), torch.randint(-2, 3, (30, 200), generator=_gen(7)).float()
    assert fc.exact32_mismatches(fc.fma_chain32(ai, wi), ai.double() @ wi.double().t())[0] == 0      # integer data: every order is exact


# ------------------------------------------------------------------------------------------------------------------ softmax
def test_softmax_checker_and_its_defect():
    s = torch.randn(130, 200, generator=_gen(6)) * 3
    for causal, tq in [(False, 1), (True, 7), (True, 77)]:
        ref, weight, hidden = fc.softmax_ref64(s, 0.125, causal, tq)
        assert fc.softmax_mismatches(fc.softmax_model(s, 0.125, causal, tq), ref, weight, hidden, 1.0)[0] == 0
        if causal:
            bad = fc.softmax_model(s, 0.125, causal, tq, "causal_limit")
            assert fc.softmax_mismatches(bad, ref, weight, hidden, C_SM)[0] > 0 and fc.softmax_ratio(bad, ref, weight, hidden) > C_SM
    ref, weight, hidden = fc.softmax_ref64(s, 1.0, True, 7)
    out = fc.softmax_model(s, 1.0, True, 7)
    out[3, 199] = -0.0                                             # a hidden column that is not +0.0
    assert fc.softmax_mismatches(out, ref, weight, hidden, C_SM) == (1, [(3, 199)]) and fc.softmax_ratio(out, ref, weight, hidden) == float("inf")
    out = fc.softmax_model(s, 1.0, False, 1)
    ref, weight, hidden = fc.softmax_ref64(s, 1.0, False, 1)
    out[5, 7] *= 1.0 + 2.0 ** -14                                   # one weight off by 2^-14 relative (~1000 x 2^-24)
    assert fc.softmax_mismatches(out, ref, weight, hidden, C_SM)[1] == [(5, 7)]


# ------------------------------------------------------------------------------------------------------------------ attention
def _attn_cases():
    cases = {"selector 17x65": (fc.selector32(B, H, 17, 65, 64, _gen(1)), "pick"),
             "selector 77x333": (fc.selector32(B, H, 77, 333, 64, _gen(2)), "pick"),
             "selector 17x65 d=40": (fc.selector32(B, H, 17, 65, 40, _gen(3)), "pick"),
             "ramp 15x63": (fc.ramp32(B, H, 15, 63, 64, False, DEV), "pick"),
             "ramp causal 77x333": (fc.ramp32(B, H, 77, 333, 64, True, DEV), "pick"),
             "ramp causal 200x96": (fc.ramp32(B, H, 200, 96, 64, True, DEV), "pick"),
             "uniform c=-8 17x65": (fc.uniform32(B, H, 17, 65, 64, -8.0, False, DEV), "uniform"),
             "uniform causal 77x77": (fc.uniform32(B, H, 77, 77, 64, -8.0, True, DEV), "uniform"),
             "real 77x333": (fc.real32(B, H, 77, 333, 64, False, False, _gen(4)), "real"),
             "real peaky causal 77x77": (fc.real32(B, H, 77, 77, 64, True, True, _gen(5)), "real")}
    for name, (case, kind) in cases.items():
        if kind == "real":
            case["budget"] = fc.attn_budget32(case["q"], case["k"], case["v"], case["scale"], case["causal"])
    return cases


@pytest.fixture(scope="module")
def attn_cases():
    return _attn_cases()


def _flagged_attn(cases, defect, c):
    hits = []
    for name, (case, kind) in cases.items():
        out = fc.attn32_model(case["q"], case["k"], case["v"], case["scale"], case["causal"], defect)
        if kind == "pick":
            n = fc.exact32_mismatches(out, case["expect"].double())[0]
        elif kind == "uniform":
            n = fc.uniform32_mismatches(out, case, c)[0]
        else:
            n = fc.attn32_mismatches(out, *case["budget"], case["k"].shape[2], c)[0]
        if n:
            hits.append(name)
    return hits


def test_attention_builders_hold_their_preconditions(attn_cases):
    """Every loser of an exact case is below 2^-150 in float64 (asserted inside the builders); the float64 attention rounds to the expected rows."""
    for name, (case, kind) in attn_cases.items():
        if kind == "pick":
            assert fc._losers_below(case) < fc.LOSER_MAX, name
            assert fc.exact32_mismatches(case["expect"], an.attn_ref64(case["q"], case["k"], case["v"], case["scale"], case["causal"]))[0] == 0, name
            assert case["q"].dtype == torch.float32
    with pytest.raises(AssertionError):
        fc.ramp32(1, 1, 8, 8, 64, False, DEV, delta=2.0 ** 20)       # a score that is not exact in fp32


def test_the_clean_model_passes_every_attention_check(attn_cases):
    assert _flagged_attn(attn_cases, None, 0.0) == []


@pytest.mark.parametrize("defect", fc.ATTN_DEFECTS)
def test_attention_defect_is_flagged(attn_cases, defect):
    _record("attention", defect, _old_attn_metric(defect), _flagged_attn(attn_cases, defect, C_ATTN32))
