"""The checkers and cases of tests/test_attn_norm_gpu.py (tests/attn_norm_check.py) on float64 models of the ops with one defect each.

For every defect the new cases must flag it, and what tests/test_ops_gpu.py asserts (one max-norm per tensor, on its N(0, 1) inputs) is
evaluated next to it.  That metric misses the defects that scale a row or a group as a whole: a phantom zero key (1.5e-3 against its 4e-3),
the unbiased variance (2.9e-3 against 3e-3 at n = 200), E[x^2] - mean^2 in one fp32 chain (3e-4: no input of the old suite has a mean).
The others it does see on random data, because a max over the tensor finds the one row whose dropped or leaked key carried a few percent of
the softmax, or because the old suite's smallest group (n = 200) moves by 1 %: dropped last key 0.25, causal mask off by one 1.1 - 1.2,
f16 accumulation 6.5e-3, row count off by one 5.3e-3, statistics of another group 0.13, wrong head / batch / fragment 0.5 - 1.5.  For those
the new cases add the diagnosis (which key, head and batch was read; which rows) and the test asserts the fact as it is: OLD_METRIC_MISSES
lists exactly the defects the old metric passes.  The float64 reference rounded once to f16 passes every checker with the rounding term alone."""
import pytest
import torch

import attn_norm_check as an
import launch_check as lc
from test_attn_norm_gpu import C_ATTN, C_NORM

OLD_ATTN_BOUND, OLD_NORM_BOUND = 4e-3, 3e-3        # tests/test_ops_gpu.py: test_attention, test_groupnorm
# the defects the old max-norm metric passes on its own inputs; it catches the others (module docstring)
OLD_METRIC_MISSES = {"phantom_key", "unbiased_variance", "fp32_single_chain"}
B, H, D = 2, 3, 64
DEV = torch.device("cpu")


def _gen(seed):
    return torch.Generator().manual_seed(seed)


# ------------------------------------------------------------------------------------------------------------------ attention
def _attn_cases():
    """Small instances of every new case family: name -> (case, kind)."""
    cases = {}
    cases["selector 77x97"] = (an.selector_case(B, H, 77, 97, D, 16.0, _gen(1)), "pick")
    cases["selector 200x333"] = (an.selector_case(B, H, 200, 333, D, 16.0, _gen(2)), "pick")
    cases["ramp 17x65"] = (an.ramp_case(B, H, 17, 65, D, False, DEV), "pick")
    cases["ramp causal 77x77"] = (an.ramp_case(B, H, 77, 77, D, True, DEV), "pick")
    cases["ramp causal 33x97"] = (an.ramp_case(B, H, 33, 97, D, True, DEV), "pick")
    cases["ramp causal 97x33"] = (an.ramp_case(B, H, 97, 33, D, True, DEV), "pick")
    for c in (0.0, -8.0, 8.0):
        cases[f"uniform c={c} 17x64"] = (an.uniform_case(B, H, 17, 64, D, c, False, DEV), "uniform")
        cases[f"uniform c={c} 16x77"] = (an.uniform_case(B, H, 16, 77, D, c, False, DEV), "uniform")
        cases[f"uniform causal c={c} 77x77"] = (an.uniform_case(B, H, 77, 77, D, c, True, DEV), "uniform")
    cases["real 77x1024"] = (an.real_case(B, H, 77, 1024, D, False, False, _gen(3)), "real")
    cases["real peaky 77x333"] = (an.real_case(B, H, 77, 333, D, True, False, _gen(4)), "real")
    cases["real causal 77x77"] = (an.real_case(B, H, 77, 77, D, False, True, _gen(5)), "real")
    return cases


@pytest.fixture(scope="module")
def attn_cases():
    return _attn_cases()


def _flagged_attn(cases, defect, c_real):
    """Names of the new cases whose checker flags the model with `defect` (None: the correct op)."""
    hits = []
    for name, (case, kind) in cases.items():
        out = an.attn_model(case["q"], case["k"], case["v"], case["scale"], case["causal"], defect)
        if kind == "pick":
            n, _ = lc.exact_mismatches(out, case["expect"].double())
        elif kind == "uniform":
            n, _ = an.uniform_mismatches(out, case["ref"], case["count"])
        else:
            ref, dev, eps = an.attn_budget64(case["q"], case["k"], case["v"], case["scale"], case["causal"])
            n, _ = an.attn_mismatches(out, ref, dev, eps, c_real)
        if n:
            hits.append(name)
    return hits


def _old_attn_metric(defect):
    """The old metric on the old inputs (tests/test_ops_gpu.py: test_attention, its ragged and its causal shape), worst of the two."""
    worst = 0.0
    for (b, hn, tq, tk, causal, seed) in [(2, 3, 200, 333, False, 1), (2, 12, 77, 77, True, 2)]:
        g = _gen(seed)
        q, k, v = (torch.randn(b, hn, t, D, generator=g).half() for t in (tq, tk, tk))
        ref = an.attn_ref64(q, k, v, D ** -0.5, causal)
        worst = max(worst, an.old_metric(an.attn_model(q, k, v, D ** -0.5, causal, defect), ref))
    return worst


def test_builders_hold_their_preconditions(attn_cases):
    """The gap of at least 40 (asserted inside the builders), and the float64 softmax of every exact case rounds to the expected rows."""
    for name, (case, kind) in attn_cases.items():
        ref = an.attn_ref64(case["q"], case["k"], case["v"], case["scale"], case["causal"])
        if kind == "pick":
            assert case["gap"] >= an.GAP_MIN, name
            assert lc.exact_mismatches(case["expect"], ref)[0] == 0, name
        elif kind == "uniform":
            assert float((ref - case["ref"]).abs().max()) < 1e-12, name
            s = case["v"].double().sum(2)
            assert bool((s == s.round()).all()) and float(case["v"].double().abs().sum(2).max()) < 2 ** 24, name
    # d = 512 (the VAE's mid-block attention): the gap holds with g = 4, and builders given too small a gain or step refuse
    assert an.selector_case(1, 2, 33, 100, 512, 4.0, _gen(6))["gap"] >= an.GAP_MIN
    assert an.ramp_case(1, 2, 33, 100, 512, True, DEV, g=4.0)["gap"] >= an.GAP_MIN
    with pytest.raises(AssertionError):
        an.selector_case(1, 1, 64, 1024, 64, 4.0, _gen(7))
    with pytest.raises(AssertionError):
        an.ramp_case(1, 1, 8, 8, 64, False, DEV, g=1.0, delta=0.5)
    with pytest.raises(AssertionError):
        an.uniform_case(1, 1, 8, 8, 64, -1.0, False, DEV)


def test_the_rounded_reference_passes_every_attention_check(attn_cases):
    assert _flagged_attn(attn_cases, None, 0.0) == []


@pytest.mark.parametrize("defect", an.ATTN_DEFECTS)
def test_attention_defect_is_flagged(attn_cases, defect):
    old = _old_attn_metric(defect)
    hits = _flagged_attn(attn_cases, defect, C_ATTN)
    print(f"\n[attn defect] {defect}: old metric {old:.2e} (bound {OLD_ATTN_BOUND}); flagged by {hits}")
    assert hits, f"{defect}: no new case flags it"
    if defect in OLD_METRIC_MISSES:
        assert old < OLD_ATTN_BOUND, f"{defect}: the old metric already sees it ({old:.2e})"
    else:
        assert old >= OLD_ATTN_BOUND, f"{defect}: the old metric misses it after all ({old:.2e}): move it into OLD_METRIC_MISSES"


def test_a_wrong_pick_is_named(attn_cases):
    case, _ = attn_cases["selector 77x97"]
    out = an.attn_model(case["q"], case["k"], case["v"], case["scale"], False, "v_head_shift")
    n, where = lc.exact_mismatches(out, case["expect"].double())
    assert n and "head 2" in an.describe_pick(out, case, where[0]) and "batch" in an.describe_pick(out, case, where[0])
    out = an.attn_model(case["q"], case["k"], case["v"], case["scale"], False, "drop_last_key")
    n, where = lc.exact_mismatches(out, case["expect"].double())
    assert n and "wanted key 96" in an.describe_pick(out, case, where[0])


def test_attention_ratio_separates_f16_accumulation_from_p_rounding():
    """P rounded to f16 toward zero (what the kernel does, numerator and denominator alike) stays at a ratio of about 1 -- the model behind
    C_ATTN; the same with an f16 accumulator is beyond C_ATTN."""
    case = an.real_case(B, H, 77, 1024, D, False, False, _gen(8))
    q, k, v, scale = case["q"], case["k"], case["v"], case["scale"]
    ref, dev, eps = an.attn_budget64(q, k, v, scale)
    qs = (q.float() * (scale * an.LOG2E)).half().double()                     # Q pre-scaled into f16 (csrc/attention.hip: attn2_kernel)
    s = qs @ k.double().transpose(-1, -2)
    p = torch.exp2(s - s.amax(-1, keepdim=True))
    p16 = p.float().half()
    p16 = torch.where(p16.double() > p, (p16.view(torch.int16) - 1).view(torch.float16), p16).double()      # round toward zero
    out = ((p16 @ v.double()) / p16.sum(-1, keepdim=True)).half()
    r_ok = an.attn_ratio(out, ref, dev, eps)
    r_bad = an.attn_ratio(an.attn_model(q, k, v, scale, False, "pv_f16"), ref, dev, eps)
    print(f"\n[attn ratio] P rounded toward zero in f16: {r_ok:.3f}; f16 accumulator: {r_bad:.1f} (C_ATTN = {C_ATTN})")
    assert r_ok <= 1.0 and r_bad > C_ATTN


# ------------------------------------------------------------------------------------------------------------------ norms
def _norm_cases():
    cases = {}
    for rows, C in [(1, 64), (5, 64), (8, 128)]:
        x = an.gn_two_level(2, rows, C, 32, DEV)
        cases[f"two-level rows={rows} C={C}"] = (x, 32, False)
    cases["offsets rows=100 C=64"] = (an.gn_input(2, 100, 64, 32, _gen(11)), 32, True)
    cases["offsets rows=4096 C=128"] = (an.gn_input(1, 4096, 128, 32, _gen(12)), 32, True)
    return cases


@pytest.fixture(scope="module")
def norm_cases():
    return _norm_cases()


def _flagged_norm(cases, defect, c):
    hits = []
    for name, (x, groups, silu) in cases.items():
        gamma, beta = an.affine(x.shape[-1], DEV)
        ref, slack = an.gn_ref64(x, groups, gamma, beta, 1e-5, silu)
        out = an.gn_model(x, groups, gamma, beta, 1e-5, silu, defect)
        if an.norm_mismatches(out, ref, slack, c)[0]:
            hits.append(name)
    return hits


def _old_norm_metric(defect):
    """The old metric on the old inputs (tests/test_ops_gpu.py: test_groupnorm, x = randn + 0.5): its smallest group (n = 200) and a VAE map."""
    worst = 0.0
    for (rows, C, silu, seed) in [(100, 64, True, 1), (4096, 128, False, 2)]:
        g = _gen(seed)
        x = (torch.randn(1, rows, C, generator=g).half() + 0.5)
        gamma, beta = torch.randn(C, generator=g).half(), torch.randn(C, generator=g).half()
        ref, _ = an.gn_ref64(x, 32, gamma, beta, 1e-5, silu)
        worst = max(worst, an.old_metric(an.gn_model(x, 32, gamma, beta, 1e-5, silu, defect), ref))
    return worst


def test_the_rounded_reference_passes_every_norm_check(norm_cases):
    assert _flagged_norm(norm_cases, None, 0.0) == []
    g = _gen(13)
    for rows, C in [(5, 64), (3, 1032)]:
        x = an.ln_input(rows, C, g)
        gamma, beta = an.affine(C, DEV)
        ref, slack = an.ln_ref64(x, gamma, beta, 1e-5)
        assert an.norm_mismatches(an.to_f16_rne(ref), ref, slack, 0.0)[0] == 0
        assert an.norm_mismatches(ref.float(), ref, slack, 0.0, f32=True)[0] == 0
        # per-row offsets reach 64 sigma, and the affine is asymmetric
        mu, sd = x.double().mean(-1), x.double().std(-1)
        assert float((mu.abs() / sd).max()) > (50 if rows > 2 else 0) and not torch.equal(gamma, gamma.flip(0))


def test_norm_inputs_cover_the_offsets():
    x = an.gn_input(2, 256, 128, 32, _gen(14)).double().view(2, 256, 32, 4)
    r = (x.mean((1, 3)).abs() / x.std((1, 3))).flatten()
    for off in an.OFFSETS:
        assert bool(((r - off).abs() < 0.05 * off + 0.2).any()), f"no group near mean / sigma = {off}"
    assert float(x.abs().max()) < 1000


@pytest.mark.parametrize("defect", an.NORM_DEFECTS)
def test_norm_defect_is_flagged(norm_cases, defect):
    old = _old_norm_metric(defect)
    hits = _flagged_norm(norm_cases, defect, C_NORM)
    print(f"\n[norm defect] {defect}: old metric {old:.2e} (bound {OLD_NORM_BOUND}); flagged by {hits}")
    assert hits, f"{defect}: no new case flags it"
    if defect in OLD_METRIC_MISSES:
        assert old < OLD_NORM_BOUND, f"{defect}: the old metric already sees it ({old:.2e})"
    else:
        assert old >= OLD_NORM_BOUND, f"{defect}: the old metric misses it after all ({old:.2e}): move it into OLD_METRIC_MISSES"


def test_f8_check_against_the_float64_reference():
    """The e4m3 outputs are compared with the float64 reference times the inverse scale (never with the op's own f16 output); the saturating
    case must give exactly +-448."""
    ref = torch.tensor([0.3, -1.7, 500.0, -1000.0, 447.0], dtype=torch.float64)
    good = ref.clamp(-448, 448).float().to(torch.float8_e4m3fn).view(torch.uint8)
    assert lc.f8_mismatches(good, ref, 1)[0] == 0
    assert good.view(torch.float8_e4m3fn).double()[2:4].tolist() == [448.0, -448.0]
    bad = good.clone()
    bad[2] -= 2                                          # 384 instead of the saturated 448: two e4m3 steps
    bad[0] += 2
    assert lc.f8_mismatches(bad, ref, 1)[0] == 2
