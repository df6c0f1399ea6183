"""The checkers and cases of tests/test_ln_fold_gpu.py (tests/ln_fold_check.py) on an fp32 CPU model of the LayerNorm-folded GEMM with one defect each,
at the GPU test's own shapes and tensors.

The clean model is exact in pass 1 and stays below 1 in pass 2 (it measures 0.26, on a constant row at K = 64).  Every structural defect moves whole
elements in pass 1 wherever it can show at all (lf.applies); the three precision defects exceed C_LN in pass 2 on every shape.  What
tests/test_ops_gpu.py::test_gemm_with_layernorm_folded_in asserts (max |out - ref| / max |ref| < 3e-3) is evaluated next to them: on the rows it runs it
reads 4.2e-4 with and without eps and 1.8e-3 with an f16 mean or accumulator, all three under its bar; the hard rows it cannot run at all, the clean
model reads 5e-3 to 1.2e-2 there."""
import pytest
import torch

import ln_fold_check as lf
from test_ln_fold_gpu import C_LN, EPS_REAL, FAMILIES, N_GEGLU, make_case, shapes

OLD_BOUND = 3e-3                      # tests/test_ops_gpu.py


def _act(geglu):
    return lf.ACT_GEGLU if geglu else lf.ACT_NONE


@pytest.fixture(scope="module")
def int_cases():
    out = []
    for geglu, K in FAMILIES:
        for M, N, _ in shapes(geglu, K):
            case = make_case(M, N, K, geglu, True)
            wf, tab = lf.fold(case)
            out.append((case, wf, tab, lf.reference(case["x"], wf, tab, lf.EPS_INT, _act(geglu))))
    return out


@pytest.fixture(scope="module")
def real_cases():
    out = []
    for geglu, K in FAMILIES:
        for M, N, _ in shapes(geglu, K):
            case = make_case(M, N, K, geglu, False)
            wf, tab = lf.fold(case)
            out.append((case, wf, tab, {eps: lf.reference(case["x"], wf, tab, eps, _act(geglu)) for eps in EPS_REAL}))
    return out


def test_integer_builder_gives_rows_whose_answer_ignores_offset_and_scale(int_cases):
    """(x - mean) / sigma = s exactly: the float64 reference of the kernel's formula equals s Wf^T + b' (to the 2^-41 that eps = 2^-40 leaves in rstd),
    and the table holds integers."""
    for case, wf, tab, r in int_cases:
        pre = case["s"].double() @ wf.double().t() + tab[:, 1].double()
        exact = lf.lc.act64(pre, _act(case["geglu"]))
        assert bool((tab == tab.round()).all())
        assert float((r.ref - exact).abs().max()) <= 1e-9 * float(exact.abs().max())
        if not case["geglu"]:
            assert lf.lc.exact_mismatches(exact.half(), r.ref)[0] == 0


def test_clean_model_is_exact_in_pass_1(int_cases):
    for case, wf, tab, r in int_cases:
        act = _act(case["geglu"])
        out = lf.model(case["x"], wf, tab, lf.EPS_INT, act)
        n, where = lf.pass1_mismatches(out, r, act)
        assert n == 0, (case["M"], case["N"], case["K"], case["geglu"], n, where)
        # the 1-ulp form kept for a device whose rsqrtf is inexact at 1, 4, 16 passes what the exact form passes
        assert lf.pass1_mismatches(out, r, act, rsqrt_exact=False)[0] == 0


def test_pass_1_at_the_product_eps_would_not_be_exact(int_cases):
    """Why pass 1 calls with eps = 2^-40: with 1e-5 the elements whose exact value is 0 come out as ~ 5e-6 b'."""
    case, wf, tab, r = next(c for c in int_cases if c[0]["K"] == 640 and not c[0]["geglu"] and c[0]["M"] == 300)
    assert lf.pass1_mismatches(lf.model(case["x"], wf, tab, 1e-5), r, lf.ACT_NONE)[0] > 0


@pytest.mark.parametrize("defect", lf.STRUCTURAL)
def test_structural_defects_move_whole_elements_in_pass_1(int_cases, defect):
    seen = 0
    for case, wf, tab, r in int_cases:
        if not lf.applies(defect, case):
            continue
        act, nout = _act(case["geglu"]), r.ref.shape[1]
        seen += 1
        buf = lf.model(case["x"], wf, tab, lf.EPS_INT, act, defect)
        n, _ = lf.pass1_mismatches(buf[:, :nout], r, act)
        assert n > 0, (defect, case["M"], case["N"], case["K"], case["geglu"])
        assert lf.pass1_mismatches(buf[:, :nout], r, act, rsqrt_exact=False)[0] > 0
    assert seen >= 2, defect


def test_columns_past_n_reach_the_gaps_of_a_strided_output(int_cases):
    """The strided case of the GPU test (ldc = nout + 8): a kernel that treats N's whole last fragment as live leaves the rows right and writes the gaps."""
    case, wf, tab, r = next(c for c in int_cases if c[0]["N"] == 200 and c[0]["M"] == 300 and c[0]["K"] == 640)
    buf = lf.model(case["x"], wf, tab, lf.EPS_INT, defect="past_n", ldc=208)
    assert lf.pass1_mismatches(buf[:, :200], r, lf.ACT_NONE)[0] == 0 and not lf.gaps_untouched(buf, 200)
    assert lf.gaps_untouched(lf.model(case["x"], wf, tab, lf.EPS_INT, ldc=208), 200)


def test_clean_model_stays_below_1_in_pass_2(real_cases):
    worst = (0.0, None)
    for case, wf, tab, refs in real_cases:
        for eps, r in refs.items():
            out = lf.model(case["x"], wf, tab, eps, _act(case["geglu"]))
            ratio, at = lf.pass2_where(out, r, case["K"])
            assert ratio == lf.pass2_ratio(out, r, case["K"])
            if ratio > worst[0]:
                worst = (ratio, f"M={case['M']} N={case['N']} K={case['K']} geglu={case['geglu']} eps={eps} element {at}")
            assert ratio < 1, (ratio, at)
            assert lf.pass2_mismatches(out, r, case["K"], 1.0)[0] == 0
    print(f"clean fp32 model, pass 2: worst ratio {worst[0]:.3f} at {worst[1]} (the device, summing in its own order: MEASURED_RATIO, C_LN = {C_LN})")


@pytest.mark.parametrize("defect", lf.PRECISION)
def test_precision_defects_exceed_the_budget_in_pass_2(real_cases, defect):
    """On every shape and eps, and already on the rows that are not constant (where a dropped eps is finite)."""
    lowest = float("inf")
    for case, wf, tab, refs in real_cases:
        act, keep = _act(case["geglu"]), case["cls"] != 5
        for eps, r in refs.items():
            out = lf.model(case["x"], wf, tab, eps, act, defect)
            sub = lf.Ref(r.ref[keep], r.budget[keep], None, None, None)
            ratio = lf.pass2_ratio(out[keep], sub, case["K"])
            lowest = min(lowest, ratio)
            assert ratio > C_LN, (defect, case["M"], case["N"], case["K"], case["geglu"], eps, ratio)
            assert lf.pass2_ratio(out, r, case["K"]) >= ratio and lf.pass2_mismatches(out, r, case["K"], C_LN)[0] > 0
    print(f"{defect}: lowest worst ratio over the cases {lowest:.1f} (C_LN = {C_LN})")


def test_unclamped_variance_is_flagged_on_constant_rows(real_cases):
    hit = 0
    for case, wf, tab, refs in real_cases:
        for eps, r in refs.items():
            ratio = lf.pass2_ratio(lf.model(case["x"], wf, tab, eps, _act(case["geglu"]), "no_clamp"), r, case["K"])
            if case["M"] == 300:                         # 50 constant rows: some E[x^2] - mean^2 comes out below -eps in fp32
                assert ratio == float("inf"), (case["N"], case["K"], eps)
            hit += ratio == float("inf")
    assert hit


def test_old_metric_misses_what_the_budget_catches():
    """max |out - ref| / max |ref| < 3e-3 against fp32 LayerNorm -> Linear: on the rows the old test runs, eps dropped reads the same as the clean model
    and an f16 mean or accumulator stays under the bar; on the hard rows of pass 2 (the constant ones left out: finite for every model) the CLEAN model
    is over the bar, so the old test could never include them.  The budget flags all three there."""
    M, N, K = 256, 192, 640
    easy = lf.easy_case(M, N, K, torch.Generator().manual_seed(5))
    wf, tab = lf.fold(easy)
    old = {d: lf.old_metric(lf.model(easy["x"], wf, tab, 1e-5, defect=d), easy["x"], easy) for d in (None,) + lf.PRECISION}
    print("old metric, easy rows:", {str(k): f"{v:.2e}" for k, v in old.items()})
    assert old[None] < OLD_BOUND and abs(old["no_eps"] - old[None]) <= 0.05 * old[None]
    assert old["mean_f16"] < OLD_BOUND and old["acc_f16"] < OLD_BOUND
    hard = lf.real_case(M + 2, N, K, torch.Generator().manual_seed(6))
    keep = hard["cls"] != 5
    x = hard["x"][keep]
    wf, tab = lf.fold(hard)
    r = lf.reference(x, wf, tab, 1e-5)
    old_h = {d: lf.old_metric(lf.model(x, wf, tab, 1e-5, defect=d), x, hard) for d in (None,) + lf.PRECISION}
    new_h = {d: lf.pass2_ratio(lf.model(x, wf, tab, 1e-5, defect=d), r, K) for d in (None,) + lf.PRECISION}
    print("old metric, hard rows:", {str(k): f"{v:.2e}" for k, v in old_h.items()})
    print("pass-2 ratio, hard rows:", {str(k): f"{v:.3g}" for k, v in new_h.items()})
    assert old_h[None] > OLD_BOUND
    assert new_h[None] < 1 and all(new_h[d] > C_LN for d in lf.PRECISION)


def test_reference_carries_geglu_in_the_packed_order():
    """value * gelu(gate) on the interleaved column pairs of the packed table, against LayerNorm -> Linear -> GEGLU on the source order."""
    case = make_case(16, N_GEGLU, 64, True, False)
    wf, tab = lf.fold(case)
    keep = case["cls"] < 3
    r = lf.reference(case["x"][keep], wf, tab, 1e-5, lf.ACT_GEGLU)
    true = lf.layernorm_linear64(case["x"][keep], case, 1e-5)
    assert r.ref.shape == true.shape == (int(keep.sum()), N_GEGLU // 2)
    assert float((r.ref - true).abs().max()) < 2e-3 * float(true.abs().max())       # what rounding W * gamma to f16 costs (tests/test_host_cpu.py)
