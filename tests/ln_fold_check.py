"""Float64 references, builders, checkers and defect models of tests/test_ln_fold_gpu.py: the LayerNorm-folded GEMM (include/fie.h: fie_gemm_ln_f16)
per element.  Device-agnostic torch; tests/test_ln_fold_check_cpu.py runs every checker on every defect model.  The comparisons themselves are
launch_check's (exact_mismatches, ulp_mismatches, precision_ratio, precision_mismatches); this module supplies what they are fed.

The reference is the kernel's own formula in float64 on the STORED operands (tests/test_host_cpu.py pins the fold algebra; this pins the device):

    ref = (x Wf^T - mean S) rstd + b'        x f16, Wf the packed f16 matrix, (S, b') the fp32 table as stored,
    mean, var = E[x^2] - mean^2 from x in float64, rstd = (max(var, 0) + eps)^-1/2; GEGLU: value * gelu(gate) on the packed (value, gate) column pairs.

  pass 1  integer rows x[m, k] = c_m + a_m s[m, k], s = +-1 with exactly K / 2 of each: (x - mean) / sigma = s exactly, ref = s Wf^T + b' whatever c_m and
          a_m are, every sum (acc, sum x, sum x^2, S, b') an integer below 2^24 -> ONE valid f16 answer; any mix-up of rows, fragments, k-slices, lanes or
          table columns moves whole elements.  Called with eps = 2^-40 (positive, and gone against a_m^2 in fp32).
  pass 2  real rows of six classes in one tensor (ROW_CLASSES), per element and never normalised by a maximum:
              |out - ref| <= 0.5 ulp16 + C sqrt(K) 2^-24 [ rstd (|x||Wf|^T + mean|x| |S|) + (E[x^2] + mean^2) / (max(var, 0) + eps) |ref - b'| ]
          first term: the fp32 chains of acc and of mean * S; second: the cancellation in E[x^2] - mean^2 carried into rstd.
  pass 3  every tile adds K in the same order: the outputs of pass 2 are the same bits on every tile (the GPU test's own assertion).
"""
import math

import torch

import launch_check as lc

ACT_NONE, ACT_GEGLU = 0, 4
EPS_INT = 2.0 ** -40                 # pass 1: positive as the entry requires, below half an fp32 ulp of a_m^2 >= 1
PREFILL = -777.0                     # what the gaps between output rows hold before a launch (ldc > N)
ROW_CLASSES = ("offset 0 sigma", "offset 3 sigma", "offset 30 sigma", "offset 300 sigma", "sigma 0.01", "constant")
GATE_NNZ = 1                         # pass 1, GEGLU: non-zero weights per gate row (and gate biases in {-2..2}), so that |gate| <= 2 + 2 + 2 = 6
BK = 64                              # the kernels' K-step (csrc/gemm_tiles.h); a lane's k-slice within it: (k // 8) % 4


def packed_order(n, geglu, device=None):
    """packed row -> source row (GEGLU: value / gate rows interleaved, as fie_pack_rows_f16 with interleave2)."""
    i = torch.arange(n, device=device)
    return torch.stack([i[: n // 2], i[: n // 2] + n // 2], 1).reshape(-1) if geglu else i


def fold(case):
    """(Wf [N, K] f16 in the packed row order, table [N, 2] fp32) of a case: hip.fold_layernorm_tables, the host code the product runs."""
    from fie_amd.hip import fold_layernorm_tables
    wf, tab = fold_layernorm_tables(case["w"], case["bias"], case["gamma"], case["beta"], geglu=case["geglu"])
    return wf[packed_order(wf.shape[0], case["geglu"], wf.device)].contiguous(), tab


# ------------------------------------------------------------------------------------------------------------------------------- builders
def integer_case(M, N, K, gen, geglu=False):
    """Pass 1 (module docstring).  W in {-1, 0, 1}, gamma in {1, 2}, beta in {-2..2}, bias in {-8..8}, c_m in {-3..3}, a_m in {1, 2, 4}; GEGLU: GATE_NNZ
    non-zero weights per gate row and gate biases in {-2..2}.  Asserted: the ranges, K / 2 of each sign per row, every partial sum below 2^24, and
    |ref| <= 2048 (above it odd integers are f16 ties, and eps, however small, moves the float64 reference off a tie that the kernel's fp32 value
    sits on)."""
    assert K % 2 == 0 and N % 2 == 0
    ri = lambda lo, hi, *shape: torch.randint(lo, hi + 1, shape, generator=gen)
    half = torch.cat([torch.ones(K // 2), -torch.ones(K // 2)])
    s = half[torch.rand(M, K, generator=gen).argsort(1)]
    c, a = ri(-3, 3, M, 1).float(), (2 ** ri(0, 2, M, 1)).float()
    w = ri(-1, 1, N, K).float()
    if geglu:
        keep = torch.rand(N // 2, K, generator=gen).argsort(1).argsort(1) < GATE_NNZ
        w[N // 2:] = torch.where(keep, ri(0, 1, N // 2, K).float() * 2 - 1, torch.zeros(()))
    gamma, beta, bias = ri(1, 2, K).float(), ri(-2, 2, K).float(), ri(-8, 8, N).float()
    if geglu:
        bias[N // 2:] = ri(-2, 2, N // 2).float()
    x = c + a * s
    assert bool((s.sum(1) == 0).all()) and bool((s.abs() == 1).all())
    assert x.abs().max() <= 7 and w.abs().max() <= 1 and 1 <= gamma.min() and gamma.max() <= 2 and beta.abs().max() <= 2 and bias.abs().max() <= 8
    wf = w * gamma
    assert float(x.abs().max()) * float(wf.abs().sum(1).max()) < 2 ** 24 and float((x * x).sum(1).max()) < 2 ** 24
    pre = s.double() @ wf.double().t() + (w.double() @ beta.double() + bias.double())
    ref = pre[:, : N // 2] * lc.gelu64(pre[:, N // 2:]) if geglu else pre
    assert float(ref.abs().max()) <= 2048, float(ref.abs().max())
    return dict(M=M, N=N, K=K, geglu=geglu, integer=True, x=x.half(), w=w.half(), gamma=gamma.half(), beta=beta.half(), bias=bias.half(), s=s, cls=None)


def real_case(M, N, K, gen, geglu=False):
    """Pass 2: row m is of class m % 6 (ROW_CLASSES): unit-sigma rows around a common offset of 0 / 3 / 30 / 300 sigma (either sign), sigma = 0.01 around
    0.03, and constant rows (var clamps to 0, rstd = eps^-1/2) up to +-50, where the fp32 E[x^2] - mean^2 is noise far above eps of either sign.
    Weights as the product's: W ~ N(0, 1 / K), gamma ~ 1 + 0.2 N, beta, bias ~ 0.1 N."""
    rn = lambda *shape: torch.randn(*shape, generator=gen)
    cls = torch.arange(M) % len(ROW_CLASSES)
    sign = torch.where(torch.rand(M, generator=gen) < 0.5, -1.0, 1.0)
    off = torch.tensor([0.0, 3.0, 30.0, 300.0, 0.03, 0.0])[cls] * sign
    sig = torch.tensor([1.0, 1.0, 1.0, 1.0, 0.01, 0.0])[cls]
    const = (torch.rand(M, generator=gen) * 100 - 50) * (cls == 5)
    x = (off + const)[:, None] + sig[:, None] * rn(M, K)
    return dict(M=M, N=N, K=K, geglu=geglu, integer=False, x=x.half(), w=(rn(N, K) / math.sqrt(K)).half(), gamma=(1 + 0.2 * rn(K)).half(),
                beta=(0.1 * rn(K)).half(), bias=(0.1 * rn(N)).half(), cls=cls)


def easy_case(M, N, K, gen, geglu=False):
    """The rows of tests/test_ops_gpu.py::test_gemm_with_layernorm_folded_in (sigma 2, common offset ~ 3 sigma): what the old metric was run on."""
    c = real_case(M, N, K, gen, geglu)
    c["x"] = (torch.randn(M, K, generator=gen) * 2 + torch.randn(M, 1, generator=gen) * 6).half()
    c["cls"] = torch.zeros(M, dtype=torch.long)
    return c


# ------------------------------------------------------------------------------------------------------------------------------ reference
class Ref:
    """ref: float64 output [M, nout]; budget: the bracket of pass 2's bound (module docstring) carried through the activation; absref: the |.| budget
    rstd (|x||Wf|^T + mean|x| |S|) + |b'| that pass 1's floors scale; mean, rstd: the float64 row statistics."""

    def __init__(self, ref, budget, absref, mean, rstd):
        self.ref, self.budget, self.absref, self.mean, self.rstd = ref, budget, absref, mean, rstd


def reference(x, wf, tab, eps, act=ACT_NONE):
    """x [M, K] f16 (any row stride), wf [N, K] f16 packed order, tab [N, 2] fp32 -> Ref, everything float64 on x's device."""
    xd, wd, S, b = x.double(), wf.double(), tab[:, 0].double()[None, :], tab[:, 1].double()[None, :]
    mean, ex2 = xd.mean(1, keepdim=True), (xd * xd).mean(1, keepdim=True)
    var0 = (ex2 - mean * mean).clamp_min(0.0)
    rstd = (var0 + eps).rsqrt()
    lin = (xd @ wd.t() - mean * S) * rstd
    chain = rstd * (xd.abs() @ wd.abs().t() + xd.abs().mean(1, keepdim=True) * S.abs())
    budget = chain + (ex2 + mean * mean) / (var0 + eps) * lin.abs()
    pre, absref = lin + b, chain + b.abs()
    return Ref(lc.act64(pre, act), lc.act_abs64(pre, budget, act), lc.act_abs64(pre, absref, act), mean, rstd)


def layernorm_linear64(x, case, eps):
    """The TRUE LayerNorm -> Linear (-> GEGLU) of a case in float64, unfolded and from the unrounded W * gamma (the accuracy table's yardstick)."""
    xd = x.double()
    mean = xd.mean(1, keepdim=True)
    var = ((xd - mean) ** 2).mean(1, keepdim=True)
    y = (xd - mean) * (var + eps).rsqrt() * case["gamma"].double() + case["beta"].double()
    y = y @ case["w"].double().t() + case["bias"].double()
    n = y.shape[1]
    return y[:, : n // 2] * lc.gelu64(y[:, n // 2:]) if case["geglu"] else y


# ------------------------------------------------------------------------------------------------------------------------------- checkers
def pass1_mismatches(out, r, act, rsqrt_exact=True):
    """(count, first positions).  Plain: f16 `out` against the float64 reference rounded once; the 1-ulp form with a 2^-22 floor only if the device's
    rsqrtf turns out inexact at 1, 4, 16 (lc.ulp_mismatches, as the fp8 flows of the launch table).  GEGLU evaluates gelu in fp32: 1 ulp, floor 2^-18."""
    if act == ACT_GEGLU:
        return lc.ulp_mismatches(out, r.ref, 1, 2.0 ** -18 * r.absref)
    if rsqrt_exact:
        return lc.exact_mismatches(out, r.ref)
    return lc.ulp_mismatches(out, r.ref, 1, 2.0 ** -22 * r.absref)


def pass2_ratio(out, r, K):
    """Worst (|out - ref| - 0.5 ulp16) / (sqrt(K) 2^-24 budget); inf where out is not finite."""
    return lc.precision_ratio(out, r.ref, r.budget, K)


def pass2_where(out, r, K):
    """(ratio, (row, column)) of the worst element."""
    o = out.double()
    excess = ((o - r.ref).abs() - 0.5 * torch.maximum(lc.ulp16(r.ref), lc.ulp16(o))).clamp_min(0.0)
    ratio = excess / (math.sqrt(K) * 2.0 ** -24 * r.budget).clamp_min(1e-300)
    ratio = torch.where(torch.isfinite(o), ratio, torch.full_like(ratio, float("inf")))
    i = int(ratio.argmax())
    return float(ratio.flatten()[i]), (i // ratio.shape[1], i % ratio.shape[1])


def pass2_mismatches(out, r, K, c):
    return lc.precision_mismatches(out, r.ref, r.budget, K, c)


def ratio_by_class(out, r, K, cls):
    """Worst pass-2 ratio of each row class present."""
    return {ROW_CLASSES[c]: pass2_ratio(out[cls == c], Ref(r.ref[cls == c], r.budget[cls == c], None, None, None), K) for c in sorted(set(cls.tolist()))}


def gaps_untouched(buf, nout):
    """The columns between the rows of an output buffer [M, ldc] still hold PREFILL."""
    return bool((buf[:, nout:] == PREFILL).all())


def old_metric(out, x, case, eps=1e-5):
    """What tests/test_ops_gpu.py asserts < 3e-3: max |out - ref| / max |ref| against LayerNorm -> Linear in fp32 (one number per tensor)."""
    import torch.nn.functional as F
    k, n = x.shape[1], case["w"].shape[0]
    y = F.layer_norm(x.float(), (k,), case["gamma"].float(), case["beta"].float(), eps) @ case["w"].float().t() + case["bias"].float()
    ref = y[:, : n // 2] * F.gelu(y[:, n // 2:]) if case["geglu"] else y
    return float((out.float() - ref).abs().max() / ref.abs().max())


# ---------------------------------------------------------------------------------------------------------------- fp32 model of the kernel
STRUCTURAL = ("mean_spot", "stats_row16", "half_slices", "last_kstep", "hoist", "s_shift", "geglu_tab_unpacked", "inv_k_padded", "past_n")
PRECISION = ("no_eps", "mean_f16", "acc_f16")
DEFECTS = STRUCTURAL + PRECISION + ("no_clamp",)


def applies(defect, case, ldc=None):
    """Whether a structural defect can show at a case at all (the others always can)."""
    M, N, K, geglu = case["M"], case["N"], case["K"], case["geglu"]
    return {"stats_row16": M > 16, "hoist": K > BK, "geglu_tab_unpacked": geglu, "inv_k_padded": K % 128 != 0,
            "past_n": not geglu and N % 16 != 0}.get(defect, True)


def model(x, wf, tab, eps, act=ACT_NONE, defect=None, ldc=None):
    """csrc/gemm_conv.hip's LN-folded kernel in fp32 torch: acc = x Wf^T, row sums of x and x^2, mean = sum * (1 / K), rstd = rsqrt(max(E[x^2] - mean^2, 0)
    + eps), out = f16((acc - mean S) rstd + b') (GEGLU: value * gelu(gate) in fp32).  Returns the output BUFFER [M, ldc] f16 (ldc >= nout, gaps PREFILL).
    defect: one of DEFECTS --
      mean_spot           the mean correction dropped on one column in one 16-row spot (the 128x80 build's anomaly)
      stats_row16         a row takes the statistics of row m ^ 16 (fragment mix-up)
      half_slices         row sums over half the k-slices (one __shfl_xor missing)
      last_kstep          the last K-step missing from the row sums only
      hoist               the first K-step's row sums taken from the next K-step's data (the scheduler hoist ln_pin() prevents)
      s_shift             S shifted by one column
      geglu_tab_unpacked  the GEGLU table in source order, not the packed (value, gate interleaved) one
      inv_k_padded        1 / K from K rounded up to 128
      past_n              columns up to the end of N's 16-column fragment treated as live: table entries past N taken as they lie in memory (not zero)
                          and the results stored, into the gap or the next row
      no_eps, no_clamp    eps dropped; the variance not clamped at 0 (NaN on constant rows)
      mean_f16, acc_f16   the mean / the accumulator rounded to f16"""
    assert defect is None or defect in DEFECTS
    M, K = x.shape
    N = wf.shape[0]
    nout = N // 2 if act == ACT_GEGLU else N
    ldc = ldc or nout
    xf = x.float()
    tab = tab.clone()
    if defect == "s_shift":
        tab[:, 0] = tab[:, 0].roll(1)
    if defect == "geglu_tab_unpacked":
        src = torch.empty_like(tab)
        src[packed_order(N, True, tab.device)] = tab
        tab = src
    S, b = tab[:, 0][None, :], tab[:, 1][None, :]
    acc = xf @ wf.float().t()
    if defect == "acc_f16":
        acc = acc.half().float()
    k = torch.arange(K, device=x.device)
    xs = xf
    if defect == "half_slices":
        xs = xf * ((k // 8) % 4 < 2)
    if defect == "last_kstep":
        xs = xf * (k < K - BK)
    if defect == "hoist" and K > BK:
        xs = xf[:, torch.where(k < BK, k + BK, k)]
    inv_k = torch.tensor(1.0 / ((K + 127) // 128 * 128 if defect == "inv_k_padded" else K), dtype=torch.float32, device=x.device)
    mu = xs.sum(1, keepdim=True) * inv_k
    var = (xs * xs).sum(1, keepdim=True) * inv_k - mu * mu
    if defect != "no_clamp":
        var = var.clamp_min(0.0)
    if defect != "no_eps":
        var = var + torch.tensor(eps, dtype=torch.float32, device=x.device)
    rstd = var.double().rsqrt().float()
    if defect == "mean_f16":
        mu = mu.half().float()
    if defect == "stats_row16":
        m = torch.arange(M, device=x.device)
        partner = torch.where((m ^ 16) < M, m ^ 16, m)
        mu, rstd = mu[partner], rstd[partner]
    pre = (acc - mu * S) * rstd + b
    if defect == "mean_spot":
        col = int(tab[:, 0].abs().argmax())
        pre[:16, col] = acc[:16, col] * rstd[:16, 0] + b[0, col]
    if act == ACT_GEGLU:
        g = pre[:, 1::2]
        out = pre[:, 0::2] * (0.5 * g * (1.0 + torch.erf(g * 0.70710678118654752)))
    else:
        out = pre
    buf = torch.full((M, ldc), PREFILL, dtype=torch.float16, device=x.device)
    buf[:, :nout] = out.half()
    if defect == "past_n" and act == ACT_NONE and N % 16:
        live = (N + 15) // 16 * 16
        extra = ((0.0 - mu * 1.0) * rstd + 1.0).half().expand(M, live - N)        # zero weight rows, (S, b') = whatever follows the table: ones here
        flat = buf.view(-1)
        pos = (torch.arange(M, device=x.device)[:, None] * ldc + torch.arange(N, live, device=x.device)[None, :])
        ok = pos < flat.numel()
        flat[pos[ok]] = extra[ok]
    return buf
