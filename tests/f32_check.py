"""Float64 references, input builders, checkers and defect models of tests/test_f32_contract_gpu.py (device-agnostic torch; the CPU self-check
in tests/test_f32_check_cpu.py runs them on the defect models below).  The code under test is csrc/f32.hip: fie_gemm_f32, fie_conv3x3_nhwc_f32,
fie_softmax_rows_f32 and the fp32 attention hip.Context.attention composes from them (Q K^T, row softmax, P V).

Contraction (GEMM / conv), out fp32, ref float64 on the stored fp32 inputs:

  exact32_mismatches   integer data (A, W in {-2..2}, integer bias / row bias / residual, scale a power of two, sum |a||w| + |bias| + |rowbias|
                       < 2^24 asserted by the builder): every fp32 partial sum is exact in any order, so out == fp32(ref) bit for bit (+0 == -0).
  act32_mismatches     the same data behind SiLU / GELU / quick-GELU / GEGLU, which the kernel evaluates in fp32 on the exact sum h:
                       |out - ref| <= C_ACT32 2^-24 (|h| + |act(h)|) |scale|  (+ 0.5 ulp32(ref) when a residual adds one more rounding).  The |h|
                       term is the cancellation in 0.5 x (1 + erf): at x = -5 the bracket is 6e-7 and carries the rounding of 1.0f + erff().
                       GEGLU: |v| (|g| + |gelu(g)|) in place of |h| + |act(h)|.
  ratio32 /            real data, per element, never normalised by a maximum:
  mismatches32             |out - ref| <= 0.5 ulp32 + C sqrt(K) 2^-24 budget + 2^-24 |residual|
                       budget = act_abs(|A||W| + |bias| + |rowbias|) |scale|: an fp32 chain of K terms loses about sqrt(K) 2^-24 of the
                       magnitudes it sums; the residual term is the rounding of x * scale before a residual that may cancel it (|x| <= |out| +
                       |residual|; the |out| share sits in the constant).  Operands cut to 10 mantissa bits land at 2^13 / sqrt(K) times the
                       constant's unit, fp16 accumulation likewise (tests/test_f32_check_cpu.py asserts the multiples).

Softmax, in place over rows of scores s:  |out - ref| <= C_SM 2^-24 (1 + |scale s| + |scale s_max|) ref + 2^-126: the exponent scale * s - max is
  rounded twice (each 2^-24 of its operands, an ABSOLUTE error of the exponent = a relative one of exp), expf, the sum, 1 / sum and the product are a few
  relative roundings; a weight below the smallest normal may be flushed (2^-126).  Masked columns (c > row % tq) are +0.0, bit for bit.

Attention:  |out - ref| <= 0.5 ulp32 + C_ATTN32 (eps32 dev + sqrt(Tk) 2^-24 sum_j w_j |v_jd|), dev = sum_j w_j |v_jd - ref_d| from attn_norm_check.
  attn_budget64 and eps32 = 2^-24 (4 + 2 max_j sum_d |q_d k_jd| scale): a relative error eps of every weight moves the normalised output by at most
  eps dev (the weights still sum to one), and the P V chain loses sqrt(Tk) 2^-24 of what it sums.
  Exact cases (attn_norm_check's selector / ramp / uniform at fp32 gaps): every losing weight of the float64 softmax is below 2^-150 (asserted), so its
  fp32 expf is exactly 0, the row sum exactly 1 and the output exactly V[pi]; uniform rows with a power-of-two count are exact too.

fma_chain32 is the k-ascending fp32 FMA chain csrc/f32.hip's header speaks of (float64 multiply-add rounded to fp32 per step: the product of two fp32
is exact in float64; the float64 sum rounds to 53 bits before it rounds to 24, which differs from one fused rounding only when the 53-bit value lands
exactly on an fp32 tie -- about 2^-29 of the steps).
"""
import math

import torch

import attn_norm_check as an
import launch_check as lc

ACT_NONE, ACT_SILU, ACT_GELU, ACT_QUICK_GELU, ACT_GEGLU, ACT_RELU = 0, 1, 2, 3, 4, 5
TILE, KSTEP = 64, 16                 # csrc/f32.hip: 64 x 64 x 16 tile, four 4-wide MFMA k-steps per stage
LOSER_MAX = 2.0 ** -150              # below half the smallest fp32 denormal: expf rounds (or flushes) to exactly 0
F32_MIN_NORMAL = 2.0 ** -126


# ------------------------------------------------------------------------------------------------------------------ activations with ReLU
def act64(h, act):
    """launch_check.act64 plus FIE_ACT_RELU (5), which only the fp32 entries take."""
    return h.clamp_min(0.0) if act == ACT_RELU else lc.act64(h, act)


def act_abs64(h, habs, act):
    return habs if act == ACT_RELU else lc.act_abs64(h, habs, act)


# ------------------------------------------------------------------------------------------------------------------ checkers
def _ulp(out, ref):
    return torch.maximum(an.ulp32(ref), an.ulp32(out.double()))


def exact32_mismatches(out, ref):
    """(count, first positions) of elements where fp32 `out` differs from fp32(ref), the single rounding of the float64 reference (+0 == -0)."""
    assert out.dtype == torch.float32
    r32 = ref.to(torch.float32)
    bad = (out != r32) & ~(torch.isnan(out) & torch.isnan(r32))
    return int(bad.sum()), lc._where(bad)


def ratio32(out, ref, budget, K, residual=None):
    """Worst (|out - ref| - 0.5 ulp32 - 2^-24 |residual|) / (sqrt(K) 2^-24 budget) over the elements; inf for a non-finite output."""
    o = out.double()
    slack = 0.5 * _ulp(out, ref) + (2.0 ** -24 * residual.double().abs() if residual is not None else 0.0)
    excess = ((o - ref).abs() - slack).clamp_min(0.0)
    denom = math.sqrt(K) * 2.0 ** -24 * budget
    ratio = torch.where(excess > 0, excess / denom.clamp_min(1e-300), torch.zeros_like(excess))
    ratio = torch.where(torch.isfinite(o), ratio, torch.full_like(ratio, float("inf")))
    return float(ratio.max())


def mismatches32(out, ref, budget, K, c, residual=None):
    """(count, first positions) of elements outside |out - ref| <= 0.5 ulp32 + c sqrt(K) 2^-24 budget + 2^-24 |residual|."""
    o = out.double()
    bound = 0.5 * _ulp(out, ref) + c * math.sqrt(K) * 2.0 ** -24 * budget + (2.0 ** -24 * residual.double().abs() if residual is not None else 0.0)
    bad = ~((o - ref).abs() <= bound)
    return int(bad.sum()), lc._where(bad)


def act_slack64(h, act):
    """|h| + |act(h)| (GEGLU: |v| (|g| + |gelu(g)|)): what the fp32 evaluation of the activation on the exact sum h rounds against."""
    if act == ACT_GEGLU:
        v, g = h[:, 0::2], h[:, 1::2]
        return v.abs() * (g.abs() + lc.gelu64(g).abs())
    return h.abs() + act64(h, act).abs()


def act32_ratio(out, h, act, scale=1.0, residual=None):
    """Worst (|out - ref| [- 0.5 ulp32 with a residual]) / (2^-24 (|h| + |act(h)|) |scale|), ref = act(h) scale + residual, h the exact sum."""
    ref = act64(h, act) * scale + (residual.double() if residual is not None else 0.0)
    o = out.double()
    err = (o - ref).abs()
    if residual is not None:
        err = (err - 0.5 * _ulp(out, ref)).clamp_min(0.0)
    denom = 2.0 ** -24 * act_slack64(h, act) * abs(scale)
    ratio = torch.where(err > 0, err / denom.clamp_min(1e-300), torch.zeros_like(err))
    ratio = torch.where(torch.isfinite(o), ratio, torch.full_like(ratio, float("inf")))
    return float(ratio.max())


def act32_mismatches(out, h, act, c, scale=1.0, residual=None):
    ref = act64(h, act) * scale + (residual.double() if residual is not None else 0.0)
    o = out.double()
    bound = c * 2.0 ** -24 * act_slack64(h, act) * abs(scale) + (0.5 * _ulp(out, ref) if residual is not None else 0.0)
    bad = ~((o - ref).abs() <= bound)
    return int(bad.sum()), lc._where(bad)


def softmax_ref64(s, scale, causal=False, tq=1):
    """(ref, weight of the bound, hidden): float64 softmax(scale s) over the last dimension of s [rows, cols], keys > row % tq hidden when causal;
    weight = (1 + |scale s| + |scale s_max|) ref."""
    x = s.double() * scale
    rows, cols = x.shape
    if causal:
        hidden = torch.arange(cols, device=s.device)[None, :] > (torch.arange(rows, device=s.device) % tq)[:, None]
    else:
        hidden = torch.zeros_like(x, dtype=torch.bool)
    xm = x.masked_fill(hidden, float("-inf"))
    mx = xm.amax(-1, keepdim=True)
    ref = torch.softmax(xm, -1)
    weight = (1.0 + x.abs() + mx.abs()) * ref
    return ref, weight, hidden


def softmax_ratio(out, ref, weight, hidden):
    """Worst (|out - ref| - 2^-126) / (2^-24 weight) over the visible columns; inf when a hidden column is not +0.0 or an output is not finite."""
    o = out.double()
    excess = ((o - ref).abs() - F32_MIN_NORMAL).clamp_min(0.0)
    ratio = torch.where(excess > 0, excess / (2.0 ** -24 * weight).clamp_min(1e-300), torch.zeros_like(excess))
    bits = out.contiguous().view(torch.int32)
    ratio = torch.where(hidden, torch.where(bits == 0, 0.0, float("inf")).to(ratio.dtype), ratio)
    ratio = torch.where(torch.isfinite(o), ratio, torch.full_like(ratio, float("inf")))
    return float(ratio.max())


def softmax_mismatches(out, ref, weight, hidden, c):
    """(count, first positions): visible columns outside |out - ref| <= c 2^-24 weight + 2^-126, hidden columns that are not +0.0 bit for bit."""
    o = out.double()
    bits = out.contiguous().view(torch.int32)
    bad = torch.where(hidden, bits != 0, ~((o - ref).abs() <= c * 2.0 ** -24 * weight + F32_MIN_NORMAL))
    return int(bad.sum()), lc._where(bad)


def attn_budget32(q, k, v, scale, causal=False):
    """(ref, dev, eps32, wabs) for fp32 q, k, v [B, H, T, D]: attn_norm_check.attn_budget64's reference and spread, eps32 = 2^-24 (4 + 2 max_j sum_d
    |q_d k_jd| scale) [B, H, Tq, 1] and wabs = sum_j w_j |v_jd|."""
    ref, dev, _ = an.attn_budget64(q, k, v, scale, causal)
    w = an.attn_weights64(q, k, scale, causal)
    wabs = w @ v.double().abs()
    a = (q.double().abs() @ k.double().abs().transpose(-1, -2)) * scale
    if causal:
        a = a.masked_fill(an._mask(q.shape[-2], k.shape[-2], q.device), 0.0)
    eps = 2.0 ** -24 * (4.0 + 2.0 * a.amax(-1, keepdim=True))
    return ref, dev, eps, wabs


def _attn_unit(dev, eps, wabs, tk):
    return eps * dev + math.sqrt(tk) * 2.0 ** -24 * wabs


def attn32_ratio(out, ref, dev, eps, wabs, tk):
    o = out.double()
    excess = ((o - ref).abs() - 0.5 * _ulp(out, ref)).clamp_min(0.0)
    ratio = torch.where(excess > 0, excess / _attn_unit(dev, eps, wabs, tk).clamp_min(1e-300), torch.zeros_like(excess))
    ratio = torch.where(torch.isfinite(o), ratio, torch.full_like(ratio, float("inf")))
    return float(ratio.max())


def attn32_mismatches(out, ref, dev, eps, wabs, tk, c):
    o = out.double()
    bad = ~((o - ref).abs() <= 0.5 * _ulp(out, ref) + c * _attn_unit(dev, eps, wabs, tk))
    return int(bad.sum()), lc._where(bad)


def uniform32_mismatches(out, case, c):
    """A uniform case: rows whose key count is a power of two bit-exact, the others under the attention bound with constant c."""
    count = case["count"]
    pow2 = ((count & (count - 1)) == 0)[None, None, :, None]
    ref, dev, eps, wabs = case["budget"]
    o = out.double()
    exact_bad = out != case["ref"].to(torch.float32)
    bound_bad = ~((o - ref).abs() <= 0.5 * _ulp(out, ref) + c * _attn_unit(dev, eps, wabs, case["k"].shape[2]))
    bad = torch.where(pow2, exact_bad, bound_bad)
    return int(bad.sum()), lc._where(bad)


def old_metric(out, ref):
    """What tests/test_fp32_gpu.py asserts below 2e-5: one number per tensor, max |out - ref| / max |ref|."""
    return float((out.double() - ref.double()).abs().max() / ref.double().abs().max().clamp_min(1e-9))


# ------------------------------------------------------------------------------------------------------------------ contraction: references
def gemm_ref64(case):
    """(h, habs): the float64 pre-activation sum [A1 | A2] W^T + bias + rowbias[m // rows_per_batch] of a case and its magnitude sum."""
    a = case["a1"].double() if case.get("a2") is None else torch.cat([case["a1"].double(), case["a2"].double()], 1)
    w = case["w"].double()
    h, habs = a @ w.t(), a.abs() @ w.abs().t()
    if case.get("bias") is not None:
        h, habs = h + case["bias"].double(), habs + case["bias"].double().abs()
    if case.get("rowbias") is not None:
        idx = torch.arange(a.shape[0], device=a.device) // case["rpb"]
        rb = case["rowbias"].double()[idx]
        h, habs = h + rb, habs + rb.abs()
    return h, habs


def finish64(h, habs, case):
    """(ref, budget) behind the epilogue of a case: act -> scale -> residual."""
    act, scale = case.get("act", ACT_NONE), case.get("scale", 1.0)
    ref = act64(h, act) * scale
    if case.get("residual") is not None:
        ref = ref + case["residual"].double()
    return ref, act_abs64(h, habs, act) * abs(scale)


def conv_ref64(case):
    """(h, habs) of a conv case through launch_check.conv_taps64: x [B, H, W, Cin] fp32, w [Cout, 9 * Cin_w] in (ky, kx, ci) order (Cin_w >= Cin:
    pack_conv3x3 pads the channels with zeros, and x then carries Cin_w channels), per-image row bias."""
    x, w = case["x"].double(), case["w"].double()
    cin = x.shape[3]
    if case["ups"]:
        x = x.repeat_interleave(2, 1).repeat_interleave(2, 2)
    geo = conv_geo(case)
    taps = [(t // 3, t % 3, w[:, t * cin:(t + 1) * cin]) for t in range(9)]
    h = lc.conv_taps64(x, taps, geo)
    habs = lc.conv_taps64(x.abs(), [(dy, dx, wt.abs()) for dy, dx, wt in taps], geo)
    if case.get("bias") is not None:
        h, habs = h + case["bias"].double(), habs + case["bias"].double().abs()
    if case.get("rowbias") is not None:
        rb = case["rowbias"].double().repeat_interleave(geo["OH"] * geo["OW"], 0)
        h, habs = h + rb, habs + rb.abs()
    return h, habs


def conv_geo(case):
    b, hh, ww, _ = case["x"].shape
    ups, stride, pad_mode = int(case["ups"]), case["stride"], case["pad_mode"]
    pads = 2 if pad_mode == 0 else 1
    return {"stride": stride, "pt": 1 if pad_mode == 0 else 0, "OH": ((hh << ups) + pads - 3) // stride + 1, "OW": ((ww << ups) + pads - 3) // stride + 1}


def fma_chain32(a, w):
    """acc = fp32(acc + a[:, k] w[:, k]) for k = 0, 1, ...: the k-ascending fp32 FMA chain (module docstring: the double-rounding caveat)."""
    a64, w64 = a.double(), w.double()
    acc = torch.zeros((a.shape[0], w.shape[0]), dtype=torch.float32, device=a.device)
    for k in range(a.shape[1]):
        acc = (acc.double() + a64[:, k, None] * w64[None, :, k]).float()
    return acc


# ------------------------------------------------------------------------------------------------------------------ contraction: builders
def _ints(shape, r, gen):
    return torch.randint(-r, r + 1, shape, generator=gen, device=gen.device).to(torch.float32)


def gemm_case(M, N, K, gen, integer, K1=None, bias=False, rpb=0, residual=False, scale=1.0, act=ACT_NONE):
    """One GEMM problem.  Integer: A, W in {-2..2} (W in {-1..1} for GEGLU, as the launch table), bias / row bias in {-8..8}, residual in {-64..64},
    every sum |a||w| + |bias| + |rowbias| < 2^24 (asserted).  Real: A ~ N(0.25, 1), W ~ N(0.25, 1) / sqrt(K), bias / row bias / residual ~ N(0.25, 1)."""
    dev = gen.device
    K1 = K if K1 is None else K1
    if integer:
        assert scale in (1.0, 0.5, 2.0)
        a, w = _ints((M, K), 2, gen), _ints((N, K), 1 if act == ACT_GEGLU else 2, gen)
        vec = lambda shape, r: _ints(shape, r, gen)
    else:
        a = torch.randn((M, K), generator=gen, device=dev) + 0.25
        w = (torch.randn((N, K), generator=gen, device=dev) + 0.25) / math.sqrt(K)
        vec = lambda shape, r: torch.randn(shape, generator=gen, device=dev) + 0.25
    case = {"a1": a[:, :K1].contiguous(), "a2": a[:, K1:].contiguous() if K1 < K else None, "w": w, "M": M, "N": N, "K": K, "K1": K1,
            "bias": vec((N,), 8) if bias else None, "rowbias": vec(((M + rpb - 1) // rpb, N), 8) if rpb else None, "rpb": rpb,
            "residual": vec((M, N // 2 if act == ACT_GEGLU else N), 64) if residual else None, "scale": scale, "act": act, "integer": integer}
    if integer:
        _, habs = gemm_ref64(case)
        assert float(habs.max()) < 2.0 ** 24, "integer case: a partial sum could leave the exact fp32 range"
    return case


def conv_case(B, H, W, Cin, Cout, gen, integer, stride=1, pad_mode=0, ups=False, cin_w=None, bias=False, rowbias=False, residual=False, scale=1.0,
              act=ACT_NONE):
    """One conv problem: x [B, H, W, Cin], OIHW weights w4 [Cout, Cin, 3, 3] and their [Cout, 9 * Cin] (ky, kx, ci) matrix w."""
    dev = gen.device
    if integer:
        x, w4 = _ints((B, H, W, Cin), 2, gen), _ints((Cout, Cin, 3, 3), 2, gen)
        vec = lambda shape, r: _ints(shape, r, gen)
    else:
        x = torch.randn((B, H, W, Cin), generator=gen, device=dev) + 0.25
        w4 = (torch.randn((Cout, Cin, 3, 3), generator=gen, device=dev) + 0.25) / math.sqrt(9 * Cin)
        vec = lambda shape, r: torch.randn(shape, generator=gen, device=dev) + 0.25
    case = {"x": x, "w4": w4, "w": w4.permute(0, 2, 3, 1).reshape(Cout, 9 * Cin).contiguous(), "stride": stride, "pad_mode": pad_mode, "ups": ups,
            "scale": scale, "act": act, "integer": integer, "K": 9 * Cin}
    geo = conv_geo(case)
    m = B * geo["OH"] * geo["OW"]
    case.update(bias=vec((Cout,), 8) if bias else None, rowbias=vec((B, Cout), 8) if rowbias else None,
                residual=vec((m, Cout), 64) if residual else None, M=m, N=Cout)
    if integer:
        _, habs = conv_ref64(case)
        assert float(habs.max()) < 2.0 ** 24
    return case


# ------------------------------------------------------------------------------------------------------------------ attention: builders
def _losers_below(case):
    """The largest float64 softmax weight of a key that is not the row's winner."""
    w = an.attn_weights64(case["q"], case["k"], case["scale"], case["causal"])
    if w.shape[-1] == 1:
        return 0.0
    return float(w.scatter(3, case["pi"][..., None], 0.0).max())


def _f32(case):
    for name in ("q", "k", "v", "expect"):
        if name in case:
            case[name] = case[name].float()
    return case


def selector32(B, H, Tq, Tk, D, gen, scale=None):
    """attn_norm_check.selector_case with the gain doubled until every loser's float64 weight is below 2^-150 (g a power of two, keys +-1: every score is an
    integer multiple of g, exact in fp32)."""
    state = gen.get_state()
    for g in (16.0, 32.0, 64.0, 128.0, 256.0):
        gen.set_state(state)
        try:
            case = an.selector_case(B, H, Tq, Tk, D, g, gen, scale)
        except AssertionError:
            continue
        if _losers_below(case) < LOSER_MAX:
            assert float((case["q"].double().abs() @ case["k"].double().abs().transpose(-1, -2)).max()) < 2.0 ** 24
            return _f32(case)
    raise AssertionError(f"selector case d={D} Tk={Tk}: no gain up to 256 pushes the losers below 2^-150")


def ramp32(B, H, Tq, Tk, D, causal, device, scale=None, delta=0.5):
    """attn_norm_check.ramp_case with g the smallest power of two whose key step is at least 150 in the log2 domain."""
    sc = D ** -0.5 if scale is None else scale
    g = 2.0 ** math.ceil(math.log2(150.0 / (D * delta * sc * an.LOG2E)))
    case = an.ramp_case(B, H, Tq, Tk, D, causal, device, g=g, delta=delta, scale=scale)
    assert _losers_below(case) < LOSER_MAX and D * g * delta * (Tk - 1) < 2.0 ** 24, "ramp case: a loser survives in fp32, or a score is not exact"
    return _f32(case)


def uniform32(B, H, Tq, Tk, D, c, causal, device, scale=None):
    """attn_norm_check.uniform_case in fp32 with the attention budget of its rows (the rows whose count is no power of two go under the bound)."""
    case = an.uniform_case(B, H, Tq, Tk, D, c, causal, device, scale)
    for name in ("q", "k", "v"):
        case[name] = case[name].float()
    case["budget"] = attn_budget32(case["q"], case["k"], case["v"], case["scale"], causal)
    return case


def real32(B, H, Tq, Tk, D, peaky, causal, gen, scale=None):
    """attn_norm_check.real_case drawn in fp32 (the same distributions, not rounded to f16)."""
    dev = gen.device
    scale = D ** -0.5 if scale is None else scale
    m = 3.0 if peaky else 1.0
    q = torch.randn((B, H, Tq, D), generator=gen, device=dev) * m
    k = torch.randn((B, H, Tk, D), generator=gen, device=dev) * m
    v = torch.randn((B, H, Tk, D), generator=gen, device=dev) + 0.25
    if Tk > 2:
        k[:, :, (Tk * 3) // 5] = q[:, :, min(5, Tq - 1)] * (4.0 / m)
    return {"q": q, "k": k, "v": v, "scale": scale, "causal": causal}


# ------------------------------------------------------------------------------------------------------------------ defect models
GEMM_DEFECTS = ["k_tail_dropped", "concat_seam", "rowbias_div", "geglu_swap", "geglu_last_pair_lost", "geglu_pair_past_n", "kn_group_transposed",
                "operands_tf32", "operands_bf16", "acc_f16"]
CONV_DEFECTS = ["tap_padded_cin", "k_tail_dropped", "operands_tf32"]
SOFTMAX_DEFECTS = ["causal_limit"]
ATTN_DEFECTS = ["causal_limit", "stride_z2_from_z1", "kn_group_transposed", "k_tail_dropped", "operands_tf32", "operands_bf16", "acc_f16"]
PREFILL = -4321.0                    # what the models (and the GPU test) put into an output before the op runs


def round_mantissa(x, bits):
    """fp32 tensor rounded (RNE) to `bits` explicit mantissa bits: 10 = TF32-like, 7 = bf16."""
    drop = 23 - bits
    i = x.contiguous().view(torch.int32).to(torch.int64)
    i = (i + ((1 << (drop - 1)) - 1) + ((i >> drop) & 1)) >> drop << drop
    return i.to(torch.int32).view(torch.float32)


def _contract(a, w, defect):
    """[M, K] x [N, K]^T in float64 (the caller rounds once), with the operand / accumulator defects."""
    if defect == "operands_tf32":
        a, w = round_mantissa(a.float(), 10), round_mantissa(w.float(), 10)
    if defect == "operands_bf16":
        a, w = round_mantissa(a.float(), 7), round_mantissa(w.float(), 7)
    if defect == "acc_f16":
        a, w = a.float(), w.float()
        acc = torch.zeros((a.shape[0], w.shape[0]), dtype=torch.float16, device=a.device)
        for k in range(a.shape[1]):
            acc = (acc.float() + a[:, k, None] * w[None, :, k]).to(torch.float16)
        return acc.double()
    return a.double() @ w.double().t()


def _kn_transpose(w):
    """The [K][N] staging of csrc/f32.hip with the LDS slot kr * 4 + i in place of kr + 4 i: inside every 16-step, k-slot s holds W[k = s / 4 + 4 (s % 4)]."""
    n, k = w.shape
    kp = (k + KSTEP - 1) // KSTEP * KSTEP
    wp = torch.zeros((n, kp), dtype=w.dtype, device=w.device)
    wp[:, :k] = w
    s = torch.arange(KSTEP, device=w.device)
    src = (s // 4 + 4 * (s % 4))[None, :] + torch.arange(0, kp, KSTEP, device=w.device)[:, None]
    return wp[:, src.reshape(-1)][:, :k]


def _drop_tail(k):
    return k // KSTEP * KSTEP if k % KSTEP else k


def gemm_model(case, defect=None, w_kn=False):
    """What fie_gemm_f32 would store for a gemm_case: the [M, Nout + 1] output buffer (one padding column behind the rows, prefilled with PREFILL)
    with one defect built in.  w_kn: the weights reach the kernel as [K][N] (the result is the same; the kn staging defect applies)."""
    a1, a2, w = case["a1"], case.get("a2"), case["w"]
    M, N, K, K1 = case["M"], case["N"], case["K"], case["K1"]
    a = a1 if a2 is None else torch.cat([a1, a2], 1)
    if defect == "concat_seam" and a2 is not None:            # `k < K1 - 1 ? A1 : A2`: column K1 - 1 comes from A2's first column
        a = a.clone()
        a[:, K1 - 1] = a2[:, 0]
    if defect == "kn_group_transposed" and w_kn:
        w = _kn_transpose(w)
    if defect == "k_tail_dropped":
        a, w = a[:, :_drop_tail(K)], w[:, :_drop_tail(K)]
    h = _contract(a, w, defect)
    if case.get("bias") is not None:
        h = h + case["bias"].double()
    if case.get("rowbias") is not None:
        rpb = case["rpb"] + 1 if defect == "rowbias_div" else case["rpb"]
        h = h + case["rowbias"].double()[torch.arange(M, device=a.device) // rpb]
    act, scale = case.get("act", ACT_NONE), case.get("scale", 1.0)
    if act == ACT_GEGLU and defect == "geglu_swap":
        y = h[:, 1::2] * lc.gelu64(h[:, 0::2])
    else:
        y = act64(h, act)
    y = y * scale
    if case.get("residual") is not None:
        y = y + case["residual"].double()
    nout = y.shape[1]
    buf = torch.full((M, nout + 1), PREFILL, dtype=torch.float32, device=a.device)
    buf[:, :nout] = y.float()
    if act == ACT_GEGLU and defect == "geglu_last_pair_lost":           # `n + r + 2 < N`: the pair that ends at N is never stored
        buf[:, nout - 1] = PREFILL
    if act == ACT_GEGLU and defect == "geglu_pair_past_n":              # `n + r < N + 1`: one pair past N is stored (0 * gelu(0) from the zero-filled tile)
        buf[:, nout] = 0.0
    return buf


def im2col(case, cin_decode=None):
    """The [M, 9 * Cin] matrix the kernel's gather builds: k -> (tap, ci) decoded with `cin_decode` (the true Cin when None), the pixel address
    ((b H + ih) W + iw) Cin + ci taken in the flat tensor as the kernel takes it."""
    x = case["x"]
    B, H, W, Cin = x.shape
    geo = conv_geo(case)
    ups, s, pt, OH, OW = int(case["ups"]), geo["stride"], geo["pt"], geo["OH"], geo["OW"]
    cd = cin_decode or Cin
    dev = x.device
    m = torch.arange(B * OH * OW, device=dev)
    b, oh, ow = m // (OH * OW), (m // OW) % OH, m % OW
    k = torch.arange(9 * Cin, device=dev)
    tap = k // cd
    ci, ky, kx = k - tap * cd, tap // 3, tap % 3
    ih = (oh * s - pt)[:, None] + ky[None, :]
    iw = (ow * s - pt)[:, None] + kx[None, :]
    inside = (ih >= 0) & (ih < (H << ups)) & (iw >= 0) & (iw < (W << ups))
    idx = ((b[:, None] * H + (ih >> ups)) * W + (iw >> ups)) * Cin + ci[None, :]
    flat = x.reshape(-1)
    vals = flat[idx.clamp(0, flat.numel() - 1)]
    return torch.where(inside, vals, torch.zeros_like(vals))


def conv_model(case, defect=None):
    """What fie_conv3x3_nhwc_f32 would store for a conv_case ([M, Cout + 1] as gemm_model)."""
    cin = case["x"].shape[3]
    a = im2col(case, (cin + 7) // 8 * 8 if defect == "tap_padded_cin" else None)
    geo = conv_geo(case)
    g = dict(case, a1=a, a2=None, K1=case["K"], rpb=geo["OH"] * geo["OW"] if case.get("rowbias") is not None else 0)
    return gemm_model(g, defect)


def softmax_model(s, scale, causal=False, tq=1, defect=None, keep64=False):
    """What fie_softmax_rows_f32 leaves in s [rows, cols]; causal_limit: lim = row % tq instead of row % tq + 1 (a row with lim = 0 stores zeros)."""
    x = s.double() * scale
    rows, cols = x.shape
    lim = torch.full((rows,), cols, device=s.device)
    if causal:
        q = torch.arange(rows, device=s.device) % tq
        lim = torch.clamp(q if defect == "causal_limit" else q + 1, max=cols)
    hidden = torch.arange(cols, device=s.device)[None, :] >= lim[:, None]
    out = torch.softmax(x.masked_fill(hidden, float("-inf")), -1)
    out = torch.where(hidden, torch.zeros_like(out), out).nan_to_num(0.0)
    return out if keep64 else out.float()


def attn32_model(q, k, v, scale, causal=False, defect=None):
    """The composition hip.Context.attention runs in an fp32 context, [B, H, T, D] fp32 tensors: S = Q K^T (fie_gemm_f32 batched over (image, head)),
    the row softmax, O = P V with V as a [K][N] matrix.  stride_z2_from_z1: the head offset z2 * sA2 taken with the image stride sA1 -- head (b, h)
    reads the Q rows of image b + h, head 0 (wrapped into the tensor: the model stays inside its allocation)."""
    B, H, Tq, D = q.shape
    Tk = k.shape[2]
    if defect == "stride_z2_from_z1":
        bb = (torch.arange(B, device=q.device)[:, None] + torch.arange(H, device=q.device)[None, :]) % B
        q = q[bb, 0]
    out = torch.empty((B, H, Tq, D), dtype=torch.float32, device=q.device)
    for b in range(B):
        for h in range(H):
            s = _contract(q[b, h], k[b, h], defect if defect in ("operands_tf32", "operands_bf16", "acc_f16") else None)
            p = softmax_model(s, scale, causal, Tq, defect, keep64=True)
            vt = v[b, h].t().contiguous()                                  # [N = D][K = Tk]
            if defect == "kn_group_transposed":
                vt = _kn_transpose(vt)
            if defect == "k_tail_dropped":
                p, vt = p[:, :_drop_tail(Tk)], vt[:, :_drop_tail(Tk)]
            out[b, h] = _contract(p, vt.to(p.dtype), defect if defect in ("operands_tf32", "operands_bf16", "acc_f16") else None)
    return out
