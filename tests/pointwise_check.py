"""Float64 references, per-element bounds, input builders and defect models of tests/test_pointwise_gpu.py (device-agnostic torch; the CPU
self-check in tests/test_pointwise_check_cpu.py runs them on fp32 emulations of the kernels of csrc/pointwise.hip and csrc/lcm.hip).

Every reference is float64 on the STORED inputs (the f16 / fp32 tensors, the scalars as the fp32 values the ABI receives).  The budget A of
an expression is the same expression with every term replaced by its absolute value; an fp32 result must lie within n 2^-24 A of the
reference, n the number of roundings of the expression as written (fused multiply-adds only lower it); an f16 output adds half an f16 ulp.
Nothing is normalised by a tensor's maximum.  Every checker returns (count, first positions, worst ratio): the ratio is
(|out - ref| - 0.5 ulp16 for f16) / (2^-24 A) and is compared with n, or |out - ref| / bound where the bound has another form.

  lcm_step      n = 8      latent_prep   n = 7      (counts beside the expressions below)
  sinusoid      |arg| (u + 1.5) 2^-23 + 2^-22, u = ln(1e4) f / half
  time_embed    layer 2 on the kernel's own hidden vector, layer 1 on the float64 sinusoid: 1.13 (K / 4 + 3) 2^-24 sum |W||v| + 2^-18
  pixels_in     f16: the float64 value rounded once; fp32: two roundings
  pixels_out    the exact byte (what decides it: pixels_out_expect)
  clip_embed, add, amax     exact
"""
import math

import torch

import launch_check as lc
from attn_norm_check import to_f16_rne

U24 = 2.0 ** -24                    # one fp32 rounding, relative
FLOOR_ACT = 2.0 ** -18              # the floor under an fp32 activation (the constant of tests/test_launch_table_gpu.py), absolute here: the sums are O(1)
LN1E4 = math.log(10000.0)
TIMESTEPS = (0.0, 0.5, 1.0, 19.0, 259.0, 499.0, 759.0, 999.0, 1024.0)
HW_SIZES = (1, 255, 1000, 2048 * 256 + 300)        # the last: the only size at which the grid-stride loop (2048 blocks of 256) repeats
KAT_499 = ((0, (-0.87116218, 0.98838931, 0.19755381)), (160, (0.49099535, -0.15194249, -0.98029202)))      # t = 499, dim 320: [cos | sin]


def f32v(v):
    """The fp32 value a C float argument receives, as a Python float."""
    return float(torch.tensor(float(v), dtype=torch.float32))


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _randn(shape, gen, device):
    return torch.randn(shape, generator=gen).to(device)


# ------------------------------------------------------------------------------------------------------------------ the checkers
def budget_check(out, ref, unit, n, f16):
    """Elements outside |out - ref| <= n unit (+ 0.5 max(ulp16(ref), ulp16(out)) for an f16 output): (count, first positions, worst ratio),
    ratio = (|out - ref| - the f16 half ulp) / unit; an output that is not finite counts as infinitely far."""
    o = out.double()
    err = (o - ref).abs()
    half = 0.5 * torch.maximum(lc.ulp16(ref), lc.ulp16(o)) if f16 else torch.zeros_like(err)
    bad = ~(err <= n * unit + half)
    excess = (err - half).clamp_min(0.0)
    ratio = torch.where(excess > 0, excess / unit.clamp_min(1e-300), torch.zeros_like(excess))
    ratio = torch.where(torch.isfinite(o), ratio, torch.full_like(ratio, float("inf")))
    return int(bad.sum()), lc._where(bad), float(ratio.max())


def bound_check(out, ref, bound):
    """Elements outside |out - ref| <= bound: (count, first positions, worst |out - ref| / bound)."""
    o = out.double()
    err = (o - ref).abs()
    bad = ~(err <= bound)
    ratio = torch.where(err > 0, err / bound.clamp_min(1e-300), torch.zeros_like(err))
    ratio = torch.where(torch.isfinite(o), ratio, torch.full_like(ratio, float("inf")))
    return int(bad.sum()), lc._where(bad), float(ratio.max())


def exact_check(out, expect):
    """Elements that differ from `expect` (+0 == -0; NaN == NaN): (count, first positions, 0.0 or inf)."""
    bad = out != expect
    if out.is_floating_point():
        bad = bad & ~(torch.isnan(out) & torch.isnan(expect))
    n = int(bad.sum())
    return n, lc._where(bad), float("inf") if n else 0.0


def zero_check(t):
    """Elements of a padding column that are not exactly zero (a NaN is not zero)."""
    bad = ~(t == 0)
    n = int(bad.sum())
    return n, lc._where(bad), float("inf") if n else 0.0


def copy_check(dst, lat, scale, f16):
    """model_in / decode_in (first four columns) against the kernel's OWN fp32 latents: dst = T(lat * scale).  scale == 1 is a conversion:
    half an f16 ulp, nothing in fp32.  Otherwise one fp32 rounding of the product on top (n = 1)."""
    ref = lat.double() * scale
    return budget_check(dst, ref, U24 * ref.abs(), 0 if scale == 1.0 else 1, f16)


# ------------------------------------------------------------------------------------------------------------------ lcm_step
LCM_N = 8
LCM_DEFECTS = ["c_skip_dropped", "guidance_swapped", "renoise_on_last", "f16_arithmetic", "divide_by_prev"]


def lcm_scalar_sets():
    """name -> scalars: the schedule's own first (t = 999) and last (t = 19) step of a 50-step plan (fie_amd/lcm.py), and a synthetic set in
    which every term carries weight.  Values are the fp32 the ABI receives."""
    from fie_amd.lcm import LCMSchedule
    steps = LCMSchedule().plan(50, 1.0)
    first, last = steps[0], steps[-1]
    assert first["t"] == 999 and last["t"] == 19 and last["last"]
    sets = {}
    for name, s, g in (("t999", first, 1.5), ("t19", last, 8.0)):
        sets[name] = dict(guidance=g, sab_t=s["sqrt_ab"], s1mab_t=s["sqrt_1mab"], c_skip=s["c_skip"], c_out=s["c_out"],
                          sab_p=s["sqrt_ab_prev"], s1mab_p=s["sqrt_1mab_prev"], inv_sf=1.0 / 0.13025)
    sets["synthetic"] = dict(guidance=7.5, sab_t=0.07, s1mab_t=math.sqrt(1.0 - 0.07 ** 2), c_skip=0.3, c_out=0.9, sab_p=0.6, s1mab_p=0.8, inv_sf=1.0 / 0.18215)
    return {k: {n: f32v(v) for n, v in s.items()} for k, s in sets.items()}


def lcm_case(hw, ld_eps, nb, use_noise, scal, seed, device, dtype=torch.float16):
    """eps [nb, hw, ld_eps] in the storage type (N(0, 1); the unused columns hold NaN), latents f32 [hw, 4] = 3 N(0, 1), noise f32 [4, hw]."""
    g = _gen(seed)
    eps = torch.full((nb, hw, ld_eps), float("nan"), dtype=dtype, device=device)
    eps[..., :4] = _randn((nb, hw, 4), g, device).to(dtype)
    return {"hw": hw, "nb": nb, "eps": eps, "lat": 3.0 * _randn((hw, 4), g, device), "noise": _randn((4, hw), g, device), "use_noise": use_noise,
            "scal": scal, "dtype": dtype}


def lcm_ref64(case):
    """(ref, A) of the updated latents [hw, 4].  Roundings of the kernel's expression, which csrc/lcm.hip: lcm_update writes out operation by
    operation:
         e   = e0 + g (e1 - e0)                  2   (the difference, then one fused multiply-add)
         x0  = (x - s e) / sab_t                 1 + 1   (fused multiply-subtract; the divide)
         den = c_out x0 + c_skip x               2   (one product, one fused multiply-add)
         den = sab_p den + s1mab_p z             3   (two rounded products, then the add: nothing fused)
    Nine in all with guidance and noise.  LCM_N stays at the 8 the kernel has been held to: the worst ratio measured is 4.74."""
    s = case["scal"]
    e0 = case["eps"][0, :, :4].double()
    x = case["lat"].double()
    if case["nb"] == 2:
        e1 = case["eps"][1, :, :4].double()
        e = e0 + s["guidance"] * (e1 - e0)
        ea = e0.abs() + abs(s["guidance"]) * (e1.abs() + e0.abs())
    else:
        e, ea = e0, e0.abs()
    x0 = (x - s["s1mab_t"] * e) / s["sab_t"]
    x0a = (x.abs() + abs(s["s1mab_t"]) * ea) / abs(s["sab_t"])
    den = s["c_out"] * x0 + s["c_skip"] * x
    a = abs(s["c_out"]) * x0a + abs(s["c_skip"]) * x.abs()
    if case["use_noise"]:
        z = case["noise"].double().t()
        den = s["sab_p"] * den + s["s1mab_p"] * z
        a = abs(s["sab_p"]) * a + abs(s["s1mab_p"]) * z.abs()
    return den, a


def lcm_emulate(case, defect=None):
    """The kernel in torch fp32, one rounding per operation (no fused multiply-add); returns (latents f32, model_in row, decode_in row), the
    rows [hw, 4] in the storage type."""
    s = case["scal"]
    f16 = defect == "f16_arithmetic"
    wt = torch.float16 if f16 else torch.float32
    c = lambda v: torch.tensor(v, dtype=wt, device=case["lat"].device)
    e0 = case["eps"][0, :, :4].to(wt)
    x = case["lat"].to(wt)
    e = e0
    if case["nb"] == 2:
        e1 = case["eps"][1, :, :4].to(wt)
        e = e1 + c(s["guidance"]) * (e0 - e1) if defect == "guidance_swapped" else e0 + c(s["guidance"]) * (e1 - e0)
    x0 = (x - c(s["s1mab_t"]) * e) / c(s["sab_p"] if defect == "divide_by_prev" else s["sab_t"])
    den = c(s["c_out"]) * x0
    if defect != "c_skip_dropped":
        den = den + c(s["c_skip"]) * x
    if case["use_noise"] or defect == "renoise_on_last":
        den = c(s["sab_p"]) * den + c(s["s1mab_p"]) * case["noise"].t().to(wt)
    lat = den.float()
    return lat, lat.to(case["dtype"]), (lat * torch.tensor(s["inv_sf"], dtype=torch.float32, device=lat.device)).to(case["dtype"])


def lcm_check(lat, case, ref=None):
    ref, a = ref or lcm_ref64(case)
    return budget_check(lat, ref, U24 * a, LCM_N, False)


# ------------------------------------------------------------------------------------------------------------------ latent_prep
PREP_N = 7
PREP_DEFECTS = ["no_clamp", "noise_hw4", "exp_logvar", "expf_residue_twice"]
LOGVAR_PLANTED = (-40.0, -30.5, -30.0, 0.0, 20.0, 20.5, 25.0)


def prep_case(hw, seed, device, dtype=torch.float16, sf=0.13025, sab=0.5269, s1mab=0.8499):
    """moments [hw, 8] in the storage type: mean N(0, 1), logvar 8 N(0, 1) with LOGVAR_PLANTED cycling through the first and the last 7 rows
    of every channel (both sides of both clamp limits); in the first block mean and noise are 0, so that exp(logvar / 2) eps is the whole
    result and the lower limit shows too.  eps_post f32 [4, hw]; noise f32 [4, hw], plane c offset by 10 c: a [hw, 4] reading of the planar
    layout moves whole elements."""
    g = _gen(seed)
    mom = _randn((hw, 8), g, device)
    mom[:, 4:] *= 8.0
    eps = _randn((4, hw), g, device)
    noise = _randn((4, hw), g, device) + 10.0 * torch.arange(4, device=device, dtype=torch.float32)[:, None]
    planted = torch.tensor(LOGVAR_PLANTED, device=device)
    n = min(hw, 7)
    r = torch.arange(n, device=device)[:, None]
    ch = torch.arange(4, device=device)[None, :]
    mom[hw - n:, 4:] = planted[(r + ch + 4) % 7]
    mom[:n, 4:] = planted[(r + ch) % 7]
    mom[:n, :4] = 0.0
    noise[:, :n] = 0.0
    mom = mom.to(dtype)
    assert set(float(v) for v in mom[:n, 4:].flatten()) <= set(LOGVAR_PLANTED)          # the planted values are exact in f16
    return {"hw": hw, "mom": mom, "eps": eps, "noise": noise, "sf": f32v(sf), "sab": f32v(sab), "s1mab": f32v(s1mab), "dtype": dtype}


def prep_ref64(case):
    """(ref, A) of the initial latents [hw, 4].  Roundings (latent_prep_kernel), n = 7:
         s  = expf(0.5 clamp(logvar))            1   (the halving is exact; expf counted as one rounding: fie_expf measures well inside it, the compiler's expf did not)
         z0 = (m + s eps) sf                     1 + 1 + 1   (product, sum, scale; 1 + 1 when the sum fuses)
         x  = sab z0 + s1mab noise               3   (2 when fused)"""
    m = case["mom"][:, :4].double()
    lv = case["mom"][:, 4:].double().clamp(-30.0, 20.0)
    sd = torch.exp(0.5 * lv)
    e, z = case["eps"].double().t(), case["noise"].double().t()
    ref = case["sab"] * ((m + sd * e) * case["sf"]) + case["s1mab"] * z
    a = abs(case["sab"]) * ((m.abs() + sd * e.abs()) * abs(case["sf"])) + abs(case["s1mab"]) * z.abs()
    return ref, a


def expf_residue_twice(x):
    """What the kernel computed before csrc/fie_internal.h: fie_expf: the compiler's expansion of expf with `x c - E` contracted into one fused
    multiply-add, which holds the residue pl of the product x c, and pl added once more (fp32 tensor in and out; fma through float64)."""
    c = torch.tensor(0x3fb8aa3b, dtype=torch.int32, device=x.device).view(torch.float32)
    cc = torch.tensor(0x32a5705f, dtype=torch.int32, device=x.device).view(torch.float32)
    fma = lambda p, q, r: (p.double() * q.double() + r.double()).float()
    ph = x * c
    pl = fma(x, cc, fma(x, c, -ph))
    e = torch.round(ph)
    a = fma(x, c, -e) + pl
    return torch.ldexp(torch.exp2(a.double()).float(), e.to(torch.int32))


def prep_emulate(case, defect=None):
    """latent_prep_kernel in torch fp32; returns (latents f32 [hw, 4], model_in row in the storage type)."""
    dev = case["eps"].device
    c = lambda v: torch.tensor(v, dtype=torch.float32, device=dev)
    m = case["mom"][:, :4].float()
    lv = case["mom"][:, 4:].float()
    if defect != "no_clamp":
        lv = lv.clamp(-30.0, 20.0)
    sd = expf_residue_twice(c(0.5) * lv) if defect == "expf_residue_twice" else torch.exp(lv if defect == "exp_logvar" else c(0.5) * lv)
    noise = case["noise"].reshape(case["hw"], 4) if defect == "noise_hw4" else case["noise"].t()
    z0 = (m + sd * case["eps"].t()) * c(case["sf"])
    lat = c(case["sab"]) * z0 + c(case["s1mab"]) * noise
    return lat, lat.to(case["dtype"])


def prep_check(lat, case, ref=None):
    ref, a = ref or prep_ref64(case)
    return budget_check(lat, ref, U24 * a, PREP_N, False)


# ------------------------------------------------------------------------------------------------------------------ sinusoid
SIN_SHAPES = [(2, 1, 320, 0, 320), (2, 6, 256, 1280, 2816), (1, 1, 64, 0, 64), (3, 2, 2, 0, 4)]          # (B, nvals, dim, col0, ld)
SIN_DEFECTS = ["sin_cos_order", "half_minus_one"]


def sin_vals(b, nvals, device, shift=0):
    """f32 [b, nvals] cycling through TIMESTEPS."""
    i = (torch.arange(b * nvals) + shift) % len(TIMESTEPS)
    return torch.tensor(TIMESTEPS, dtype=torch.float32)[i].view(b, nvals).to(device)


def sin_ref64(vals, dim):
    """(ref, delta) [B, nvals, dim] = [cos | sin] of t exp(-ln(1e4) f / half) in float64, and the fp32 bound of one element:
         delta = |arg| (u + 1.5) 2^-23 + 2^-22,   u = ln(1e4) f / half
    two roundings of the exponent's argument (u 2^-24 each) and expf's ulp (2^-23) move the frequency by (u + 1) 2^-23 relative, the product
    t * freq adds 2^-24: |arg| (u + 1.5) 2^-23 in the angle, which cos / sin pass on with slope <= 1; the trig call itself 2^-22."""
    half = dim // 2
    f = torch.arange(half, device=vals.device, dtype=torch.float64)
    u = LN1E4 * f / half
    arg = vals.double()[..., None] * torch.exp(-u)
    ref = torch.cat([torch.cos(arg), torch.sin(arg)], -1)
    d = arg.abs() * (u + 1.5) * 2.0 ** -23 + 2.0 ** -22
    return ref, torch.cat([d, d], -1)


def sin_emulate(vals, dim, dtype, defect=None):
    """sinusoid_kernel in torch fp32: [B, nvals, dim] in the storage type."""
    half = dim // 2
    f = torch.arange(half, device=vals.device, dtype=torch.float32)
    den = torch.tensor(float(half - 1 if defect == "half_minus_one" else half), dtype=torch.float32, device=vals.device)
    freq = torch.exp(torch.tensor(-9.210340371976184, dtype=torch.float32, device=vals.device) * f / den)
    arg = vals[..., None] * freq
    parts = [torch.sin(arg), torch.cos(arg)] if defect == "sin_cos_order" else [torch.cos(arg), torch.sin(arg)]
    return torch.cat(parts, -1).to(dtype)


def sin_check(out, ref, delta, f16):
    """|out - ref| <= delta (+ 0.5 ulp16); the ratio is in units of delta."""
    return budget_check(out, ref, delta, 1, f16)


# ------------------------------------------------------------------------------------------------------------------ time_embed
TE_SHAPES = [(32, 64), (64, 256), (320, 1280)]          # (C0, E); the first runs ONE workgroup: no partner at the barrier
TE_DEFECTS = ["no_add", "quarter_skipped", "batch_swapped"]


def te_case(c0, e, b, add, seed, device, t_shift=0):
    """t f32 [b] from TIMESTEPS; W1 [e, c0], W2 [e, e] f16 scaled to unit output variance, biases 0.1 N(0, 1); add [b, e + 24] (a row stride
    larger than e) or None."""
    g = _gen(seed)
    case = {"b": b, "c0": c0, "e": e, "t": sin_vals(b, 1, device, t_shift).view(b),
            "w1": (_randn((e, c0), g, device) * c0 ** -0.5).half(), "b1": (_randn((e,), g, device) * 0.1).half(),
            "w2": (_randn((e, e), g, device) * e ** -0.5).half(), "b2": (_randn((e,), g, device) * 0.1).half(), "add": None}
    if add:
        buf = torch.full((b, e + 24), float("nan"), dtype=torch.float16, device=device)
        buf[:, :e] = _randn((b, e), g, device).half()
        case["add"] = buf[:, :e]
    return case


def te_structural_case(c0, e, b, device):
    """Every sum an exact small integer: t = 0, so x = [1 .. 1 | 0 .. 0] exactly; W1[n] holds one integer of {-2 .. 2} per K quarter, which
    depends on n and on the quarter (the two sine quarters meet x = 0), b1 in {-2 .. 2}; W2 = one-hot rows through a permutation, b2 = add = 0:
    hbuf[b, n] = f16(silu(w(n, 0) + w(n, 1) + b1[n])) and out[b, n] = f16(silu(hbuf[b, perm(n)])).  Returns the case with 'pre' (the
    integer pre-activations [e]) and 'perm'."""
    n = torch.arange(e, device=device)
    kq = c0 // 4
    w1 = torch.zeros((e, c0), dtype=torch.float16, device=device)
    pre = torch.zeros(e, dtype=torch.float64, device=device)
    for q in range(4):
        wq = ((n * 3 + 2 * q) % 5 - 2).double()
        w1[n, q * kq + (5 * n + q) % kq] = wq.half()
        if q < 2:
            pre += wq
    b1 = ((n * 7 + 1) % 5 - 2).double()
    perm = (n * 77 + 13) % e                               # 77 is odd and no multiple of 5: a permutation of every e = 2^k or 5 * 2^k
    assert len(set(perm.tolist())) == e
    w2 = torch.zeros((e, e), dtype=torch.float16, device=device)
    w2[n, perm] = 1.0
    return {"b": b, "c0": c0, "e": e, "t": torch.zeros(b, dtype=torch.float32, device=device), "w1": w1, "b1": b1.half(), "w2": w2,
            "b2": torch.zeros(e, dtype=torch.float16, device=device), "add": None, "pre": pre + b1, "perm": perm}


def _silu64(x):
    return lc.act64(x, 1)


def te_layer1_check(hbuf, case):
    """The hidden vector [b, e] (f16) against float64 silu(W1 x + b1), x the float64 sinusoid:
         0.5 ulp16 + 1.13 (C0 / 4 + 3) 2^-24 (sum |W1||x| + |b1|) + FLOOR_ACT + 1.13 sum_k |W1[n, k]| (0.5 ulp16(x_k) + delta_k)
    C0 / 4 + 3: one thread's chain of fused multiply-adds, two shuffle adds, the bias; the last term: the kernel rounds its sinusoid to f16
    (within delta_k of the float64 one: sin_ref64)."""
    x, delta = sin_ref64(case["t"].view(-1, 1), case["c0"])
    x, delta = x[:, 0], delta[:, 0]
    w, bias = case["w1"].double(), case["b1"].double()
    pre = x @ w.t() + bias
    a = x.abs() @ w.abs().t() + bias.abs()
    xin = (0.5 * lc.ulp16(x) + delta) @ w.abs().t()
    bound = lc.act_abs64(pre, (case["c0"] / 4 + 3) * U24 * a + xin, 1) + FLOOR_ACT            # act_abs64: |SiLU'| <= 1.13
    return budget_check(hbuf, _silu64(pre), bound, 1, True)            # the ratio: what exceeds the f16 half ulp, in units of the rest


def te_layer2_check(out, hbuf, case):
    """out [b, e] (f16) against float64 silu(W2 hbuf + b2 + add) on the kernel's OWN hbuf (layer 1's uncertainty does not enter):
         0.5 ulp16 + 1.13 (E / 4 + 3) 2^-24 (sum |W2||hbuf| + |b2| + |add|) + FLOOR_ACT"""
    h = hbuf.double()
    w, bias = case["w2"].double(), case["b2"].double()
    pre = h @ w.t() + bias
    a = h.abs() @ w.abs().t() + bias.abs()
    if case["add"] is not None:
        pre, a = pre + case["add"].double(), a + case["add"].double().abs()
    return budget_check(out, _silu64(pre), lc.act_abs64(pre, (case["e"] / 4 + 3) * U24 * a, 1) + FLOOR_ACT, 1, True)


def te_structural_check(out, hbuf, case):
    """Both layers of te_structural_case within 1 ulp16 of the one valid answer (the fp32 SiLU rounds before the f16 store): returns the two
    (count, first positions, worst ratio in ulp16)."""
    res = []
    h_ref = _silu64(case["pre"])[None, :].expand(case["b"], -1)
    o_ref = _silu64(hbuf.double()[:, case["perm"]])
    for got, ref in ((hbuf, h_ref), (out, o_ref)):
        res.append(bound_check(got, ref, torch.maximum(lc.ulp16(ref), lc.ulp16(got.double()))))
    return res


def _quarter_dot32(w, v, skip=None):
    """[b, n] = the four K quarters of sum_k w[n, k] v[b, k] in fp32, met as the two shuffles meet them: (q0 + q1) + (q2 + q3)."""
    kq = w.shape[1] // 4
    q = [torch.zeros((v.shape[0], w.shape[0]), dtype=torch.float32, device=w.device) if i == skip else
         v[:, i * kq:(i + 1) * kq].float() @ w[:, i * kq:(i + 1) * kq].float().t() for i in range(4)]
    return (q[0] + q[1]) + (q[2] + q[3])


def _silu32(x):
    return x / (1.0 + torch.exp(-x))


def te_emulate(case, defect=None):
    """time_embed_kernel in torch fp32: (out [b, e], hbuf [b, e]), both f16."""
    x = sin_emulate(case["t"].view(-1, 1), case["c0"], torch.float16)[:, 0]
    hbuf = _silu32(_quarter_dot32(case["w1"], x) + case["b1"].float()).half()
    pre = _quarter_dot32(case["w2"], hbuf, skip=1 if defect == "quarter_skipped" else None) + case["b2"].float()
    if case["add"] is not None and defect != "no_add":
        pre = pre + case["add"].float()
    out = _silu32(pre).half()
    if defect == "batch_swapped" and case["b"] > 1:
        out = out[torch.arange(case["b"], device=out.device) ^ 1 if case["b"] % 2 == 0 else torch.roll(torch.arange(case["b"], device=out.device), 1)]
    return out, hbuf


# ------------------------------------------------------------------------------------------------------------------ pixels
PIX_SIZES = [(1, 1), (16, 16), (769, 683)]             # 769 x 683 = 525 227 pixels > 2048 * 256: the grid-stride loop repeats
PIX_DEFECTS = ["in_over_256", "out_truncates", "out_half_away"]
TIE_BAND = 2.0 ** -15       # fp32 only: within this of k + 0.5 the two fp32 roundings of the expression decide the byte (2 * 2^-24 * 255 = 3.04e-5 < 2^-15)


def pix_image(h, w, device):
    """u8 [h, w, 3]: pixel i = y w + x holds (i + 85 c) % 256 in channel c."""
    i = torch.arange(h * w, device=device)[:, None]
    c = torch.arange(3, device=device)[None, :]
    return ((i + 85 * c) % 256).to(torch.uint8).view(h, w, 3)


def pix_all_values(device):
    """Three u8 [16, 16, 3] images: image c holds all 256 values in channel c (and shifted copies in the others)."""
    i = torch.arange(256, device=device)
    imgs = []
    for c in range(3):
        img = torch.stack([i if k == c else (3 * i + 7 * k + 1) % 256 for k in range(3)], 1)
        imgs.append(img.to(torch.uint8).view(16, 16, 3))
    return imgs


def pixels_in_ref64(img, normalize):
    """(ref, A) [h, w, 3]: u / 255, then 2 x - 1."""
    x = img.double() / 255.0
    return (2.0 * x - 1.0, 2.0 * x + 1.0) if normalize else (x, x)


def pixels_in_emulate(img, normalize, dtype, defect=None):
    x = img.float() / torch.tensor(256.0 if defect == "in_over_256" else 255.0, dtype=torch.float32, device=img.device)
    if normalize:
        x = torch.tensor(2.0, dtype=torch.float32, device=img.device) * x - torch.tensor(1.0, dtype=torch.float32, device=img.device)
    return x.to(dtype)


def pixels_in_check(out3, img, normalize, f16):
    """f16: the float64 value rounded ONCE (exact: the fp32 route gives that for all 256 bytes, tests/test_pointwise_check_cpu.py);
    fp32: two roundings (the divide; 2 x - 1 fuses or the doubling is exact)."""
    ref, a = pixels_in_ref64(img, normalize)
    if f16:
        return exact_check(out3, to_f16_rne(ref))
    return budget_check(out3, ref, U24 * a, 2, False)


def f16_finite_values(device):
    """All 63 488 finite f16 bit patterns (both zeros, the subnormals), as f16 [63488]."""
    bits = torch.arange(0x7C00, device=device, dtype=torch.int32)              # 0x0000 .. 0x7bff; with the sign bit: the same minus 2^15 as int16
    return torch.cat([bits, bits - 32768]).to(torch.int16).view(torch.float16)


def f32_tie_values(device):
    """fp32 values at and one / two ulp32 on either side of every (k + 0.5) / 255 * 2 - 1, k = 0 .. 254: 1275 values."""
    k = torch.arange(255, device=device, dtype=torch.float64)
    v0 = ((k + 0.5) / 255.0 * 2.0 - 1.0).float()
    up, dn = torch.tensor(2.0, device=device), torch.tensor(-2.0, device=device)
    v = [v0, torch.nextafter(v0, up), torch.nextafter(v0, dn)]
    v += [torch.nextafter(v[1], up), torch.nextafter(v[2], dn)]
    return torch.cat(v)


def pixels_out_src(values, ld, device):
    """[1, 248 or more, 256, ld] in values.dtype: every value of `values` appears in each of the three channels (shifted against each other);
    columns past 2 hold NaN.  Returns (src, [npix, 3] view of the values)."""
    n = values.numel()
    npix = -(-n // 256) * 256
    i = torch.arange(npix, device=device)[:, None]
    c = torch.arange(3, device=device)[None, :]
    v3 = values[(i + c * 20011) % n]
    src = torch.full((1, npix // 256, 256, ld), float("nan"), dtype=values.dtype, device=device)
    src[0, :, :, :3] = v3.view(npix // 256, 256, 3)
    return src, v3


def pixels_out_fp32_spec(v):
    """The expression of include/fie.h as the fp32 kernel evaluates it: x = fl(v / 2 + 0.5) (the halving is exact, so a fused and an unfused
    form agree), clamp, p = fl(255 x), round half to even.  Returns (byte, p)."""
    x = (v.double() * 0.5 + 0.5).float()
    x = torch.where(torch.isnan(x), torch.zeros_like(x), x).clamp(0.0, 1.0)             # fmaxf(NaN, 0) = 0
    p = (x.double() * 255.0).float()
    return torch.round(p).to(torch.uint8), p


def pixels_out_expect(v):
    """(expected byte, decided_by_fp32_spec mask) for inputs v (f16 or fp32 tensor).  The byte is float64 rint(clip(v / 2 + 0.5, 0, 1) * 255),
    half to even; +inf -> 255, -inf -> 0, NaN -> 0.  For EVERY finite f16 input the fp32 expression gives exactly this byte (the only exact
    ties are +-0 -> 127.5 -> 128; tests/test_pointwise_check_cpu.py checks all 63 488), so the f16 entry is compared with it and nothing else.
    fp32 inputs one or two ulp32 from a tie (k + 0.5) / 255 * 2 - 1 are different: the two fp32 roundings of the expression (2 * 2^-24 * 255
    = 3.0e-5 in p) carry 310 of the 1275 values of f32_tie_values across or exactly onto k + 0.5, where float64 cannot be what a correct
    fp32 kernel returns.  Within TIE_BAND of a tie the byte is therefore what the fp32 expression AS WRITTEN gives (pixels_out_fp32_spec:
    bit-defined, half to even); everywhere else float64 decides."""
    v64 = v.double()
    p = torch.where(torch.isnan(v64), torch.zeros_like(v64), v64 * 0.5 + 0.5).clamp(0.0, 1.0) * 255.0
    byte = torch.round(p).to(torch.uint8)
    if v.dtype == torch.float16:
        return byte, torch.zeros_like(byte, dtype=torch.bool)
    near = ((p - torch.floor(p)) - 0.5).abs() <= TIE_BAND
    return torch.where(near, pixels_out_fp32_spec(v)[0], byte), near


def pixels_out_emulate(v, defect=None):
    """pixels_out_kernel in torch fp32 on v (f16 or fp32): u8 of the same shape."""
    _, p = pixels_out_fp32_spec(v.float())
    if defect == "out_truncates":
        return p.to(torch.uint8)
    if defect == "out_half_away":
        return torch.floor(p.double() + 0.5).to(torch.uint8)
    return torch.round(p).to(torch.uint8)


# ------------------------------------------------------------------------------------------------------------------ exact tables: clip_embed, add
CLIP_SHAPES = [(1, 1, 8, 2), (2, 77, 64, 1000), (3, 5, 1280, 50)]           # (B, T, C, vocab)


def exact_f16(shape, seed, device):
    """f16 values with |v| in [2^-6, 8) (random sign, exponent, mantissa): the fp32 sum of any two is exact."""
    g = _gen(seed)
    n = int(torch.tensor(shape).prod())
    exp = torch.randint(9, 18, (n,), generator=g)                  # biased exponents 9 .. 17: 2^-6 .. just below 2^3
    man = torch.randint(0, 1024, (n,), generator=g)
    sign = torch.randint(0, 2, (n,), generator=g)
    bits = ((exp << 10) | man) - 32768 * sign                      # the sign bit, as int16
    v = bits.to(torch.int16).view(torch.float16).view(shape).to(device)
    assert bool((v.abs() >= 2.0 ** -6).all()) and bool((v.abs() < 8.0).all())
    return v


def clip_case(b, t, c, vocab, seed, device, dtype=torch.float16):
    """ids int32 [b, t] with 0, vocab - 1 and repeats; tok [vocab, c], pos [t, c] from exact_f16 (every position row is its own)."""
    g = _gen(seed)
    ids = torch.randint(0, vocab, (b, t), generator=g, dtype=torch.int32)
    flat = ids.view(-1)
    flat[0] = 0
    flat[-1] = vocab - 1
    if flat.numel() > 3:
        flat[1], flat[2] = vocab - 1, vocab - 1
    return {"ids": ids.to(device), "tok": exact_f16((vocab, c), seed + 1, device).to(dtype), "pos": exact_f16((t, c), seed + 2, device).to(dtype), "dtype": dtype}


def clip_expect(case):
    """[b * t, c] in the storage type: the float64 sum rounded once (exact in fp32)."""
    b, t = case["ids"].shape
    s = case["tok"].double()[case["ids"].long()] + case["pos"].double()[None]
    s = s.view(b * t, -1)
    return to_f16_rne(s) if case["dtype"] == torch.float16 else s.float()


# ------------------------------------------------------------------------------------------------------------------ amax
AMAX_PLACES = ["first_vector", "last_vector", "lane7", "second_trip", "negative"]
AMAX_BIG = (2049, 2048)             # rows x C: rows * C / 8 = 524 544 > 2048 * 256 vectors, the loop's second trip


def amax_case(place, device, seed=0):
    """x f16 [rows, C] inside a [rows, C + 8] buffer whose padding holds 60000, NaN and Inf; the body |N(0, 1)| <= 8 with NaN and +-Inf
    sprinkled in (they must not count) and the maximum 100 (or -100) planted at `place`.  Returns (view, expected max |x|)."""
    rows, c = AMAX_BIG if place == "second_trip" else (37, 72)
    g = _gen(seed)
    buf = _randn((rows, c + 8), g, device).clamp(-8.0, 8.0).half()
    buf[:, c:] = torch.tensor([60000.0, float("nan"), float("inf"), -60000.0, float("-inf"), 1000.0, float("nan"), 65504.0], dtype=torch.float16, device=device)
    x = buf[:, :c]
    x[rows // 2, 3], x[rows // 3, 9], x[rows - 1, 0] = float("nan"), float("inf"), float("-inf")
    r, col, val = {"first_vector": (0, 2, 100.0), "last_vector": (rows - 1, c - 5, 100.0), "lane7": (rows // 2, 15, 100.0),
                   "second_trip": (rows - 1, c - 1, 100.0), "negative": (5, 11, -100.0)}[place]
    if place == "second_trip":
        assert (r * (c // 8) + col // 8) >= 2048 * 256
    x[r, col] = val
    return x, 100.0


def amax_expect(x):
    a = x.double().abs()
    a = torch.where(torch.isfinite(a), a, torch.zeros_like(a))
    return float(a.max())
