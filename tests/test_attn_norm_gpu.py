"""Attention (csrc/attention.hip) and the norm kernels (csrc/norm.hip) against the float64 references and checkers of tests/attn_norm_check.py
(tests/test_attn_norm_check_cpu.py shows on the CPU which defects they catch).

Attention, every forced variant (fie_debug_attn_variant 0 .. 6) and the d = 512 kernels:
  exact cases   selector (q_i = g k_pi(i), random +-1 keys), ramp (the last visible key wins; causal: row i = V[i], also Tq != Tk) and uniform
                (every P = 1, integer V: out = sum V / count, negative scores so that an unmasked zero-filled key would take the row): bit for
                bit (uniform with a count that is no power of two: 1 ulp16), fused-QKV strides, padded output rows, an explicit scale.
  real data     |out - ref| <= 0.5 ulp16 + C_ATTN eps_q dev per element; e4m3 outputs within 1 e4m3 ulp of the float64 reference.
Norms: |out - ref| <= 0.5 ulp + C_NORM 2^-24 (|x| + |mu| + sigma) |gamma| / sigma A per element at group means of 0, 8 and 64 sigma, one
constant for every GroupNorm form (each single-pass instantiation, the three-kernel plan, its column split, statistics from a producer's
epilogue: per group, per quad, gathered granules, coefficients), the f32 entry points and LayerNorm; which form ran is read from the launch log.
"""
import re

import pytest
import torch

import attn_norm_check as an
import launch_check as lc

DEV = "cuda"

# The two constants, as MEASURED_RATIO / C_FP32 in tests/test_launch_table_gpu.py: the worst ratio one MI355X run of this module printed, doubled.
#   attention: 1.429 at variant 0 (and 2 .. 6: the same bits), d = 64, Tq = Tk = 1024, N(0, 1) data, fused-QKV strides; the first-generation kernel
#              (variant 1) 1.005, d = 512 below both.  The model (P rounded toward zero in f16, tests/test_attn_norm_check_cpu.py) gives 0.2 - 1.
#   norms:     4.352 at fie_groupnorm_nhwc_f32, three-kernel plan, rows = 100, C = 64 (f16: 3.819 at rows = 1100, C = 1280 + 1280, column split 2);
#              the single-pass kernels 1.3 - 2.6, LayerNorm 0.84 at most.
#              Statistics from a producer's epilogue (fie_gn_stats_target): 1.2 - 1.7 per group and per quad, 4.52 through gathered granules
#              (rows = 131 072, C = 128), 4.25 through fie_groupnorm_coef_f16 -- inside the constant, which was fixed before those paths met it:
#              their raw fp32 sums of y^2 measured 26 - 47 at 64 sigma until groups beyond 8 sigma took their variance from the tensor itself
#              (csrc/norm.hip: gn_centred_m2), as the three-kernel plan measured 235 before its sums were shifted by a per-group pivot.
MEASURED_RATIO_ATTN = 1.429
C_ATTN = 2.9
MEASURED_RATIO_NORM = 4.352
C_NORM = 8.7
F8_OUT_OF_BOUND_CAP = 0.005         # e4m3 outputs: share of elements allowed beyond 1 e4m3 ulp of the float64 reference (ties on a rounding boundary)

B, H = 2, 3
# (Tq, Tk): every Tq of {1, 15, 16, 17, 77, 200, 333, 1024} and every Tk of {1, 63, 64, 65, 77, 96, 97, 200, 333, 1024}
PAIRS = [(1, 1), (15, 63), (16, 64), (17, 65), (77, 77), (200, 96), (333, 97), (1024, 200), (77, 333), (200, 1024), (1024, 1024), (1, 97)]
PAIRS_512 = [(1, 31), (17, 32), (77, 33), (200, 100), (333, 1024)]
_CACHE = {}


def _cached(key, make):
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


def _gen(seed):
    g = torch.Generator(device=DEV)
    g.manual_seed(seed)
    return g


# ------------------------------------------------------------------------------------------------------------------ launch helpers
def _rows(t):
    """[B, H, T, D] -> [B * T, H * D] (the library's layout)."""
    b, h, n, d = t.shape
    return t.permute(0, 2, 1, 3).reshape(b * n, h * d).contiguous()


def _run_attention(ctx, case, variant=0, fused=False, pad=0, f8_inv=None):
    """One launch on the case's q, k, v; fused: q, k, v are column slices of one [B * T, 3 C] buffer (Tq == Tk); pad: extra columns behind the
    output rows (ldo > H * D), which must keep their fill.  Returns [B, H, Tq, D]."""
    from fie_amd import hip
    q, k, v = case["q"], case["k"], case["v"]
    b, h, tq, d = q.shape
    tk, c = k.shape[2], h * d
    if fused:
        assert tq == tk
        buf = torch.cat([_rows(q), _rows(k), _rows(v)], 1).contiguous()
        q2, k2, v2 = buf[:, :c], buf[:, c:2 * c], buf[:, 2 * c:]
    else:
        q2, k2, v2 = _rows(q), _rows(k), _rows(v)
    if f8_inv is None:
        full = torch.full((b * tq, c + pad), float("nan"), device=DEV, dtype=torch.float16)
    else:
        full = torch.full((b * tq, c + pad), 0x7f, device=DEV, dtype=torch.uint8)
    out = full[:, :c]
    assert hip.lib().fie_debug_attn_variant(ctx.h, variant) == 0
    try:
        ctx.attention(q2, k2, v2, h, d, tq, tk, b, out=out, causal=case["causal"], scale=case["scale"], out_f8=f8_inv is not None,
                      out_inv_scale=f8_inv or 1.0)
    finally:
        hip.lib().fie_debug_attn_variant(ctx.h, 0)
    if pad:
        tail = full[:, c:]
        assert bool(torch.isnan(tail).all()) if f8_inv is None else bool((tail == 0x7f).all()), "the padding behind the output rows was written"
    return out.reshape(b, tq, h, d).permute(0, 2, 1, 3)


def _template_ints(symbol):
    """The integer template arguments in a kernel symbol (mangled 'Li64ELi2E...' or demangled '<64, 2, ...>')."""
    ints = [int(v) for v in re.findall(r"Li(\d+)E", symbol)]
    if not ints and "<" in symbol:
        ints = [int(v) for v in re.findall(r"(?<![\w.])(\d+)(?![\w.])", symbol[symbol.index("<"):])]
    return ints


def _logged(ctx, fn):
    """Runs fn() with the launch log on; returns (result, [(symbol, blocks, threads, description)])."""
    ctx.oplog(True)
    try:
        res = fn()
        lines = ctx.oplog_read()
    finally:
        ctx.oplog(False)
    recs = []
    for l in lines:
        if not l.startswith("#"):
            sym, blocks, threads, _, desc = l.split("|", 4)
            recs.append((sym, int(blocks), int(threads), desc))
    return res, recs


def _attn_form(recs):
    """(kernel generation, template ints) of the one attention launch in `recs`."""
    at = [r for r in recs if r[3].startswith("attn ")]
    assert len(at) == 1, recs
    sym = at[0][0]
    return ("attn2" if "attn2_kernel" in sym else "attn1" if "attn_kernel" in sym else sym), _template_ints(sym), at[0][1], at[0][2]


# what each forced variant launches at d = 64 (csrc/attention.hip: attention_impl): (generation, D, QF, KT[, waves, stages])
def _expected_form(variant, tq, tk, causal, nblk128, num_cus):
    if variant == 1:
        return ("attn1", [64, 2, 64] if nblk128 >= 2 * num_cus else [64, 1, 64])
    if variant == 0:
        if nblk128 >= 4 * num_cus:
            return ("attn2", [64, 2, 64, 4, 2])
        return ("attn2", [64, 1, 96, 4, 2] if tk <= 96 and not causal else [64, 1, 64, 4, 2])
    return ("attn2", {2: [64, 2, 64, 4, 2], 3: [64, 1, 64, 4, 2], 4: [64, 2, 64, 2, 2], 5: [64, 1, 64, 4, 3], 6: [64, 1, 64, 8, 2]}[variant])


def _check_form(ctx, recs, variant, case):
    b, h, tq, d = case["q"].shape
    tk = case["k"].shape[2]
    gen, ints, blocks, threads = _attn_form(recs)
    if d == 512:
        want = ("attn1" if variant == 1 else "attn2", [512, 1, 32])
    else:
        want = _expected_form(variant, tq, tk, case["causal"], (tq + 127) // 128 * h * b, torch.cuda.get_device_properties(0).multi_processor_count)
    assert gen == want[0] and ints[:len(want[1])] == want[1], f"variant {variant} Tq={tq} Tk={tk}: ran {gen}{ints}, expected {want}"
    return ints


# ------------------------------------------------------------------------------------------------------------------ attention: exact cases
def _exact_cases(tq, tk, d):
    """name -> (case, kind) for one (Tq, Tk): built once, shared by the variants."""
    def make():
        g = 16.0 if d == 64 else 4.0
        gr = 8.0 if d == 64 else 4.0
        out = {}
        out["selector"] = (an.selector_case(B, H, tq, tk, d, g, _gen(tq * 4099 + tk)), "pick")
        out["ramp"] = (an.ramp_case(B, H, tq, tk, d, False, DEV, g=gr), "pick")
        out["ramp causal"] = (an.ramp_case(B, H, tq, tk, d, True, DEV, g=gr), "pick")
        for c in (0.0, -8.0, 8.0):
            out[f"uniform c={c:g}"] = (an.uniform_case(B, H, tq, tk, d, c, False, DEV), "uniform")
        out["uniform causal c=-8"] = (an.uniform_case(B, H, tq, tk, d, -8.0, True, DEV), "uniform")
        if (tq, tk) in ((77, 333), (77, 77), (77, 33)):                       # an explicit scale other than d^-0.5
            sc = 0.2 if d == 64 else 0.07
            out["selector scale"] = (an.selector_case(B, H, tq, tk, d, g, _gen(7), scale=sc), "pick")
            out["uniform scale c=-8"] = (an.uniform_case(B, H, tq, tk, d, -8.0, False, DEV, scale=sc), "uniform")
            out["ramp causal scale"] = (an.ramp_case(B, H, tq, tk, d, True, DEV, g=2 * gr, scale=sc), "pick")
        return out
    return _cached(("exact", tq, tk, d), make)


def _exact_failures(ctx, variant, pairs, d):
    fails, forms, n = [], set(), 0
    for pi, (tq, tk) in enumerate(pairs):
        for ci, (name, (case, kind)) in enumerate(_exact_cases(tq, tk, d).items()):
            fused, pad = (tq == tk and ci % 2 == 0), (64 if (pi + ci) % 2 else 0)
            out, recs = _logged(ctx, lambda: _run_attention(ctx, case, variant, fused=fused, pad=pad))
            forms.add(tuple(_check_form(ctx, recs, variant, case)))
            n += 1
            tag = f"variant {variant} d={d} Tq={tq} Tk={tk} {name}{' fused-qkv' if fused else ''}{' padded-out' if pad else ''}"
            if kind == "pick":
                bad, where = lc.exact_mismatches(out, case["expect"].double())
                if bad:
                    fails.append(f"{tag}: {bad} elements differ, first {an.describe_pick(out, case, where[0])}")
            else:
                bad, where = an.uniform_mismatches(out, case["ref"], case["count"])
                if bad:
                    i = where[0]
                    fails.append(f"{tag}: {bad} elements off, first at {i}: out {float(out[i])} ref {float(case['ref'][i]):.6f} (count {int(case['count'][i[2]])})")
    return fails, forms, n


@pytest.mark.gpu
@pytest.mark.parametrize("variant", [0, 1, 2, 3, 4, 5, 6])
def test_attention_exact_cases_d64(fie, variant):
    fails, forms, n = _exact_failures(fie, variant, PAIRS, 64)
    print(f"\n[attn exact] variant {variant}: {n} launches, kernel forms {sorted(forms)}")
    for f in fails:
        print(f"[attn exact] FAIL {f}")
    assert not fails, f"{len(fails)} of {n} exact cases failed (printed above)"
    if variant == 0:                                    # both default forms at these sizes: the one-tile KT = 96 form and the 64-key tiles
        assert (64, 1, 96, 4, 2) in forms and (64, 1, 64, 4, 2) in forms


@pytest.mark.gpu
@pytest.mark.parametrize("variant", [0, 1])
def test_attention_exact_cases_d512(fie, variant):
    fails, forms, n = _exact_failures(fie, variant, PAIRS_512, 512)
    print(f"\n[attn exact] d=512 variant {variant}: {n} launches, kernel forms {sorted(forms)}")
    for f in fails:
        print(f"[attn exact] FAIL {f}")
    assert not fails, f"{len(fails)} of {n} exact cases failed (printed above)"


@pytest.mark.gpu
def test_attention_exact_cases_reach_the_128_query_form_by_the_default_rule(fie):
    """B = 2, H = 16, Tq = 4096, Tk = 200: (Tq / 128) H B blocks >= 4 x the CU count, so variant 0 itself picks attn2_kernel<64, 2, 64>."""
    b, h, tq, tk = 2, 16, 4096, 200
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    assert (tq // 128) * h * b >= 4 * cus, f"{cus} CUs: the shape does not reach the rule's threshold"
    cases = {"selector": (an.selector_case(b, h, tq, tk, 64, 16.0, _gen(11)), "pick"),
             "ramp": (an.ramp_case(b, h, tq, tk, 64, False, DEV), "pick"),
             "uniform c=-8": (an.uniform_case(b, h, tq, tk, 64, -8.0, False, DEV), "uniform")}
    for name, (case, kind) in cases.items():
        out, recs = _logged(fie, lambda: _run_attention(fie, case, 0))
        gen, ints, blocks, threads = _attn_form(recs)
        assert (gen, ints[:5]) == ("attn2", [64, 2, 64, 4, 2]) and blocks == (tq // 128) * h * b and threads == 256, (gen, ints, blocks, threads)
        if kind == "pick":
            bad, where = lc.exact_mismatches(out, case["expect"].double())
            assert not bad, f"{name}: {bad} elements differ, first {an.describe_pick(out, case, where[0])}"
        else:
            bad, where = an.uniform_mismatches(out, case["ref"], case["count"])
            assert not bad, f"{name}: {bad} elements off, first at {where}"


# ------------------------------------------------------------------------------------------------------------------ attention: real data
REAL_64 = [(77, 77, False, True), (200, 333, True, False), (333, 200, False, False), (1024, 1024, False, False), (77, 1024, True, False),
           (17, 97, True, False), (200, 96, False, False), (1024, 1024, True, True)]           # (Tq, Tk, peaky, causal)
REAL_512 = [(100, 100, False, False), (77, 1024, True, False), (33, 31, False, False)]


def _real(tq, tk, d, peaky, causal):
    def make():
        case = an.real_case(B, H, tq, tk, d, peaky, causal, _gen(tq * 31 + tk * 7 + d + peaky))
        case["budget"] = an.attn_budget64(case["q"], case["k"], case["v"], case["scale"], causal)
        return case
    return _cached(("real", tq, tk, d, peaky, causal), make)


def _real_worst(ctx, variant, shapes, d):
    worst, fails = (0.0, None), []
    for tq, tk, peaky, causal in shapes:
        case = _real(tq, tk, d, peaky, causal)
        ref, dev, eps = case["budget"]
        out = _run_attention(ctx, case, variant, fused=(tq == tk and not causal), pad=8 if peaky else 0)
        r = an.attn_ratio(out, ref, dev, eps)
        tag = f"variant {variant} d={d} Tq={tq} Tk={tk}{' peaky' if peaky else ''}{' causal' if causal else ''}"
        if r > worst[0]:
            worst = (r, tag)
        if r > C_ATTN:
            n, where = an.attn_mismatches(out, ref, dev, eps, C_ATTN)
            fails.append(f"{tag}: ratio {r:.2f} > {C_ATTN} at {n} elements, first at {where}")
    return worst, fails


@pytest.mark.gpu
@pytest.mark.parametrize("variant", [0, 1, 2, 3, 4, 5, 6])
def test_attention_real_data_per_element(fie, variant):
    worst, fails = _real_worst(fie, variant, REAL_64, 64)
    if variant in (0, 1):
        w5, f5 = _real_worst(fie, variant, REAL_512, 512)
        worst, fails = max(worst, w5), fails + f5
    print(f"\n[attn real] variant {variant}: worst ratio {worst[0]:.3f} (C_ATTN = {C_ATTN}) at {worst[1]}")
    for f in fails:
        print(f"[attn real] FAIL {f}")
    assert not fails, f"{len(fails)} cases beyond the per-element bound (printed above)"


@pytest.mark.gpu
@pytest.mark.parametrize("variant", [0, 2, 3, 4, 5, 6])
def test_attention_e4m3_output_against_float64(fie, variant):
    inv = 8.0
    for tq, tk, peaky, causal in REAL_64[:5]:
        case = _real(tq, tk, 64, peaky, causal)
        ref = case["budget"][0]
        o8 = _run_attention(fie, case, variant, pad=16 if peaky else 0, f8_inv=inv)
        n, where = lc.f8_mismatches(o8.contiguous(), ref * inv, n_ulp=1)
        print(f"\n[attn e4m3] variant {variant} Tq={tq} Tk={tk}: {n} of {ref.numel()} elements beyond 1 e4m3 ulp of the float64 reference")
        assert n <= F8_OUT_OF_BOUND_CAP * ref.numel(), (variant, tq, tk, n, where)
    # saturation: |out * inv| > 448 must store exactly +-448
    case = _real(77, 77, 64, False, True)
    ref = case["budget"][0]
    o = _run_attention(fie, case, variant, f8_inv=4096.0).contiguous().view(torch.float8_e4m3fn).double()
    sat = (ref * 4096.0).abs() > 480.0
    assert int(sat.sum()) > 1000 and bool((o[sat] == 448.0 * torch.sign(ref[sat])).all())


# ------------------------------------------------------------------------------------------------------------------ norms
def _gn_form(c1, c2, groups, rows):
    """(V, NV) of the single-pass kernel csrc/norm.hip: gn_onepass() launches for this shape, or None (three-kernel plan)."""
    c = c1 + c2
    cg = c // groups
    if c2 and c1 % cg:
        return None
    v = 8 if cg % 8 == 0 else 4 if cg % 4 == 0 else 0
    if not v or c1 % v or c2 % v or cg // v > 1024:
        return None
    npv = cg // v
    nv = -(-rows // (1024 // npv))
    if v == 8 and nv <= 5:
        return (8, 5)
    if v == 8 and nv <= 10:
        return (8, 10)
    if v == 4 and nv <= 20:
        return (4, 20)
    return None


def _gn_csplit(c, groups):
    """Column split of csrc/norm.hip: gn_plan()."""
    nc8 = c // 8
    split = (nc8 + 255) // 256
    while split <= nc8 and (nc8 % split or ((nc8 // split) * 8) % (c // groups)):
        split += 1
    return split


def _row_step(c1, c2, groups):
    cg = (c1 + c2) // groups
    v = 8 if cg % 8 == 0 else 4
    return 1024 // (cg // v)


# (rows, C1, C2, groups, form the default dispatch must take): every single-pass instantiation, the fallback, the column split, a seam on and
# off a group border, 20 / 40-channel groups, cg = 2 (n = 2 .. 16 at rows 1 .. 8), rows 1 / 5 / 8 / 100 and one row past a row step
GN_SHAPES = [(1, 256, 0, 32, (8, 5)), (5, 256, 0, 32, (8, 5)), (8, 256, 0, 32, (8, 5)), (100, 256, 0, 32, (8, 5)), (1025, 256, 0, 32, (8, 5)),
             (5121, 256, 0, 32, (8, 10)), (1024, 1280, 0, 32, (8, 10)), (205, 1280, 0, 32, (8, 5)), (100, 320, 960, 32, (8, 5)),
             (100, 640, 0, 32, (4, 20)), (1024, 640, 0, 32, (4, 20)), (4096, 128, 0, 32, (4, 20)), (1025, 128, 0, 32, (4, 20)),
             (1, 64, 0, 32, None), (5, 64, 0, 32, None), (8, 64, 0, 32, None), (100, 64, 0, 32, None),
             (10300, 256, 0, 32, None), (100, 328, 952, 32, None), (1100, 1280, 1280, 32, None), (4100, 640, 0, 32, None)]


def _run_groupnorm(ctx, x1, x2, groups, gamma, beta, silu, onepass=True, f8_inv=None):
    from fie_amd import hip
    try:
        hip.lib().fie_debug_gn_onepass(ctx.h, int(onepass))
        return _logged(ctx, lambda: ctx.groupnorm(x1, gamma, beta, groups, 1e-5, silu, x2=x2, out_f8=f8_inv is not None, out_inv_scale=f8_inv or 1.0))
    finally:
        hip.lib().fie_debug_gn_onepass(ctx.h, 1)


def _ran_gn(recs):
    """'onepass (V, NV)' / 'partial' / 'finalize-from-epilogue' / 'gather-granules' from the launch log's descriptions."""
    descs = [r[3] for r in recs]
    one = [r for r in recs if r[3].startswith("groupnorm onepass")]
    if one:
        return tuple(_template_ints(one[0][0])[:2])
    for key in ("partial", "gather-granules", "finalize-from-epilogue"):
        if any(d.startswith("groupnorm " + key) for d in descs):
            return key
    raise AssertionError(f"no GroupNorm launch in {recs}")


@pytest.mark.gpu
def test_groupnorm_every_form_per_element(fie):
    worst, fails, forms, by_form = (0.0, None), [], set(), {}
    for si, (rows, c1, c2, groups, form) in enumerate(GN_SHAPES):
        assert _gn_form(c1, c2, groups, rows) == form, (rows, c1, c2, form)
        c = c1 + c2
        gamma, beta = an.affine(c, DEV)
        inputs = [("offsets", an.gn_input(B, rows, c, groups, _gen(100 + si)))]
        if rows * (c // groups) % 2 == 0 and rows <= 1100:
            inputs.append(("two-level", an.gn_two_level(B, rows, c, groups, DEV)))
        for iname, x in inputs:
            silu = (si + len(iname)) % 2 == 0
            ref, slack = an.gn_ref64(x, groups, gamma, beta, 1e-5, silu)
            x1, x2 = (x[..., :c1].contiguous(), x[..., c1:].contiguous()) if c2 else (x, None)
            for onepass in (True, False):
                out, recs = _run_groupnorm(fie, x1, x2, groups, gamma, beta, silu, onepass)
                ran = _ran_gn(recs)
                assert ran == (form if onepass and form else "partial"), f"rows={rows} C={c1}+{c2}: ran {ran}, expected {form if onepass else 'partial'}"
                forms.add(ran if ran != "partial" else f"partial csplit={_gn_csplit(c, groups)}")
                if ran == "partial":
                    blocks = [r[1] for r in recs if r[3].startswith("groupnorm partial")][0]
                    assert blocks % (B * _gn_csplit(c, groups)) == 0
                r = an.norm_ratio(out, ref, slack)
                tag = f"groupnorm rows={rows} C={c1}+{c2} G={groups} silu={silu} {iname} ran {ran}"
                by_form[str(ran)] = max(by_form.get(str(ran), (0.0, "")), (r, tag))
                if r > worst[0]:
                    worst = (r, tag)
                if r > C_NORM:
                    n, where = an.norm_mismatches(out, ref, slack, C_NORM)
                    i = where[0]
                    fails.append(f"{tag}: ratio {r:.2f} > {C_NORM} at {n} elements, first at {i}: out {float(out[i])} ref {float(ref[i]):.6f}")
    print(f"\n[groupnorm] forms run: {sorted(map(str, forms))}")
    for k, (r, tag) in sorted(by_form.items()):
        print(f"[groupnorm] form {k}: worst ratio {r:.3f} at {tag}")
    print(f"[groupnorm] worst ratio {worst[0]:.3f} (C_NORM = {C_NORM}) at {worst[1]}")
    for f in fails:
        print(f"[groupnorm] FAIL {f}")
    for want in [(8, 5), (8, 10), (4, 20), "partial csplit=1", "partial csplit=2"]:
        assert want in forms, f"{want} never ran: {forms}"
    assert not fails, f"{len(fails)} cases beyond the per-element bound (printed above)"
    # one row past a multiple of the kernel's row step is among the shapes
    assert 1025 % _row_step(256, 0, 32) == 1 and 205 % _row_step(1280, 0, 32) == 1


def _offset_bias(cout, groups, device):
    """A conv bias that puts group g of the output at 0, 8 or 64 sigma (the conv's own output has sigma ~ 1), with alternating sign."""
    g = torch.arange(cout, device=device) // (cout // groups)
    off = torch.tensor(an.OFFSETS, device=device)[g % 3] * torch.where(g % 2 == 0, 1.0, -1.0)
    return off.to(torch.float16)


def _producer(ctx, b, h, w, cin, cout, groups, seed):
    """A conv whose epilogue leaves the GroupNorm sums of its output, the output's groups offset through the bias."""
    g = _gen(seed)
    x0 = torch.randn((b, h, w, cin), generator=g, device=DEV).half()
    wt = (torch.randn((cout, cin, 3, 3), generator=g, device=DEV) * (9 * cin) ** -0.5).half()
    y = ctx.conv3x3(x0, ctx.pack_conv3x3(wt), cout, bias=_offset_bias(cout, groups, DEV), gn_groups=groups)
    assert y._gn_tag is not None
    return y


@pytest.mark.gpu
@pytest.mark.parametrize("b,h,w,cin,cout,expect", [(2, 48, 48, 64, 128, "finalize-from-epilogue"), (2, 48, 48, 64, 256, "finalize-from-epilogue"),
                                                   (1, 48, 48, 64, 512, "finalize-from-epilogue"), (1, 64, 64, 128, 640, "finalize-from-epilogue"),
                                                   (1, 64, 64, 128, 1280, "finalize-from-epilogue"), (1, 512, 256, 64, 128, "gather-granules")])
def test_groupnorm_from_the_producers_statistics_per_element(fie, b, h, w, cin, cout, expect):
    """fie_groupnorm_stats_nhwc_f16 behind a conv armed with gn_groups=: per-group slots (4 / 8 / 16 channels), per-quad slots (20 / 40 channels,
    partial_groups = C / 4) and, from 4096 granules on, gn_gather_granules_kernel.  The conv's bias puts its output groups at 0, 8 and 64 sigma."""
    groups = 32
    y = _producer(fie, b, h, w, cin, cout, groups, 200 + cout)
    if cout in (640, 1280):
        assert y._gn_tag[7] == cout // 4
    else:
        assert y._gn_tag[7] == groups
    gamma, beta = an.affine(cout, DEV)
    silu = cout != 256
    out, recs = _logged(fie, lambda: fie.groupnorm(y, gamma, beta, groups, 1e-6, silu))
    assert _ran_gn(recs) == expect and not any(r[3].startswith("groupnorm partial") for r in recs), recs
    y3 = y.view(b, h * w, cout)
    ref, slack = an.gn_ref64(y3, groups, gamma, beta, 1e-6, silu)
    mu = y3.double().view(b, h * w, groups, -1).mean((1, 3))
    sd = y3.double().view(b, h * w, groups, -1).std((1, 3))
    assert float((mu.abs() / sd).max()) > 40, "the producer's output does not reach the 64-sigma regime"
    r = an.norm_ratio(out.view(b, h * w, cout), ref, slack)
    print(f"\n[groupnorm stats] {expect} rows={h * w} C={cout}: ratio {r:.3f} (C_NORM = {C_NORM}), max mean/sigma {float((mu.abs() / sd).max()):.1f}")
    assert r <= C_NORM, an.norm_mismatches(out.view(b, h * w, cout), ref, slack, C_NORM)


@pytest.mark.gpu
def test_groupnorm_coefficients_per_element(fie):
    """fie_groupnorm_coef_f16 (the GroupNorm a fused conv applies in LDS, fie_conv3x3_gn_nhwc_f16): the coefficients (sc, sh) evaluated in float64
    are a GroupNorm within the bound (groups of 0, 8 and 64 sigma through the producer's bias).  What the conv makes of the coefficients stays with tests/test_ops_gpu.py: test_groupnorm_fused_into_the_halo_conv."""
    groups, h, w, cin, cout = 32, 32, 48, 128, 128
    fuse0, fie.gn_fuse_conv = fie.gn_fuse_conv, True
    try:
        y = _producer(fie, 1, h, w, 64, cin, groups, 300)
        assert fie.conv3x3_gn_ok(y, cout, groups)
        gamma, beta = an.affine(cin, DEV)
        coef, recs = _logged(fie, lambda: fie.groupnorm_coef(y, gamma, beta, groups, 1e-6))
        assert any(r[3].startswith("groupnorm coefficients") for r in recs)
        y3 = y.view(1, h * w, cin)
        ref, slack = an.gn_ref64(y3, groups, gamma, beta, 1e-6, False)
        applied = y3.double() * coef[:, :, 0].double()[:, None, :] + coef[:, :, 1].double()[:, None, :]
        r = an.norm_ratio(applied.float(), ref, slack, f32=True)
        print(f"\n[groupnorm coef] ratio {r:.3f} (C_NORM = {C_NORM})")
        assert r <= C_NORM, an.norm_mismatches(applied.float(), ref, slack, C_NORM, f32=True)
    finally:
        fie.gn_fuse_conv = fuse0


def _call_f32(ctx, name, *args):
    from fie_amd import hip
    ctx.sync_stream()
    hip._chk(getattr(hip.lib(), name)(ctx.h, *args))


@pytest.mark.gpu
def test_f32_norm_entry_points_per_element(fie):
    """fie_groupnorm_nhwc_f32 (each single-pass width and the three-kernel plan) and fie_layernorm_f32: the same bound with the fp32 spacing."""
    from fie_amd import hip
    P = hip._p
    worst, by_form = (0.0, None), {}
    for si, (rows, c, groups, form) in enumerate([(100, 256, 32, (8, 5)), (1024, 640, 32, (4, 20)), (1024, 1280, 32, (8, 10)), (100, 64, 32, None)]):
        assert _gn_form(c, 0, groups, rows) == form
        x = an.gn_input(B, rows, c, groups, _gen(400 + si), dtype=torch.float32)
        gamma, beta = an.affine(c, DEV, torch.float32)
        ws = torch.empty(hip.lib().fie_groupnorm_workspace_bytes(B, rows, groups), device=DEV, dtype=torch.uint8)
        for silu in (False, True):
            ref, slack = an.gn_ref64(x, groups, gamma, beta, 1e-5, silu)
            for onepass in (True, False):
                out = torch.full_like(x, float("nan"))
                try:
                    hip.lib().fie_debug_gn_onepass(fie.h, int(onepass))
                    _, recs = _logged(fie, lambda: _call_f32(fie, "fie_groupnorm_nhwc_f32", P(x), c, None, 0, P(out), B, rows, groups, P(gamma), P(beta), 1e-5,
                                                             int(silu), P(ws)))
                finally:
                    hip.lib().fie_debug_gn_onepass(fie.h, 1)
                ran = _ran_gn(recs)
                assert ran == (form if onepass and form else "partial")
                r = an.norm_ratio(out, ref, slack, f32=True)
                by_form[str(ran)] = max(by_form.get(str(ran), (0.0, "")), (r, f"rows={rows} C={c} silu={silu}"))
                if r > worst[0]:
                    worst = (r, f"groupnorm f32 rows={rows} C={c} silu={silu} ran {ran}")
    for si, (rows, c) in enumerate([(5, 64), (77, 1032), (3, 1544), (4, 4096)]):
        x = an.ln_input(rows, c, _gen(450 + si), dtype=torch.float32)
        gamma, beta = an.affine(c, DEV, torch.float32)
        ref, slack = an.ln_ref64(x, gamma, beta, 1e-5)
        out = torch.full_like(x, float("nan"))
        _call_f32(fie, "fie_layernorm_f32", P(x), c, P(out), c, rows, c, P(gamma), P(beta), 1e-5)
        r = an.norm_ratio(out, ref, slack, f32=True)
        if r > worst[0]:
            worst = (r, f"layernorm f32 rows={rows} C={c}")
    for k, (r, tag) in sorted(by_form.items()):
        print(f"\n[norm f32] groupnorm form {k}: worst ratio {r:.3f} at {tag}")
    print(f"\n[norm f32] worst ratio {worst[0]:.3f} (C_NORM = {C_NORM}) at {worst[1]}")
    assert worst[0] <= C_NORM, worst


@pytest.mark.gpu
@pytest.mark.parametrize("c", [64, 768, 1024, 1032, 1536, 1544, 4096])
def test_layernorm_per_element(fie, c):
    """Every width class of ln_kernel (NV = 2 up to 1024, 3 up to 1536, 8 beyond), rows 1 / 3 / 4 / 5 / 77 (four rows per block), row strides
    larger than C on both sides, rows offset by 0, 8 and 64 sigma."""
    gamma, beta = an.affine(c, DEV)
    worst = (0.0, None)
    for ri, rows in enumerate([1, 3, 4, 5, 77]):
        x = an.ln_input(rows, c, _gen(500 + c + ri))
        ref, slack = an.ln_ref64(x, gamma, beta, 1e-5)
        xbuf = torch.zeros((rows, c + 8 * (ri + 1)), device=DEV, dtype=torch.float16)
        xbuf[:, :c] = x
        obuf = torch.full((rows, c + 16), float("nan"), device=DEV, dtype=torch.float16)
        fie.layernorm(xbuf[:, :c], gamma, beta, 1e-5, out=obuf[:, :c])
        assert bool(torch.isnan(obuf[:, c:]).all())
        r = an.norm_ratio(obuf[:, :c], ref, slack)
        if r > worst[0]:
            worst = (r, f"layernorm rows={rows} C={c}")
    print(f"\n[layernorm] C={c}: worst ratio {worst[0]:.3f} (C_NORM = {C_NORM}) at {worst[1]}")
    assert worst[0] <= C_NORM, worst


@pytest.mark.gpu
def test_norm_e4m3_outputs_against_float64(fie):
    """LayerNorm's and GroupNorm's e4m3 outputs against the float64 reference times the inverse scale, and the saturating case."""
    for c in (768, 1032, 1544):
        gamma, beta = an.affine(c, DEV)
        x = an.ln_input(77, c, _gen(600 + c))
        ref, _ = an.ln_ref64(x, gamma, beta, 1e-5)
        for inv, sat in ((16.0, False), (2048.0, True)):
            o8 = fie.layernorm(x, gamma, beta, 1e-5, out_f8=True, out_inv_scale=inv)
            n, where = lc.f8_mismatches(o8, ref * inv, n_ulp=1)
            print(f"\n[norm e4m3] layernorm C={c} inv={inv:g}: {n} of {ref.numel()} elements beyond 1 e4m3 ulp of the float64 reference")
            assert n <= F8_OUT_OF_BOUND_CAP * ref.numel(), (c, inv, n, where)
            if sat:
                big = (ref * inv).abs() > 480.0
                o = o8.view(torch.float8_e4m3fn).double()
                assert int(big.sum()) > 1000 and bool((o[big] == 448.0 * torch.sign(ref[big])).all())
    for rows, c, form in [(100, 256, (8, 5)), (1024, 640, (4, 20)), (4100, 640, None)]:
        gamma, beta = an.affine(c, DEV)
        x = an.gn_input(B, rows, c, 32, _gen(700 + c + rows))
        for silu in (False, True):
            ref, _ = an.gn_ref64(x, 32, gamma, beta, 1e-5, silu)
            for inv, sat in ((16.0, False), (2048.0, True)):
                o8, recs = _run_groupnorm(fie, x, None, 32, gamma, beta, silu, f8_inv=inv)
                assert _ran_gn(recs) == (form or "partial")
                n, where = lc.f8_mismatches(o8, ref * inv, n_ulp=1)
                print(f"\n[norm e4m3] groupnorm rows={rows} C={c} silu={silu} inv={inv:g}: {n} of {ref.numel()} elements beyond 1 e4m3 ulp")
                assert n <= F8_OUT_OF_BOUND_CAP * ref.numel(), (rows, c, silu, inv, n, where)
                if sat:
                    big = (ref * inv).abs() > 480.0
                    o = o8.view(torch.float8_e4m3fn).double()
                    assert int(big.sum()) > 1000 and bool((o[big] == 448.0 * torch.sign(ref[big])).all())
