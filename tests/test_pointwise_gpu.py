"""The pointwise kernels of the denoising loop (csrc/pointwise.hip, csrc/lcm.hip) per element, on the f16 context and, wherever an _f32 entry exists, on an
fp32 context: float64 references on the stored inputs, bounds derived from the fp32 arithmetic of each expression and the builders of
tests/pointwise_check.py (tests/test_pointwise_check_cpu.py shows on the CPU that a straight fp32 emulation passes every check and which
defects each one flags).  No assertion is normalised by a tensor's maximum; every message names the first bad elements.

The worst ratio each test printed in one MI355X run stands beside its bound below (MEASURED_*; profiles/pointwise_pins.md has the table).  One
finding: latent_prep measured 8.47 (f16) / 8.64 (fp32) of its 7 roundings, because the compiler's expansion of expf under -ffp-contract=fast
counts the residue of x log2(e) twice (up to 6 ulp in exp(logvar / 2)); csrc/fie_internal.h: fie_expf replaced it: 3.93 / 3.87."""
import pytest
import torch

import pointwise_check as pc

pytestmark = pytest.mark.gpu
DEV = "cuda"
F16, F32 = torch.float16, torch.float32

# Worst ratio of one MI355X run of this module; the bounds were derived before it (tests/pointwise_check.py) and none was moved by it.
MEASURED_LCM = {"f16": 4.132, "f32": 4.737}            # of LCM_N = 8 roundings (hw = 524 588, the synthetic scalars, nb = 2, noise)
MEASURED_PREP = {"f16": 3.926, "f32": 3.870}           # of PREP_N = 7 (hw = 524 588); 8.471 / 8.639 with the compiler's expf
MEASURED_SIN = {"f16": 0.340, "f32": 0.580}            # of 1: |arg| (u + 1.5) 2^-23 + 2^-22 (t = 759 / 999 at dim 320; dim 256 behind col0 = 1280)
MEASURED_TE = {"layer1": 0.192, "layer2": 0.001}       # of 1: what exceeds the f16 half ulp, over the rest of the bound (C0 = 32, E = 64; E = 256)
MEASURED_PIXELS_IN_F32 = 0.992                         # of 2 roundings; the f16 entry, pixels_out, clip_embed, add and amax are exact


@pytest.fixture(scope="module")
def f32():
    import fie_amd  # noqa: F401
    from fie_amd import hip
    return hip.context(0, torch.float32)


@pytest.fixture(params=["f16", "f32"])
def ctx(request, fie, f32):
    return fie if request.param == "f16" else f32


def _name(ctx):
    return "f32" if ctx.f32 else "f16"


def _fail(fails, tag, res, what="elements beyond the bound"):
    n, where, r = res
    if n:
        fails.append(f"{tag}: {n} {what}, first at {where}, worst ratio {r:.3g}")
    return r


def _report(fails, label):
    for f in fails:
        print(f"[{label}] FAIL {f}")
    assert not fails, f"{len(fails)} checks failed, first: {fails[0]}"


# ------------------------------------------------------------------------------------------------------------------ 1. lcm_step
# (ld_eps, nb, noise, copies of model_in (0: NULL), decode_in): every value of every argument, at the large size and at the small ones
LCM_COMBOS = [(4, 2, True, 2, False), (8, 1, False, 0, True), (8, 2, True, 1, True), (4, 1, False, 1, False)]


def _run_lcm(ctx, case, copies, decode):
    hw, dt = case["hw"], case["dtype"]
    lat = case["lat"].clone()
    mi = torch.full((copies, hw, 8), float("nan"), device=DEV, dtype=dt) if copies else None
    dec = torch.full((hw, 8), float("nan"), device=DEV, dtype=dt) if decode else None
    s = case["scal"]
    ctx.lcm_step(case["eps"], case["nb"], s["guidance"], lat, case["noise"] if case["use_noise"] else None, hw, s["sab_t"], s["s1mab_t"], s["c_skip"],
                 s["c_out"], s["sab_p"], s["s1mab_p"], mi, s["inv_sf"], dec)
    return lat, mi, dec


def test_lcm_step_per_element(ctx):
    """|lat - ref| <= 8 x 2^-24 A on the fp32 master latents (c_skip = 2.5e-9 at t = 999 would be 0 in f16; at the synthetic scalars every
    term carries weight); model_in / decode_in against the kernel's own latents; the padding columns exactly zero in every copy."""
    dt = F32 if ctx.f32 else F16
    sets = pc.lcm_scalar_sets()
    names = list(sets)
    fails, worst = [], (0.0, "")
    for i, hw in enumerate(pc.HW_SIZES):
        for k, (ld, nb, noise, copies, decode) in enumerate(LCM_COMBOS):
            sname = names[(i + k) % 3]
            case = pc.lcm_case(hw, ld, nb, noise, sets[sname], 100 + 10 * i + k, DEV, dt)
            lat, mi, dec = _run_lcm(ctx, case, copies, decode)
            tag = f"{_name(ctx)} hw={hw} ld_eps={ld} nb={nb} noise={noise} copies={copies} decode={decode} {sname}"
            r = _fail(fails, tag + " latents", pc.lcm_check(lat, case))
            worst = max(worst, (r, tag))
            for c in range(copies):
                _fail(fails, f"{tag} model_in[{c}]", pc.copy_check(mi[c, :, :4], lat, 1.0, not ctx.f32))
                _fail(fails, f"{tag} model_in[{c}] padding", pc.zero_check(mi[c, :, 4:]), "elements not zero")
            if decode:
                _fail(fails, tag + " decode_in", pc.copy_check(dec[:, :4], lat, case["scal"]["inv_sf"], not ctx.f32))
                _fail(fails, tag + " decode_in padding", pc.zero_check(dec[:, 4:]), "elements not zero")
    print(f"\n[lcm_step {_name(ctx)}] worst ratio {worst[0]:.3f} of n = {pc.LCM_N} at {worst[1]}")
    _report(fails, "lcm_step")


# ------------------------------------------------------------------------------------------------------------------ 2. latent_prep
def test_latent_prep_per_element(ctx):
    """|lat - ref| <= 7 x 2^-24 A with the logvar clamp reached on both sides and distinguishable noise planes; model_in as above."""
    dt = F32 if ctx.f32 else F16
    fails, worst = [], (0.0, "")
    for i, hw in enumerate(pc.HW_SIZES):
        case = pc.prep_case(hw, 200 + i, DEV, dt)
        ref = pc.prep_ref64(case)
        for copies in (1, 3):
            lat = torch.full((hw, 4), float("nan"), device=DEV)
            mi = torch.full((copies, hw, 8), float("nan"), device=DEV, dtype=dt)
            ctx.latent_prep(case["mom"], case["eps"], case["noise"], hw, case["sf"], case["sab"], case["s1mab"], lat, mi)
            tag = f"{_name(ctx)} hw={hw} copies={copies}"
            r = _fail(fails, tag + " latents", pc.prep_check(lat, case, ref))
            worst = max(worst, (r, tag))
            for c in range(copies):
                _fail(fails, f"{tag} model_in[{c}]", pc.copy_check(mi[c, :, :4], lat, 1.0, not ctx.f32))
                _fail(fails, f"{tag} model_in[{c}] padding", pc.zero_check(mi[c, :, 4:]), "elements not zero")
    print(f"\n[latent_prep {_name(ctx)}] worst ratio {worst[0]:.3f} of n = {pc.PREP_N} at {worst[1]}")
    _report(fails, "latent_prep")


# ------------------------------------------------------------------------------------------------------------------ 3. sinusoid
def test_sinusoid_every_element_every_timestep(ctx):
    """Every element of [cos | sin] at every value of TIMESTEPS in every shape, and the three known answers at t = 499."""
    dt = F32 if ctx.f32 else F16
    fails, worst = [], (0.0, "")
    for si, (b, nv, dim, col0, ld) in enumerate(pc.SIN_SHAPES):
        seen = set()
        for shift in range(0, len(pc.TIMESTEPS), b * nv):
            vals = pc.sin_vals(b, nv, DEV, shift)
            seen |= set(vals.flatten().tolist())
            ref, delta = pc.sin_ref64(vals, dim)
            buf = torch.full((b, ld), float("nan"), device=DEV, dtype=dt)
            ctx.sinusoid(vals, dim, buf, col0)
            out = buf[:, col0:col0 + nv * dim].reshape(b, nv, dim)
            tag = f"{_name(ctx)} {(b, nv, dim, col0, ld)} t={vals.flatten().tolist()}"
            r = _fail(fails, tag, pc.sin_check(out, ref, delta, not ctx.f32))
            worst = max(worst, (r, tag))
            rest = torch.cat([buf[:, :col0], buf[:, col0 + nv * dim:]], 1)
            if rest.numel() and not bool(torch.isnan(rest).all()):
                fails.append(f"{tag}: columns outside [col0, col0 + nvals dim) were written")
            if dim == 320:
                for bi in (vals.flatten() == 499.0).nonzero().flatten().tolist():
                    for at, want in pc.KAT_499:
                        got = out[bi, 0, at:at + 3].double()
                        tol = 2e-3 if not ctx.f32 else float(delta[bi, 0, at:at + 3].max()) + 5e-9
                        if not torch.allclose(got, torch.tensor(want, dtype=torch.float64, device=DEV), rtol=0, atol=tol):
                            fails.append(f"{tag}: known answers at column {at}: {got.tolist()} for {want}")
        assert seen == set(pc.TIMESTEPS)
    print(f"\n[sinusoid {_name(ctx)}] worst ratio {worst[0]:.3f} of the bound at {worst[1]}")
    _report(fails, "sinusoid")


# ------------------------------------------------------------------------------------------------------------------ 4. time_embed
def _run_te(fie, case, ws):
    b, e = case["b"], case["e"]
    buf = torch.full((b, e + 40), float("nan"), device=DEV, dtype=F16)           # ld_out > E
    fie.time_embed(case["t"], case["w1"], case["b1"], case["w2"], case["b2"], ws, add=case["add"], out=buf[:, :e])
    hbuf = ws[:b * e * 2].view(F16).view(b, e).clone()
    assert bool(torch.isnan(buf[:, e:]).all()), "the padding behind the output rows was written"
    return buf[:, :e], hbuf


@pytest.mark.parametrize("c0,e", pc.TE_SHAPES)
def test_time_embed_layers_apart(fie, c0, e):
    """Layer 1 (the hidden vector the kernel leaves in its workspace) against float64 silu(W1 sinusoid + b1); layer 2 against float64 on that
    hidden vector: a defect in one layer cannot hide behind the other's rounding.  B = 1 .. 4, add present (row stride > E) and NULL."""
    ws = fie.time_embed_workspace(e)
    fails, w1, w2 = [], (0.0, ""), (0.0, "")
    for b in (1, 2, 3, 4):
        for add in (True, False):
            case = pc.te_case(c0, e, b, add, 300 + 10 * b + add, DEV, t_shift=2 * b + add)
            out, hbuf = _run_te(fie, case, ws)
            tag = f"C0={c0} E={e} B={b} add={add} t={case['t'].tolist()}"
            w1 = max(w1, (_fail(fails, tag + " layer 1", pc.te_layer1_check(hbuf, case)), tag))
            w2 = max(w2, (_fail(fails, tag + " layer 2", pc.te_layer2_check(out, hbuf, case)), tag))
    fie.check_device_errors()
    assert int(ws[-16:-8].view(torch.int32).abs().sum()) == 0          # both barrier counters back at zero
    print(f"\n[time_embed C0={c0} E={e}] worst ratio layer 1 {w1[0]:.3f} at {w1[1]}; layer 2 {w2[0]:.3f} at {w2[1]}")
    _report(fails, "time_embed")


@pytest.mark.parametrize("c0,e", pc.TE_SHAPES)
def test_time_embed_structural(fie, c0, e):
    """Integer sums, one valid answer per element (1 ulp16): a wrong neuron, K quarter or output row moves whole elements."""
    ws = fie.time_embed_workspace(e)
    fails = []
    for b in (1, 4):
        case = pc.te_structural_case(c0, e, b, DEV)
        out, hbuf = _run_te(fie, case, ws)
        res = pc.te_structural_check(out, hbuf, case)
        _fail(fails, f"C0={c0} E={e} B={b} hidden vector", res[0], "elements off the integer answer")
        _fail(fails, f"C0={c0} E={e} B={b} output", res[1], "elements off silu(hbuf[perm])")
    _report(fails, "time_embed structural")


# ------------------------------------------------------------------------------------------------------------------ 5. / 6. pixels
def test_pixels_in_per_element(ctx):
    """f16: the float64 value rounded once, bit for bit; fp32: two roundings; columns 3 .. 7 exactly zero; every copy."""
    images = [(f"{h}x{w}", pc.pix_image(h, w, DEV)) for h, w in pc.PIX_SIZES] + [(f"all values in channel {c}", im) for c, im in enumerate(pc.pix_all_values(DEV))]
    fails, worst = [], 0.0
    for name, img in images:
        for copies in (1, 3):
            for normalize in (0, 1):
                out = torch.full((copies,) + tuple(img.shape[:2]) + (8,), float("nan"), device=DEV, dtype=ctx.dtype)
                ctx.pixels_in(img, normalize, copies=copies, out=out)
                for c in range(copies):
                    tag = f"{_name(ctx)} {name} normalize={normalize} copy {c} of {copies}"
                    worst = max(worst, _fail(fails, tag, pc.pixels_in_check(out[c, ..., :3], img, normalize, not ctx.f32)))
                    _fail(fails, tag + " padding", pc.zero_check(out[c, ..., 3:]), "elements not zero")
    print(f"\n[pixels_in {_name(ctx)}] worst ratio {worst:.3f}" + (" of 2 roundings" if ctx.f32 else " (exact)"))
    _report(fails, "pixels_in")


def test_pixels_out_every_input(ctx):
    """Every finite f16 bit pattern in every channel (the fp32 entry: the same values widened, and fp32 values at and next to every rounding
    tie) at ld = 3 and 8, NaN behind the three channels; +inf -> 255, -inf -> 0, NaN -> 0.  Exact: no element is excluded."""
    values = pc.f16_finite_values(DEV)
    if ctx.f32:
        values = torch.cat([values.float(), pc.f32_tie_values(DEV)])
    fails = []
    for ld in (3, 8):
        src, v3 = pc.pixels_out_src(values, ld, DEV)
        want, near = pc.pixels_out_expect(v3)
        out = ctx.pixels_out(src).view(-1, 3)
        res = pc.exact_check(out, want)
        _fail(fails, f"{_name(ctx)} ld={ld}", res, "bytes differ")
        if res[0]:
            i = res[1][0]
            fails[-1] += f": input {float(v3[i]):.9g} gave {int(out[i])}, expected {int(want[i])}"
        print(f"\n[pixels_out {_name(ctx)}] ld={ld}: {v3.numel()} inputs, {int(near.sum())} within the tie band (decided by the fp32 expression)")
    sp = torch.tensor([float("inf"), float("-inf"), float("nan"), 0.0, -0.0, 1.0, -1.0, 70000.0 if ctx.f32 else 65504.0], device=DEV, dtype=ctx.dtype)
    src = sp[:, None].expand(8, 4).contiguous().view(1, 2, 4, 4)
    got = ctx.pixels_out(src)[..., 0].flatten().tolist()
    assert got == [255, 0, 0, 128, 128, 255, 0, 255], got
    _report(fails, "pixels_out")


def test_pixels_round_trip_at_the_grid_stride_size(ctx):
    """769 x 683 = 525 227 pixels: both kernels' loops repeat; pixels_out(pixels_in(img)) == img."""
    h, w = pc.PIX_SIZES[-1]
    assert h * w > 2048 * 256
    img = pc.pix_image(h, w, DEV)
    x = ctx.pixels_in(img, 1, copies=1)
    back = ctx.pixels_out(x)
    n, where, _ = pc.exact_check(back, img)
    assert n == 0, f"{_name(ctx)}: {n} bytes differ after the round trip, first at {where}"
    want, _ = pc.pixels_out_expect(x[0, ..., :3])
    n, where, _ = pc.exact_check(back, want)
    assert n == 0, f"{_name(ctx)}: {n} bytes differ from the expected byte, first at {where}"


# ------------------------------------------------------------------------------------------------------------------ 7. clip_embed
@pytest.mark.parametrize("b,t,c,vocab", pc.CLIP_SHAPES)
def test_clip_embed_exact(ctx, b, t, c, vocab):
    """tok[ids] + pos with exact fp32 sums: the float64 sum rounded once, bit for bit (a wrong row of either table moves whole rows)."""
    case = pc.clip_case(b, t, c, vocab, 400 + c, DEV, ctx.dtype)
    out = torch.full((b * t, c), float("nan"), device=DEV, dtype=ctx.dtype)
    ctx.clip_embed(case["ids"], case["tok"], case["pos"], out=out)
    n, where, _ = pc.exact_check(out, pc.clip_expect(case))
    assert n == 0, f"{_name(ctx)} {(b, t, c, vocab)}: {n} elements differ, first at {where} (row r = b T + t, ids {case['ids'].view(-1)[:4].tolist()} ...)"


# ------------------------------------------------------------------------------------------------------------------ 8. add, amax
@pytest.mark.parametrize("n", [8, 8 * 257, 8 * (4096 * 256 + 3)])
def test_add_exact(fie, n):
    """out = a + b on values whose fp32 sum is exact (the last size: the loop's second trip over 4096 blocks)."""
    from fie_amd import hip
    a, b = pc.exact_f16((n,), 500, DEV), pc.exact_f16((n,), 501, DEV)
    out = torch.full((n,), float("nan"), device=DEV, dtype=F16)
    fie.sync_stream()
    hip._chk(hip.lib().fie_add_f16(fie.h, hip._p(a), hip._p(b), hip._p(out), n))
    cnt, where, _ = pc.exact_check(out, pc.to_f16_rne(a.double() + b.double()))
    assert cnt == 0, f"n={n}: {cnt} elements differ, first at {where}"


@pytest.mark.parametrize("place", pc.AMAX_PLACES)
def test_amax_finds_the_planted_maximum(fie, place):
    """max |x| over the finite body: larger values, NaN and Inf in the row padding and NaN / Inf in the body do not count."""
    x, want = pc.amax_case(place, DEV)
    assert pc.amax_expect(x) == want
    slot = torch.zeros(1, device=DEV)
    fie.amax_into(x, slot)
    assert float(slot) == want, f"{place}: amax {float(slot)} for {want}"
    fie.amax_into(x * 0.5, slot)                        # folds into the slot: a smaller tensor leaves it
    assert float(slot) == want


def test_amax_subnormal_and_zero_tensors(fie):
    sub = (torch.arange(1, 1 + 16 * 24, device=DEV) % 1023 + 1).to(torch.int16).view(F16).view(16, 24)      # bit patterns 1 .. 1023: all subnormal
    sub[7, 13] = torch.tensor(1023, dtype=torch.int16).view(F16)
    assert float(sub.float().max()) < 2.0 ** -14
    slot = torch.zeros(1, device=DEV)
    fie.amax_into(sub, slot)
    assert float(slot) == 1023 * 2.0 ** -24
    zero = torch.zeros((5, 16), device=DEV, dtype=F16)
    zero[2, 3] = -0.0
    slot = torch.zeros(1, device=DEV)
    fie.amax_into(zero, slot)
    assert float(slot) == 0.0 and slot.view(torch.int32).item() == 0
