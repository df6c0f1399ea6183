"""The references, bounds and builders of tests/test_pointwise_gpu.py (tests/pointwise_check.py) on fp32 emulations of the kernels of
csrc/pointwise.hip and csrc/lcm.hip: a straight emulation (torch fp32, one rounding per operation, no fused multiply-add) stays inside every bound with no
mismatch, and every defect model is flagged on the builders' data.  The sizes are the GPU module's small ones; the large ones differ only
in the number of elements.

What tests/test_ops_gpu.py::test_lcm_step_and_latent_prep asserts (allclose, atol = 1e-4, at c_skip = 1e-8) is evaluated on the model that
drops the c_skip term: it passes."""
import pytest
import torch

import pointwise_check as pc

DEV = torch.device("cpu")
F16, F32 = torch.float16, torch.float32
DTYPES = [F16, F32]
HW_CPU = (1, 255, 1000, 20011)


def _lcm_cases(dtype):
    sets = pc.lcm_scalar_sets()
    cases = []
    for i, hw in enumerate(HW_CPU):
        for j, (name, scal) in enumerate(sets.items()):
            for nb in (1, 2):
                for use_noise in (True, False):
                    cases.append((f"hw={hw} {name} nb={nb} noise={use_noise}", pc.lcm_case(hw, 4 + 4 * ((i + j + nb) % 2), nb, use_noise, scal, 10 * i + j, DEV, dtype)))
    return cases


@pytest.fixture(scope="module", params=DTYPES, ids=["f16", "f32"])
def lcm_cases(request):
    return _lcm_cases(request.param)


def test_lcm_step_emulation_is_inside_the_bound(lcm_cases):
    worst = 0.0
    for name, case in lcm_cases:
        lat, mi, dec = pc.lcm_emulate(case)
        n, where, r = pc.lcm_check(lat, case)
        assert n == 0, f"{name}: {n} elements beyond {pc.LCM_N} roundings, first at {where}, worst ratio {r:.2f}"
        f16 = case["dtype"] == F16
        for what, dst, scale in (("model_in", mi, 1.0), ("decode_in", dec, case["scal"]["inv_sf"])):
            n, where, _ = pc.copy_check(dst, lat, scale, f16)
            assert n == 0, f"{name} {what}: {n} elements, first at {where}"
        worst = max(worst, r)
    print(f"\n[lcm_step emulation] worst ratio {worst:.2f} of n = {pc.LCM_N}")
    assert 0.5 < worst <= pc.LCM_N


@pytest.mark.parametrize("defect", pc.LCM_DEFECTS)
def test_lcm_step_defects_are_flagged(lcm_cases, defect):
    hits = [name for name, case in lcm_cases if pc.lcm_check(pc.lcm_emulate(case, defect)[0], case)[0]]
    print(f"\n[lcm_step {defect}] flagged by {len(hits)} of {len(lcm_cases)} cases")
    assert hits, f"{defect}: no case flags it"
    if defect == "c_skip_dropped":          # the synthetic scalars and the schedule's own at t = 19 carry the term; at t = 999 it is 2.5e-9 x
        assert any("synthetic" in h for h in hits)
    if defect == "renoise_on_last":
        assert all("noise=False" in h for h in hits)
    if defect == "guidance_swapped":
        assert all("nb=2" in h for h in hits)


def test_todays_assertion_passes_a_kernel_without_the_c_skip_term():
    """tests/test_ops_gpu.py::test_lcm_step_and_latent_prep: hw = 1024, nb = 2, guidance 1.5, c_skip = 1e-8, allclose(atol = 1e-4) against a
    torch fp32 expression: the model that drops c_skip x passes it, and the new check flags the same model on the same inputs once c_skip
    carries weight."""
    hw = 1024
    g = torch.Generator().manual_seed(0)
    lat0 = torch.randn(hw, 4, generator=g)
    eps = torch.randn(2, hw, 4, generator=g).half()
    z = torch.randn(4, hw, generator=g)
    old = dict(guidance=1.5, sab_t=0.5269, s1mab_t=0.8499, c_skip=1e-8, c_out=1.0, sab_p=0.8118, s1mab_p=0.5840, inv_sf=1 / 0.13025)
    case = {"hw": hw, "nb": 2, "eps": eps, "lat": lat0, "noise": z, "use_noise": True, "scal": {k: pc.f32v(v) for k, v in old.items()}, "dtype": F16}
    e = eps[0].float() + 1.5 * (eps[1].float() - eps[0].float())
    ref2 = 0.8118 * (1.0 * ((lat0 - 0.8499 * e) / 0.5269) + 1e-8 * lat0) + 0.5840 * z.T
    broken = pc.lcm_emulate(case, "c_skip_dropped")[0]
    assert torch.allclose(broken, ref2, atol=1e-4)                     # today's assertion: passes the broken kernel
    assert pc.lcm_check(broken, case)[0] == 0                          # ... and at c_skip = 1e-8 nothing can tell (the term is below one rounding)
    case["scal"] = dict(case["scal"], c_skip=pc.f32v(0.3))
    n, where, r = pc.lcm_check(pc.lcm_emulate(case, "c_skip_dropped")[0], case)
    assert n > 0.9 * 4 * hw and r > 1e4, (n, r)
    assert pc.lcm_check(pc.lcm_emulate(case)[0], case)[0] == 0


# ------------------------------------------------------------------------------------------------------------------ latent_prep
@pytest.fixture(scope="module", params=DTYPES, ids=["f16", "f32"])
def prep_cases(request):
    return [(f"hw={hw}", pc.prep_case(hw, 30 + i, DEV, request.param)) for i, hw in enumerate(HW_CPU)]


def test_latent_prep_emulation_is_inside_the_bound(prep_cases):
    worst = 0.0
    for name, case in prep_cases:
        lv = case["mom"][:, 4:].float()
        if case["hw"] >= 7:
            assert float(lv.min()) < -30 and float(lv.max()) > 20            # both clamp limits are reached
        lat, mi = pc.prep_emulate(case)
        n, where, r = pc.prep_check(lat, case)
        assert n == 0, f"{name}: {n} elements beyond {pc.PREP_N} roundings, first at {where}, worst ratio {r:.2f}"
        assert pc.copy_check(mi, lat, 1.0, case["dtype"] == F16)[0] == 0
        worst = max(worst, r)
    print(f"\n[latent_prep emulation] worst ratio {worst:.2f} of n = {pc.PREP_N}")
    assert 0.5 < worst <= pc.PREP_N


@pytest.mark.parametrize("defect", pc.PREP_DEFECTS)
def test_latent_prep_defects_are_flagged(prep_cases, defect):
    hits = {name: pc.prep_check(pc.prep_emulate(case, defect)[0], case) for name, case in prep_cases}
    flagged = [k for k, v in hits.items() if v[0]]
    print(f"\n[latent_prep {defect}] flagged by {flagged}")
    assert flagged
    if defect == "no_clamp":                # both limits: a row planted below -30 (first block: nothing but exp(logvar / 2) eps) and one above 20
        case = dict(prep_cases)["hw=1000"]
        lat = pc.prep_emulate(case, defect)[0]
        ref, a = pc.prep_ref64(case)
        bad = ~((lat.double() - ref).abs() <= pc.PREP_N * pc.U24 * a)
        lv = case["mom"][:, 4:].float()
        assert bool((bad & (lv < -30)).any()) and bool((bad & (lv > 20)).any())
    if defect == "expf_residue_twice":      # the finding of tests/test_pointwise_gpu.py: up to 6 ulp in exp(logvar / 2) at |logvar| = 16 .. 30
        worst = max(v[2] for v in hits.values())
        print(f"[latent_prep {defect}] worst ratio {worst:.2f} of n = {pc.PREP_N}")
        assert "hw=20011" in flagged and pc.PREP_N < worst < 16
    if defect == "noise_hw4":
        assert "hw=1" not in flagged and len(flagged) == len(prep_cases) - 1           # one pixel: the two layouts coincide


# ------------------------------------------------------------------------------------------------------------------ sinusoid
def _sin_outputs(dtype, defect=None):
    for si, (b, nv, dim, col0, ld) in enumerate(pc.SIN_SHAPES):
        for shift in (0, 4):
            vals = pc.sin_vals(b, nv, DEV, shift + si)
            ref, delta = pc.sin_ref64(vals, dim)
            yield f"{(b, nv, dim)} shift {shift}", pc.sin_emulate(vals, dim, dtype, defect), ref, delta, vals


@pytest.mark.parametrize("dtype", DTYPES, ids=["f16", "f32"])
def test_sinusoid_emulation_is_inside_the_bound(dtype):
    worst, seen = 0.0, set()
    for name, out, ref, delta, vals in _sin_outputs(dtype):
        n, where, r = pc.sin_check(out, ref, delta, dtype == F16)
        assert n == 0, f"{name}: {n} elements, first at {where}, ratio {r:.2f}"
        worst = max(worst, r)
        seen |= set(vals.flatten().tolist())
    print(f"\n[sinusoid emulation] worst ratio {worst:.2f} of the bound")
    assert seen == set(pc.TIMESTEPS) and worst <= 1.0


def test_sinusoid_known_answers_agree_with_the_reference():
    ref, delta = pc.sin_ref64(torch.tensor([[499.0]]), 320)
    for at, want in pc.KAT_499:
        assert torch.allclose(ref[0, 0, at:at + 3], torch.tensor(want, dtype=torch.float64), atol=float(delta[0, 0, at:at + 3].max()) + 5e-9)


@pytest.mark.parametrize("defect", pc.SIN_DEFECTS)
@pytest.mark.parametrize("dtype", DTYPES, ids=["f16", "f32"])
def test_sinusoid_defects_are_flagged(dtype, defect):
    hits = [name for name, out, ref, delta, _ in _sin_outputs(dtype, defect) if pc.sin_check(out, ref, delta, dtype == F16)[0]]
    assert len(hits) >= 6, hits            # every shape (at dim = 2 half - 1 = 0 divides by zero); t = 0 alone in a row hides the frequency


# ------------------------------------------------------------------------------------------------------------------ time_embed
def _te_cases():
    cases = []
    for si, (c0, e) in enumerate(pc.TE_SHAPES):
        for b in (1, 2, 3, 4):
            if e == 1280 and b in (2, 3):
                continue                                      # the CPU self-check keeps one small and one full batch of the large shape
            cases.append((f"C0={c0} E={e} B={b}", pc.te_case(c0, e, b, (b + si) % 2 == 0 or b == 4, 50 + 4 * si + b, DEV, t_shift=b + si)))
    return cases


@pytest.fixture(scope="module")
def te_cases():
    return _te_cases()


def test_time_embed_emulation_is_inside_both_layers_bounds(te_cases):
    w1, w2 = 0.0, 0.0
    for name, case in te_cases:
        out, hbuf = pc.te_emulate(case)
        n, where, r1 = pc.te_layer1_check(hbuf, case)
        assert n == 0, f"{name} layer 1: {n} elements, first at {where}, ratio {r1:.2f}"
        n, where, r2 = pc.te_layer2_check(out, hbuf, case)
        assert n == 0, f"{name} layer 2: {n} elements, first at {where}, ratio {r2:.2f}"
        w1, w2 = max(w1, r1), max(w2, r2)
    print(f"\n[time_embed emulation] worst ratio layer 1 {w1:.2f}, layer 2 {w2:.2f} of the bound")


@pytest.mark.parametrize("c0,e", pc.TE_SHAPES)
def test_time_embed_structural_case_has_one_answer(c0, e):
    case = pc.te_structural_case(c0, e, 3, DEV)
    x = pc.sin_emulate(case["t"].view(-1, 1), c0, F16)[:, 0]
    assert bool((x[:, :c0 // 2] == 1).all()) and bool((x[:, c0 // 2:] == 0).all())
    assert len(set(case["pre"].tolist())) >= 5 and float(case["pre"].abs().max()) <= 6
    out, hbuf = pc.te_emulate(case)
    for n, where, r in pc.te_structural_check(out, hbuf, case):
        assert n == 0, (where, r)
    for defect in ("quarter_skipped",):
        o, h = pc.te_emulate(case, defect)
        assert pc.te_structural_check(o, h, case)[1][0] > 0
    wrong_neuron = torch.roll(out, 1, 1)                       # every output one neuron off
    assert pc.te_structural_check(wrong_neuron, hbuf, case)[1][0] > e // 2
    w1 = case["w1"].clone()
    kq = c0 // 4
    case2 = dict(case, w1=torch.cat([w1[:, kq:2 * kq], w1[:, :kq], w1[:, 2 * kq:]], 1))        # quarters 0 and 1 exchanged: the sums stay, the check must pass
    o2, h2 = pc.te_emulate(case2)
    assert pc.te_structural_check(o2, h2, case)[0][0] == 0
    case3 = dict(case, w1=torch.cat([w1[:, 2 * kq:3 * kq], w1[:, kq:2 * kq], w1[:, :kq], w1[:, 3 * kq:]], 1))      # quarter 0 read where quarter 2 is
    o3, h3 = pc.te_emulate(case3)
    assert pc.te_structural_check(o3, h3, case)[0][0] > 0


@pytest.mark.parametrize("defect", pc.TE_DEFECTS)
def test_time_embed_defects_are_flagged(te_cases, defect):
    hits = []
    for name, case in te_cases:
        out, hbuf = pc.te_emulate(case, defect)
        if pc.te_layer2_check(out, hbuf, case)[0]:
            hits.append(name)
    print(f"\n[time_embed {defect}] flagged by {len(hits)} of {len(te_cases)} cases")
    assert hits
    if defect == "quarter_skipped":
        assert len(hits) == len(te_cases)


def test_time_embed_layers_are_checked_apart():
    """A hidden vector that is wrong is flagged by layer 1's check alone: layer 2 is held to the hidden vector the kernel left."""
    case = pc.te_case(64, 256, 2, True, 7, DEV)
    out, hbuf = pc.te_emulate(case)
    bad_h = hbuf.clone()
    bad_h[1, 5] += 0.01
    out2 = pc.te_emulate(dict(case))[0]
    assert pc.te_layer1_check(bad_h, case)[0] == 1 and pc.te_layer1_check(hbuf, case)[0] == 0
    assert pc.te_layer2_check(out2, hbuf, case)[0] == 0


# ------------------------------------------------------------------------------------------------------------------ pixels
def test_pixels_in_fp32_route_is_the_single_rounding_for_every_byte():
    """What makes the f16 check exact: u / 255 (then 2 x - 1) in fp32, stored as f16, is the float64 value rounded once for all 256 bytes."""
    for img in pc.pix_all_values(DEV) + [pc.pix_image(16, 16, DEV), pc.pix_image(1, 1, DEV)]:
        for normalize in (0, 1):
            assert pc.pixels_in_check(pc.pixels_in_emulate(img, normalize, F16), img, normalize, True)[0] == 0
            n, _, r = pc.pixels_in_check(pc.pixels_in_emulate(img, normalize, F32), img, normalize, False)
            assert n == 0 and r <= 2
            assert pc.pixels_in_check(pc.pixels_in_emulate(img, normalize, F16, "in_over_256"), img, normalize, True)[0] > 0 or img.numel() == 3
            assert pc.pixels_in_check(pc.pixels_in_emulate(img, normalize, F32, "in_over_256"), img, normalize, False)[0] > 0 or img.numel() == 3
    img = pc.pix_image(769, 683, DEV)
    assert [int(img[..., c].flatten()[:256].unique().numel()) for c in range(3)] == [256] * 3


def test_pixels_out_fp32_expression_is_exact_for_every_finite_f16():
    """What makes the f16 check exact, and the three pinned special values."""
    v = pc.f16_finite_values(DEV)
    assert v.numel() == 63488
    want, near = pc.pixels_out_expect(v)
    assert not bool(near.any())
    assert bool((pc.pixels_out_emulate(v) == want).all())
    p = pc.pixels_out_fp32_spec(v.float())[1]
    ties = (p - torch.floor(p)) == 0.5
    # +-0 -> 127.5 -> 128; the smallest subnormal 2^-24 rounds onto 0.5 in fp32 and goes to 128 as well, where float64's 127.5000038 goes
    assert v[ties].double().tolist() == [0.0, 2.0 ** -24, -0.0] and bool((want[ties] == 128).all())
    sp = torch.tensor([float("inf"), float("-inf"), float("nan")])
    for dt in DTYPES:
        assert pc.pixels_out_expect(sp.to(dt))[0].tolist() == [255, 0, 0] and pc.pixels_out_emulate(sp.to(dt)).tolist() == [255, 0, 0]
    assert int((pc.pixels_out_emulate(v, "out_truncates") != want).sum()) > 10000
    assert int((pc.pixels_out_emulate(v, "out_half_away") != want).sum()) == 0          # not reachable from f16: only the fp32 entry's ties show it


def test_pixels_out_fp32_tie_neighbours():
    """Float64 decides every fp32 input farther than TIE_BAND (in p = 255 x) from a tie; inside the band the fp32 expression as written does.
    The band holds every tie neighbour, 638 of them land exactly on k + 0.5 in fp32, and float64 disagrees with the correct fp32 kernel on
    310: comparing those with float64 would fail a correct kernel."""
    v = torch.cat([pc.f32_tie_values(DEV), pc.f16_finite_values(DEV).float()])
    want, near = pc.pixels_out_expect(v)
    assert bool(near[:1275].all()) and int(near[1275:].sum()) <= 20          # the tie neighbours, and a few f16 values (next to +-0, 2 / 255, 4 / 255)
    assert bool((pc.pixels_out_emulate(v) == want).all())
    p64 = (v.double() * 0.5 + 0.5).clamp(0, 1) * 255.0
    f64_byte = torch.round(p64).to(torch.uint8)
    assert int((f64_byte[:1275] != want[:1275]).sum()) == 310
    p = pc.pixels_out_fp32_spec(v)[1]
    assert int(((p - torch.floor(p)) == 0.5)[:1275].sum()) == 638
    assert int((pc.pixels_out_emulate(v, "out_half_away") != want).sum()) > 100          # half away from zero: flagged here, and only here
    assert int((pc.pixels_out_emulate(v, "out_truncates") != want).sum()) > 10000
    rnd = torch.randn(100000, generator=torch.Generator().manual_seed(1))                # away from the band float64 and fp32 agree
    w2, n2 = pc.pixels_out_expect(rnd)
    assert bool((pc.pixels_out_emulate(rnd)[~n2] == w2[~n2]).all()) and float(n2.float().mean()) < 0.02


def test_pixels_out_src_holds_every_value_in_every_channel():
    v = pc.f16_finite_values(DEV)
    for ld in (3, 8):
        src, v3 = pc.pixels_out_src(v, ld, DEV)
        assert src.shape == (1, 248, 256, ld) and bool(torch.isnan(src[..., 3:]).all())
        for c in range(3):
            assert len(set(v3[:, c].view(torch.int16).tolist())) == 63488


# ------------------------------------------------------------------------------------------------------------------ exact tables
@pytest.mark.parametrize("dtype", DTYPES, ids=["f16", "f32"])
def test_clip_embed_sums_are_exact_in_fp32(dtype):
    for i, (b, t, c, vocab) in enumerate(pc.CLIP_SHAPES):
        case = pc.clip_case(b, t, c, vocab, 70 + i, DEV, dtype)
        ids = case["ids"].view(-1).tolist()
        assert vocab - 1 in ids and (len(ids) < 4 or (0 in ids and len(set(ids)) < len(ids)))
        s32 = (case["tok"].float()[case["ids"].long()] + case["pos"].float()[None]).view(b * t, c)
        s64 = (case["tok"].double()[case["ids"].long()] + case["pos"].double()[None]).view(b * t, c)
        assert bool((s32.double() == s64).all())                                       # exact in fp32
        assert pc.exact_check(s32.to(dtype), pc.clip_expect(case))[0] == 0
        if t > 1:                                                                      # a wrong r % T moves whole rows
            wrong = (case["tok"].float()[case["ids"].long()] + torch.roll(case["pos"].float(), 1, 0)[None]).view(b * t, c).to(dtype)
            assert pc.exact_check(wrong, pc.clip_expect(case))[0] > 0.9 * b * t * c


def test_amax_cases():
    for place in pc.AMAX_PLACES:
        if place == "second_trip":
            continue                                           # the same builder at 2049 x 2048; the GPU module runs it
        x, want = pc.amax_case(place, DEV)
        assert pc.amax_expect(x) == want == 100.0
        assert not bool(torch.isfinite(x).all()) and x.stride(0) == x.shape[1] + 8
    rows, c = pc.AMAX_BIG
    assert rows * c // 8 > 2048 * 256 and ((rows - 1) * (c // 8) + (c - 1) // 8) >= 2048 * 256
