"""The fp32 contraction path (csrc/f32.hip: fie_gemm_f32, fie_conv3x3_nhwc_f32, fie_softmax_rows_f32 and the fp32 attention hip.Context.attention
composes from them) against the float64 references and checkers of tests/f32_check.py (tests/test_f32_check_cpu.py shows on the CPU which defects
they catch).  Small shapes at the edges of the 64 x 64 x 16 tile, the 4-wide MFMA k-step and the 4-column lane ownership; every row stride wider than
its matrix and no multiple of 4; every output inside a prefilled buffer whose other elements must keep their bits.

  integer pass   A, W in {-2..2}: bit for bit the float64 result (act NONE / RELU), the activation bound for SiLU / GELU / quick-GELU / GEGLU.
  real pass      |out - ref| <= 0.5 ulp32 + C_F32 sqrt(K) 2^-24 budget + 2^-24 |residual| per element.
  softmax        C_SM 2^-24 (1 + |scale s| + |scale s_max|) ref per element, hidden columns +0.0, dominant rows exactly one-hot.
  attention      selector / ramp / uniform bit for bit, real data under C_ATTN32 (eps32 dev + sqrt(Tk) 2^-24 sum w |v|), and the causal convention
                 of the f16 kernels and of this path compared on one case.
  refusals       every FIE_REQUIRE of the three entries raises and leaves the output untouched.
28 tests, 4.2 s for the module on an MI355X (tests/test_fp32_gpu.py: 15 tests, 5.2 s).
"""
import math

import pytest
import torch

import attn_norm_check as an
import f32_check as fc
import launch_check as lc

pytestmark = pytest.mark.gpu
DEV = "cuda"

# The four constants, as MEASURED_RATIO / C_FP32 in tests/test_launch_table_gpu.py: the worst ratio one MI355X run of this module printed, doubled.
# The measured quantity is the kernel's distance from the float64 reference in units of the analytic budget (never another run of the kernel).
#   contraction: 1.813 at fie_gemm_f32 M = 64, N = 65, K = 1, bias + SiLU + scale 2 + residual (at K = 1 the sqrt(K) chain term is one rounding and the
#                epilogue's four roundings carry the ratio); every K >= 3 case is below 0.73: GEGLU 0.690, concat 0.724, column range 0.524, the [K][N]
#                batch 0.475, conv 0.495 (9 x 7, Cin = 4 packed to 8, stride 2, pad_mode 1).
#   activations: 0.701 on the exact integer sums, GEGLU M = 129, N = 130, K = 200 (SiLU / GELU / quick-GELU 0.653 at most, conv + SiLU 0.634).
#   softmax:     2.352 at rows = 7, cols = 200, scale 0.125, causal, tq = 7.
#   attention:   1.170 at d = 64, Tq = 200, Tk = 96, peaky, causal (B = 2, H = 3).
# The FMA-chain count of the same run: 79 503 of 79 503 elements of the 22 real-data GEMMs equal the k-ascending fp32 FMA chain (33 582 of them also equal
# the float64 sum rounded once), so test_gemm_against_the_fp32_fma_chain asserts the claim of csrc/f32.hip's header as it stands.
MEASURED_RATIO_F32 = 1.813
C_F32 = 3.7
MEASURED_RATIO_ACT32 = 0.701
C_ACT32 = 1.5
MEASURED_RATIO_SM = 2.352
C_SM = 4.8
MEASURED_RATIO_ATTN32 = 1.170
C_ATTN32 = 2.4

# a covering list, not the product: every M of {1, 63, 64, 65, 129}, every N of {1, 2, 3, 63, 64, 65, 130}, every K of {1, 3, 4, 5, 15, 16, 17, 33, 200}
TRIPLES = [(1, 1, 1), (1, 2, 3), (1, 3, 4), (1, 130, 16), (63, 2, 1), (63, 63, 5), (63, 64, 15), (63, 65, 16), (64, 1, 17), (64, 2, 33), (64, 63, 200),
           (64, 64, 16), (64, 65, 1), (65, 3, 15), (65, 63, 4), (65, 64, 17), (65, 65, 33), (65, 130, 5), (129, 1, 200), (129, 64, 3), (129, 65, 200),
           (129, 130, 33)]
RPBS = [7, 64, 100, 1]
GEGLU_SHAPES = [(1, 2, 5), (65, 2, 200), (65, 66, 17), (129, 66, 5), (1, 130, 17), (129, 130, 200)]                     # (M, N, K), N / 2 columns out
CONCAT = [(k1, k2) for k1 in (1, 15, 16, 17) for k2 in (1, 16, 23)]
KN_SHAPES = [(17, 40, 1), (65, 64, 63), (17, 72, 65), (65, 40, 200), (1, 64, 200), (65, 72, 63)]                          # (M, N, K) of the [K][N] batch
# (H, W, Cin, Cout, stride, pad_mode, ups, raw weights, bias, row bias, residual, channel range, scale, act)
CONVS = [(1, 1, 4, 1, 1, 0, False, True, True, False, False, False, 1.0, fc.ACT_NONE),
         (1, 5, 8, 24, 1, 0, False, False, True, True, False, False, 1.0, fc.ACT_RELU),
         (2, 3, 24, 65, 2, 0, False, False, False, False, True, False, 1.0, fc.ACT_SILU),
         (9, 7, 40, 24, 1, 1, False, False, True, False, False, True, 1.0, fc.ACT_NONE),
         (9, 7, 4, 65, 2, 1, False, False, True, False, False, False, 1.0, fc.ACT_RELU),
         (16, 16, 8, 65, 2, 0, False, False, True, False, False, False, 0.5, fc.ACT_NONE),
         (16, 16, 24, 1, 1, 1, False, True, False, True, False, False, 1.0, fc.ACT_NONE),
         (2, 3, 40, 24, 1, 0, True, False, True, False, True, False, 2.0, fc.ACT_NONE),
         (9, 7, 4, 65, 2, 0, True, True, True, False, False, True, 1.0, fc.ACT_RELU),
         (1, 5, 24, 1, 1, 1, True, False, True, False, False, False, 1.0, fc.ACT_SILU),
         (16, 16, 40, 24, 2, 1, False, True, True, True, True, True, 1.0, fc.ACT_SILU),
         (1, 1, 8, 65, 1, 1, True, False, False, False, False, False, 1.0, fc.ACT_NONE),
         (9, 7, 24, 24, 2, 0, False, True, True, False, False, False, 1.0, fc.ACT_NONE)]
SM_ROWS, SM_COLS, SM_TQ = [1, 5, 7, 130], [1, 63, 64, 65, 77, 200, 1025], [1, 7, 77]
B, H = 2, 3
# (Tq, Tk, d); the exact causal cases run on every pair, the real-data causal ones on CAUSAL
PAIRS = [(1, 1, 64), (15, 63, 64), (17, 65, 64), (77, 77, 64), (200, 96, 64), (77, 333, 64), (1, 97, 64), (17, 65, 40), (17, 33, 512)]
CAUSAL = [(77, 77, 64), (77, 333, 64), (200, 96, 64)]


@pytest.fixture(scope="module")
def f32():
    import fie_amd  # noqa: F401
    from fie_amd import hip
    return hip.context(0, torch.float32)


def _gen(seed):
    g = torch.Generator(device=DEV)
    g.manual_seed(seed)
    return g


# ------------------------------------------------------------------------------------------------------------------ buffers
def _ld(cols, extra):
    """A row stride wider than `cols` that is no multiple of 4."""
    ld = cols + extra
    return ld + 1 if ld % 4 == 0 else ld


def _wide(t, extra):
    """t [rows, cols] as a view of a NaN-filled [rows, ld] buffer, ld > cols and ld % 4 != 0."""
    if t is None:
        return None
    buf = torch.full((t.shape[0], _ld(t.shape[1], extra)), float("nan"), device=t.device, dtype=t.dtype)
    v = buf[:, :t.shape[1]]
    v.copy_(t)
    return v


class Out:
    """A [rows, cols] output view at column c0 of a [rows, ld] buffer prefilled with fc.PREFILL; untouched(): everything else kept its bits."""

    def __init__(self, rows, cols, ld, c0=0, init=None):
        self.buf = torch.full((rows, ld), fc.PREFILL, device=DEV, dtype=torch.float32)
        self.view = self.buf[:, c0:c0 + cols]
        if init is not None:
            self.view.copy_(init)
        self.outside = torch.ones((rows, ld), dtype=torch.bool, device=DEV)
        self.outside[:, c0:c0 + cols] = False
        self.before = self.buf.clone()

    def untouched(self):
        return bool((self.buf.view(torch.int32)[self.outside] == self.before.view(torch.int32)[self.outside]).all())

    def unwritten(self):
        """The whole buffer, the view included, kept its bits (a refused call)."""
        return bool((self.buf.view(torch.int32) == self.before.view(torch.int32)).all())


def _gemm_raw(ctx, a1, a2, K1, w, w_kn, out, M, N, K, bias=None, rb=None, rpb=0, res=None, scale=1.0, act=0, nb=(1, 1), strides=(0, 0, 0, 0, 0, 0),
              ldw=None, ld_rb=None):
    from fie_amd import hip
    P = hip._p
    ctx.sync_stream()
    hip._chk(hip.lib().fie_gemm_f32(ctx.h, P(a1), a1.stride(0), K1, P(a2), a2.stride(0) if a2 is not None else 0, P(w), w.stride(0) if ldw is None else ldw,
                                    int(w_kn), P(out), out.stride(0), M, N, K, P(bias), P(rb), (rb.stride(0) if rb is not None else 0) if ld_rb is None else ld_rb,
                                    rpb, P(res), res.stride(0) if res is not None else 0, float(scale), act, nb[0], nb[1], *strides))


def _run_gemm(ctx, case, inplace=False, c0=0, extra_cols=0):
    """One fie_gemm_f32 launch on a gemm_case with every operand strided; returns (out view, Out)."""
    M, N, K, K1, act = case["M"], case["N"], case["K"], case["K1"], case["act"]
    nout = N // 2 if act == fc.ACT_GEGLU else N
    a1, a2, w = _wide(case["a1"], 3), _wide(case["a2"], 6), _wide(case["w"], 5)
    assert a2 is None or a1.stride(0) != a2.stride(0)
    rb, res = _wide(case["rowbias"], 9), case["residual"]
    o = Out(M, nout, _ld(nout + c0 + extra_cols, 2), c0, init=res if inplace else None)
    resv = o.view if inplace else _wide(res, 7)
    _gemm_raw(ctx, a1, a2, K1, w, 0, o.view, M, N, K, case["bias"], rb, case["rpb"], resv if res is not None else None, case["scale"], act)
    assert all(v is None or v.stride(0) % 4 for v in (a1, a2, w, rb, resv, o.view)) and (rb is None or rb.stride(0) > N)
    return o.view, o


def _check_case(out, case, h, habs, tag, worst, fails):
    """The pass's checker on one output; worst: {'f32': (ratio, tag), 'act': ...}."""
    act, scale, res = case["act"], case["scale"], case["residual"]
    if case["integer"]:
        if act in (fc.ACT_NONE, fc.ACT_RELU):
            ref, _ = fc.finish64(h, habs, case)
            n, where = fc.exact32_mismatches(out, ref)
            if n:
                i = where[0]
                fails.append(f"{tag}: {n} elements differ from the exact result, first at {i}: out {float(out[i])} ref {float(ref[i])}")
        else:
            r = fc.act32_ratio(out, h, act, scale, res)
            if r > worst["act"][0]:
                worst["act"] = (r, tag)
            if r > C_ACT32:
                n, where = fc.act32_mismatches(out, h, act, C_ACT32, scale, res)
                fails.append(f"{tag}: activation ratio {r:.2f} > {C_ACT32} at {n} elements, first at {where}")
    else:
        ref, budget = fc.finish64(h, habs, case)
        r = fc.ratio32(out, ref, budget, case["K"], res)
        if r > worst["f32"][0]:
            worst["f32"] = (r, tag)
        if r > C_F32:
            n, where = fc.mismatches32(out, ref, budget, case["K"], C_F32, res)
            fails.append(f"{tag}: ratio {r:.2f} > {C_F32} at {n} elements, first at {where}")


def _report(name, worst, fails, n):
    for key, const in (("f32", C_F32), ("act", C_ACT32)):
        if worst[key][1] is not None:
            print(f"\n[f32 {name}] worst {key} ratio {worst[key][0]:.3f} (constant {const}) at {worst[key][1]}")
    for f in fails:
        print(f"[f32 {name}] FAIL {f}")
    assert not fails, f"{len(fails)} of {n} launches failed (printed above)"


def _variants(i, M):
    """The epilogues one triple runs: (bias, rpb, residual, in place, scale, act)."""
    rpb = next(r for r in RPBS[i % 4:] + RPBS[:i % 4] if M % r or r == 1)
    return [(True, 0, False, False, 1.0, fc.ACT_NONE),
            (True, rpb, True, i % 2 == 0, 0.5, fc.ACT_RELU),
            (True, 0, i % 3 == 0, False, 2.0, (fc.ACT_SILU, fc.ACT_GELU, fc.ACT_QUICK_GELU)[i % 3]),
            (False, RPBS[(i + 1) % 4], False, False, 1.0, (fc.ACT_GELU, fc.ACT_QUICK_GELU, fc.ACT_SILU, fc.ACT_NONE)[i % 4])]


# ------------------------------------------------------------------------------------------------------------------ GEMM
@pytest.mark.parametrize("integer", [True, False], ids=["integer", "real"])
def test_gemm_every_tile_edge_and_epilogue(f32, integer):
    worst, fails, n = {"f32": (0.0, None), "act": (0.0, None)}, [], 0
    acts, rpbs = set(), set()
    for i, (M, N, K) in enumerate(TRIPLES):
        for bias, rpb, res, inplace, scale, act in _variants(i, M):
            case = fc.gemm_case(M, N, K, _gen(1000 + 7 * i + act), integer, bias=bias, rpb=rpb, residual=res, scale=scale, act=act)
            h, habs = fc.gemm_ref64(case)
            out, o = _run_gemm(f32, case, inplace=inplace and res)
            n += 1
            acts.add(act)
            rpbs.add(rpb)
            tag = f"M={M} N={N} K={K} bias={bias} rpb={rpb} residual={'in place' if inplace and res else res} scale={scale} act={act}"
            assert o.untouched(), f"{tag}: the padding behind the output rows was written"
            _check_case(out, case, h, habs, tag, worst, fails)
    assert acts == {0, 1, 2, 3, 5} and {1, 7, 64, 100} <= rpbs
    _report("gemm integer" if integer else "gemm real", worst, fails, n)


@pytest.mark.parametrize("integer", [True, False], ids=["integer", "real"])
def test_gemm_geglu_pairs(f32, integer):
    """(value, gate) column pairs at N = 2, 66, 130: N / 2 columns written, the column behind them not."""
    worst, fails, n = {"f32": (0.0, None), "act": (0.0, None)}, [], 0
    for i, (M, N, K) in enumerate(GEGLU_SHAPES):
        for bias, rpb, scale in [(True, 0, 1.0), (i % 2 == 0, 7, 0.5)]:
            case = fc.gemm_case(M, N, K, _gen(2000 + 3 * i + rpb), integer, bias=bias, rpb=rpb, scale=scale, act=fc.ACT_GEGLU)
            h, habs = fc.gemm_ref64(case)
            out, o = _run_gemm(f32, case)
            n += 1
            tag = f"GEGLU M={M} N={N} K={K} bias={bias} rpb={rpb} scale={scale}"
            assert out.shape[1] == N // 2 and o.untouched(), f"{tag}: a column past N / 2 was written"
            _check_case(out, case, h, habs, tag, worst, fails)
    _report("geglu integer" if integer else "geglu real", worst, fails, n)


@pytest.mark.parametrize("integer", [True, False], ids=["integer", "real"])
def test_gemm_concat_seam(f32, integer):
    """A = [A1 | A2] with K1 in {1, 15, 16, 17}, K2 in {1, 16, 23} and lda1 != lda2."""
    worst, fails = {"f32": (0.0, None), "act": (0.0, None)}, []
    for i, (k1, k2) in enumerate(CONCAT):
        M, N = (65, 3, 129)[i % 3], (65, 64, 2)[i % 3]
        case = fc.gemm_case(M, N, k1 + k2, _gen(3000 + i), integer, K1=k1, bias=i % 2 == 0, act=fc.ACT_RELU if i % 4 == 1 else fc.ACT_NONE)
        h, habs = fc.gemm_ref64(case)
        out, o = _run_gemm(f32, case)
        tag = f"concat K1={k1} K2={k2} M={M} N={N}"
        assert o.untouched(), tag
        _check_case(out, case, h, habs, tag, worst, fails)
    _report("concat integer" if integer else "concat real", worst, fails, len(CONCAT))


@pytest.mark.parametrize("integer", [True, False], ids=["integer", "real"])
def test_gemm_output_as_a_column_range(f32, integer):
    """The Fire modules' form (fie_amd/lpips.py): the op writes columns [c0, c0 + N) of a wider tensor through the wrapper; the neighbours keep their bits."""
    from fie_amd import hip
    worst, fails = {"f32": (0.0, None), "act": (0.0, None)}, []
    for i, (M, N, K, c0, tail) in enumerate([(65, 64, 16, 64, 0), (129, 3, 33, 1, 2), (63, 65, 200, 0, 65), (1, 130, 5, 7, 1)]):
        case = fc.gemm_case(M, N, K, _gen(4000 + i), integer, bias=True, act=fc.ACT_RELU)
        h, habs = fc.gemm_ref64(case)
        o = Out(M, N, c0 + N + tail + 1, c0)
        got = f32.gemm_f32(_wide(case["a1"], 3), case["w"], N, out=o.view, bias=case["bias"], act=hip.ACT_RELU)
        assert got is o.view
        tag = f"column range M={M} N={N} K={K} c0={c0} of {o.buf.shape[1]}"
        assert o.untouched(), f"{tag}: a neighbouring column was written"
        _check_case(o.view, case, h, habs, tag, worst, fails)
    _report("column range", worst, fails, 4)


def _kn_case(M, N, K, integer, gen):
    """The P V product of hip.Context.attention: A [nb1 * nb2, M, K] (lda = K), W = V [nb1 * K, nb2 * N (+ pad)] read as [K][N] per (z1, z2), C [nb1 * M, nb2 * N (+ pad)]."""
    nb1, nb2 = 2, 3
    if integer:
        a = torch.randint(-2, 3, (nb1 * nb2, M, K), generator=gen, device=DEV).float()
        v = torch.randint(-2, 3, (nb1 * K, nb2 * N), generator=gen, device=DEV).float()
    else:
        a = torch.randn((nb1 * nb2, M, K), generator=gen, device=DEV) + 0.25
        v = (torch.randn((nb1 * K, nb2 * N), generator=gen, device=DEV) + 0.25) / math.sqrt(K)
    return a, v


@pytest.mark.parametrize("integer", [True, False], ids=["integer", "real"])
def test_gemm_kn_weights_two_level_batch(f32, integer):
    """w_is_kn = 1 over a 2 x 3 batch with the strides attention() passes for P V: K in {1, 63, 65, 200} (Tk % 16 != 0), N in {40, 64, 72}."""
    nb1, nb2 = 2, 3
    worst, fails = {"f32": (0.0, None), "act": (0.0, None)}, []
    for i, (M, N, K) in enumerate(KN_SHAPES):
        a, v = _kn_case(M, N, K, integer, _gen(5000 + i))
        vw = _wide(v, 5)
        o = Out(nb1 * M, nb2 * N, _ld(nb2 * N, 6))
        _gemm_raw(f32, a.view(-1, K), None, K, vw, 1, o.view, M, N, K, nb=(nb1, nb2),
                  strides=(nb2 * M * K, M * K, K * vw.stride(0), N, M * o.view.stride(0), N))
        tag = f"[K][N] batch M={M} N={N} K={K}"
        assert o.untouched(), tag
        for z1 in range(nb1):
            for z2 in range(nb2):
                az, wz = a[z1 * nb2 + z2], v[z1 * K:(z1 + 1) * K, z2 * N:(z2 + 1) * N].t()
                case = {"a1": az, "a2": None, "w": wz, "bias": None, "rowbias": None, "residual": None, "act": 0, "scale": 1.0, "K": K, "integer": integer}
                h, habs = fc.gemm_ref64(case)
                _check_case(o.view[z1 * M:(z1 + 1) * M, z2 * N:(z2 + 1) * N], case, h, habs, f"{tag} z1={z1} z2={z2}", worst, fails)
    _report("[K][N] batch", worst, fails, len(KN_SHAPES))


def test_gemm_against_the_fp32_fma_chain(f32):
    """csrc/f32.hip's header: the MFMA accumulates as a k-ascending fp32 FMA chain.  On the real-data GEMMs (no epilogue) every element is compared
    with f32_check.fma_chain32, and separately with the float64 sum rounded once (which a chain is not)."""
    total, equal, once, rows = 0, 0, 0, []
    for i, (M, N, K) in enumerate(TRIPLES):
        case = fc.gemm_case(M, N, K, _gen(6000 + i), False)
        out, _ = _run_gemm(f32, case)
        chain = fc.fma_chain32(case["a1"], case["w"])
        h, _ = fc.gemm_ref64(case)
        eq = int((out == chain).sum())
        total, equal, once = total + out.numel(), equal + eq, once + int((out == h.float()).sum())
        if eq != out.numel():
            rows.append(f"M={M} N={N} K={K}: {out.numel() - eq} of {out.numel()} elements differ from the chain, worst by "
                        f"{float(((out.double() - chain.double()).abs() / an.ulp32(chain.double())).max()):.1f} ulp32")
    print(f"\n[f32 chain] {equal} of {total} elements equal the k-ascending fp32 FMA chain ({once} equal the float64 sum rounded once)")
    for r in rows:
        print(f"[f32 chain] {r}")
    assert equal == total, f"{total - equal} of {total} elements are not the k-ascending fp32 FMA chain (printed above)"


# ------------------------------------------------------------------------------------------------------------------ conv
def _run_conv(ctx, case, raw, crange, res_wide=True):
    """One launch on a conv_case: through pack_conv3x3 of the fp32 context (Cin padded to 8 in the weights and in x) or with raw [Cout][9 Cin] weights,
    ldw > 9 Cin.  Returns (out [M, Cout] view, Out)."""
    from fie_amd import hip
    P = hip._p
    x, w4 = case["x"], case["w4"]
    b, hh, ww, cin = x.shape
    cout, geo = case["N"], fc.conv_geo(case)
    oh, ow, m = geo["OH"], geo["OW"], case["M"]
    c0 = 5 if crange else 0
    o = Out(m, cout, _ld(c0 + cout + (3 if crange else 0), 2), c0)
    res = _wide(case["residual"], 7)
    rb = _wide(case["rowbias"], 9)
    if raw:
        wbuf = _wide(case["w"], 5)
        ctx.sync_stream()
        hip._chk(hip.lib().fie_conv3x3_nhwc_f32(ctx.h, P(x), b, hh, ww, cin, int(case["ups"]), case["stride"], case["pad_mode"], P(wbuf), wbuf.stride(0),
                                                P(o.view), o.view.stride(0), cout, P(case["bias"]), P(rb), rb.stride(0) if rb is not None else 0,
                                                P(res), res.stride(0) if res is not None else 0, float(case["scale"]), case["act"]))
    else:
        wp = ctx.pack_conv3x3(w4)
        cp = wp.shape[1] // 9
        assert cp == (cin + 7) // 8 * 8 and wp.dtype == torch.float32
        xp = torch.zeros((b, hh, ww, cp), device=DEV, dtype=torch.float32)
        xp[..., :cin] = x
        view4 = lambda t: None if t is None else torch.as_strided(t, (b, oh, ow, t.shape[1]), (oh * ow * t.stride(0), ow * t.stride(0), t.stride(0), 1), t.storage_offset())
        got = ctx.conv3x3(xp, wp, cout, out=view4(o.view), stride=case["stride"], pad_mode=case["pad_mode"], upsample=case["ups"], bias=case["bias"],
                          rowbias=rb, residual=view4(res), scale=case["scale"], act=case["act"])
        assert got.data_ptr() == o.view.data_ptr()
    return o.view, o


@pytest.mark.parametrize("integer", [True, False], ids=["integer", "real"])
def test_conv_every_geometry_and_epilogue(f32, integer):
    worst, fails = {"f32": (0.0, None), "act": (0.0, None)}, []
    seen = set()
    for i, (hh, ww, cin, cout, stride, pad_mode, ups, raw, bias, rowbias, res, crange, scale, act) in enumerate(CONVS):
        case = fc.conv_case(B, hh, ww, cin, cout, _gen(7000 + i), integer, stride=stride, pad_mode=pad_mode, ups=ups, bias=bias, rowbias=rowbias,
                            residual=res, scale=scale, act=act)
        h, habs = fc.conv_ref64(case)
        out, o = _run_conv(f32, case, raw, crange)
        tag = (f"conv {hh}x{ww} Cin={cin} Cout={cout} stride={stride} pad_mode={pad_mode} ups={ups} {'raw' if raw else 'packed'} weights bias={bias} "
               f"rowbias={rowbias} residual={res} channel range={crange} scale={scale} act={act}")
        assert o.untouched(), f"{tag}: a neighbouring channel was written"
        seen |= {("cin", cin), ("cout", cout), ("map", hh, ww), ("stride", stride), ("pad", pad_mode), ("ups", ups), ("raw", raw)}
        _check_case(out, case, h, habs, tag, worst, fails)
    assert {("cin", c) for c in (4, 8, 24, 40)} | {("cout", c) for c in (1, 24, 65)} | {("map", 1, 1), ("map", 1, 5), ("map", 2, 3), ("map", 9, 7), ("map", 16, 16)} <= seen
    _report("conv integer" if integer else "conv real", worst, fails, len(CONVS))


# ------------------------------------------------------------------------------------------------------------------ softmax
def _softmax(ctx, s, cols, ld, scale, causal, tq):
    from fie_amd import hip
    ctx.sync_stream()
    hip._chk(hip.lib().fie_softmax_rows_f32(ctx.h, hip._p(s), s.shape[0], cols, ld, float(scale), int(causal), tq))


def _run_softmax(ctx, s, scale, causal, tq):
    rows, cols = s.shape
    o = Out(rows, cols, _ld(cols, 3), init=s)
    _softmax(ctx, o.view, cols, o.view.stride(0), scale, causal, tq)
    return o.view, o


def test_softmax_rows_per_element(f32):
    """rows in {1, 5, 7, 130} (four rows per block) x cols in {1, 63, 64, 65, 77, 200, 1025}, ld > cols; scale 1 and 64^-0.5; causal with tq in {1, 7, 77}."""
    worst, fails, n = (0.0, None), [], 0
    for ri, rows in enumerate(SM_ROWS):
        for ci, cols in enumerate(SM_COLS):
            s = torch.randn((rows, cols), generator=_gen(8000 + 10 * ri + ci), device=DEV) * 3.0
            s[0] = float(ci - 3)                                                  # a constant row: every visible output is 1 / count
            for scale, causal, tq in [(1.0, False, 1), (0.125, True, SM_TQ[(ri + ci) % 3]), (1.0, True, SM_TQ[(ri + ci + 1) % 3])]:
                ref, weight, hidden = fc.softmax_ref64(s, scale, causal, tq)
                out, o = _run_softmax(f32, s, scale, causal, tq)
                n += 1
                tag = f"softmax rows={rows} cols={cols} scale={scale} causal={causal} tq={tq}"
                assert o.untouched(), f"{tag}: columns [cols, ld) were written"
                r = fc.softmax_ratio(out, ref, weight, hidden)
                if r > worst[0]:
                    worst = (r, tag)
                if r > C_SM:
                    k, where = fc.softmax_mismatches(out, ref, weight, hidden, C_SM)
                    fails.append(f"{tag}: ratio {r:.2f} > {C_SM} at {k} elements, first at {where}")
    print(f"\n[f32 softmax] worst ratio {worst[0]:.3f} (C_SM = {C_SM}) at {worst[1]}")
    for f in fails:
        print(f"[f32 softmax] FAIL {f}")
    assert not fails, f"{len(fails)} of {n} launches failed (printed above)"


def test_softmax_dominant_and_constant_rows(f32):
    """One score leads by 256: every other weight underflows, the row is exactly one-hot.  Constant rows: 1 / count, exact for a power of two."""
    for rows, cols in [(5, 65), (7, 200), (130, 1025), (5, 64)]:
        s = torch.randn((rows, cols), generator=_gen(8500 + cols), device=DEV)
        win = (torch.arange(rows, device=DEV) * 37 + cols - 1) % cols
        s[torch.arange(rows, device=DEV), win] = 256.0
        out, o = _run_softmax(f32, s, 1.0, False, 1)
        onehot = torch.zeros_like(s)
        onehot[torch.arange(rows, device=DEV), win] = 1.0
        assert o.untouched() and bool((out.contiguous().view(torch.int32) == onehot.view(torch.int32)).all()), (rows, cols)
        const = torch.full((rows, cols), -3.0, device=DEV)
        out, o = _run_softmax(f32, const, 0.125, True, 7)
        count = torch.clamp(torch.arange(rows, device=DEV) % 7 + 1, max=cols)
        ref, weight, hidden = fc.softmax_ref64(const, 0.125, True, 7)
        assert float((ref - (1.0 / count.double())[:, None]).abs()[~hidden].max()) < 1e-15
        assert fc.softmax_mismatches(out, ref, weight, hidden, C_SM)[0] == 0
        pow2 = ((count & (count - 1)) == 0)[:, None] & ~hidden
        assert bool((out[pow2] == ref.float()[pow2]).all()), "a power-of-two count is exact"


# ------------------------------------------------------------------------------------------------------------------ attention
def _rows(t):
    b, h, n, d = t.shape
    return t.permute(0, 2, 1, 3).reshape(b * n, h * d).contiguous()


def _run_attention(ctx, case, fused=False, pad=0):
    """One attention() on the case's q, k, v ([B, H, T, D]); fused: column slices of one [B T, 3 C] buffer; pad: columns behind the output rows, which must
    keep their fill.  Returns [B, H, Tq, D]."""
    q, k, v = case["q"], case["k"], case["v"]
    b, h, tq, d = q.shape
    tk, c = k.shape[2], h * d
    if fused:
        assert tq == tk
        buf = torch.cat([_rows(q), _rows(k), _rows(v)], 1).contiguous()
        q2, k2, v2 = buf[:, :c], buf[:, c:2 * c], buf[:, 2 * c:]
    else:
        q2, k2, v2 = _wide(_rows(q), 3), _wide(_rows(k), 6), _wide(_rows(v), 9)
    o = Out(b * tq, c, c + pad)
    got = ctx.attention(q2, k2, v2, h, d, tq, tk, b, out=o.view, causal=case["causal"], scale=case["scale"])
    assert got is o.view and o.untouched(), "the padding behind the output rows was written"
    return o.view.reshape(b, tq, h, d).permute(0, 2, 1, 3)


_CASES = {}


def _exact_cases(tq, tk, d):
    key = (tq, tk, d)
    if key not in _CASES:
        c = 16.0 if d == 40 else 8.0                       # uniform: an unmasked zero key would lead by GAP_MIN at every d
        out = {"selector": (fc.selector32(B, H, tq, tk, d, _gen(tq * 4099 + tk + d)), "pick"),
               "ramp": (fc.ramp32(B, H, tq, tk, d, False, DEV), "pick"),
               "ramp causal": (fc.ramp32(B, H, tq, tk, d, True, DEV), "pick")}
        for cc in (0.0, -c, c):
            out[f"uniform c={cc:g}"] = (fc.uniform32(B, H, tq, tk, d, cc, False, DEV), "uniform")
        out["uniform causal"] = (fc.uniform32(B, H, tq, tk, d, -c, True, DEV), "uniform")
        if (tq, tk) in ((77, 77), (77, 333)):              # an explicit scale other than d^-0.5 (a power of two: the scaled scores stay exact)
            out["selector scale"] = (fc.selector32(B, H, tq, tk, d, _gen(7), scale=0.25), "pick")
            out["ramp causal scale"] = (fc.ramp32(B, H, tq, tk, d, True, DEV, scale=0.0625), "pick")
            out["uniform scale"] = (fc.uniform32(B, H, tq, tk, d, -c, False, DEV, scale=0.25), "uniform")
        _CASES[key] = out
    return _CASES[key]


@pytest.mark.parametrize("tq,tk,d", PAIRS)
def test_attention_exact_cases(f32, tq, tk, d):
    fails, n = [], 0
    for ci, (name, (case, kind)) in enumerate(_exact_cases(tq, tk, d).items()):
        fused, pad = (tq == tk and ci % 2 == 0), (9 if ci % 2 else 0)
        out = _run_attention(f32, case, fused=fused, pad=pad)
        n += 1
        tag = f"d={d} Tq={tq} Tk={tk} {name}{' fused-qkv' if fused else ''}{' padded-out' if pad else ''}"
        if kind == "pick":
            bad, where = fc.exact32_mismatches(out, case["expect"].double())
            if bad:
                fails.append(f"{tag}: {bad} elements differ, first {an.describe_pick(out, case, where[0])}")
        else:
            bad, where = fc.uniform32_mismatches(out, case, C_ATTN32)
            if bad:
                i = where[0]
                fails.append(f"{tag}: {bad} elements off, first at {i}: out {float(out[i])} ref {float(case['ref'][i]):.9f} (count {int(case['count'][i[2]])})")
    for f in fails:
        print(f"[f32 attn exact] FAIL {f}")
    assert not fails, f"{len(fails)} of {n} exact cases failed (printed above)"


def test_attention_real_data_per_element(f32):
    worst, fails, n = (0.0, None), [], 0
    for pi, (tq, tk, d) in enumerate(PAIRS):
        for peaky in (False, True):
            for causal in ([False, True] if (tq, tk, d) in CAUSAL else [False]):
                case = fc.real32(B, H, tq, tk, d, peaky, causal, _gen(9000 + 10 * pi + 2 * peaky + causal))
                ref, dev, eps, wabs = fc.attn_budget32(case["q"], case["k"], case["v"], case["scale"], causal)
                out = _run_attention(f32, case, fused=(tq == tk and not peaky), pad=5 if peaky else 0)
                n += 1
                r = fc.attn32_ratio(out, ref, dev, eps, wabs, tk)
                tag = f"d={d} Tq={tq} Tk={tk}{' peaky' if peaky else ''}{' causal' if causal else ''}"
                if r > worst[0]:
                    worst = (r, tag)
                if r > C_ATTN32:
                    k, where = fc.attn32_mismatches(out, ref, dev, eps, wabs, tk, C_ATTN32)
                    fails.append(f"{tag}: ratio {r:.2f} > {C_ATTN32} at {k} elements, first at {where}")
    print(f"\n[f32 attn real] worst ratio {worst[0]:.3f} (C_ATTN32 = {C_ATTN32}) at {worst[1]}")
    for f in fails:
        print(f"[f32 attn real] FAIL {f}")
    assert not fails, f"{len(fails)} of {n} cases beyond the per-element bound (printed above)"


def _picks(out, v):
    """[B, H, Tq]: the key whose V row equals the output row bit for bit, -1 where none does."""
    hit = (out[:, :, :, None, :] == v[:, :, None, :, :]).all(-1)
    return torch.where(hit.any(-1), hit.int().argmax(-1), torch.full(hit.shape[:-1], -1, device=out.device))


@pytest.mark.parametrize("tq,tk", [(77, 333), (200, 96)])
def test_causal_convention_matches_the_f16_kernels(fie, f32, tq, tk):
    """The fp32 path is the f16 path's on-device reference: on the causal ramp case at Tq != Tk (row i must return V[min(i, Tk - 1)]) both contexts
    pick the same key in every row."""
    c16 = an.ramp_case(B, H, tq, tk, 64, True, DEV)
    c = H * 64
    o16 = fie.attention(_rows(c16["q"]), _rows(c16["k"]), _rows(c16["v"]), H, 64, tq, tk, B, causal=True, scale=c16["scale"])
    p16 = _picks(o16.reshape(B, tq, H, 64).permute(0, 2, 1, 3), c16["v"])
    c32 = fc.ramp32(B, H, tq, tk, 64, True, DEV)
    p32 = _picks(_run_attention(f32, c32), c32["v"])
    assert bool((p16 >= 0).all()) and bool((p32 >= 0).all()), "a row is no key's V"
    assert bool((p16 == p32).all()) and bool((p32 == c32["pi"]).all()), f"first rows that differ: {lc._where(p16 != p32)}"
    assert c == o16.shape[1]


# ------------------------------------------------------------------------------------------------------------------ refusals
def test_every_refusal_leaves_the_output_untouched(f32):
    from fie_amd import hip
    P, L = hip._p, hip.lib()
    M, N, K = 5, 6, 7
    a, a2, w = (torch.ones((M, K), device=DEV), torch.ones((M, 3), device=DEV), torch.ones((N, K + 3), device=DEV))
    vec, rb, res = torch.ones(N, device=DEV), torch.ones((M, N), device=DEV), torch.ones((M, N), device=DEV)
    o = Out(M, N, N + 3)

    def gemm(match, **kw):
        arg = dict(a1=a, a2=None, K1=K, w=w, w_kn=0, out=o.view, M=M, N=N, K=K)
        arg.update(kw)
        with pytest.raises(hip.FieError, match=match):
            _gemm_raw(f32, **arg)
        torch.cuda.synchronize()
        assert o.unwritten(), f"a refused call ({match}) wrote its output"

    gemm("bad epilogue", act=fc.ACT_GEGLU, res=res)
    gemm("bad epilogue", act=fc.ACT_GEGLU, N=5)
    gemm("bad epilogue", act=6)
    gemm("bad shape", K1=K + 1)
    gemm("bad shape", K1=K - 3)                                            # K1 < K without A2
    gemm("bad shape", K=0, K1=0)
    gemm("rowbias needs rows_per_batch", rb=rb, rpb=0)
    gemm("bad batch", nb=(256, 256))
    gemm("bad batch", nb=(0, 1))
    gemm(rf"M={65535 * 64 + 1} rows exceed the {65535 * 64}", M=65535 * 64 + 1)       # the check fires before any memory is touched
    x, wc = torch.ones((1, 3, 3, 4), device=DEV), torch.ones((N, 40), device=DEV)
    oc = Out(9, N, N + 3)

    def conv(match, b=1, hh=3, ww=3, cin=4, stride=1, pad_mode=0, ldw=40, act=0):
        f32.sync_stream()
        with pytest.raises(hip.FieError, match=match):
            hip._chk(L.fie_conv3x3_nhwc_f32(f32.h, P(x), b, hh, ww, cin, 0, stride, pad_mode, P(wc), ldw, P(oc.view), oc.view.stride(0), N, P(vec), None, 0, None, 0,
                                            1.0, act))
        torch.cuda.synchronize()
        assert oc.unwritten(), f"a refused call ({match}) wrote its output"

    conv("bad argument", ldw=35)
    conv("bad argument", stride=3)
    conv("bad argument", pad_mode=2)
    conv("bad argument", act=fc.ACT_GEGLU)
    conv("a 1 x 3 map has no output pixel with pad_mode 1", hh=1, pad_mode=1, stride=2)      # (1 + 1 - 3) / 2 truncates to 0 in C: one row would be written
    conv(rf"M={4097 * 1024} output pixels .* exceed the {65535 * 64}", b=4097, hh=32, ww=32)
    s = Out(4, 8, 11)
    for kw in (dict(ld=7), dict(tq=0), dict(cols=0)):
        arg = dict(cols=8, ld=11, tq=4)
        arg.update(kw)
        with pytest.raises(hip.FieError, match="fie_softmax_rows_f32: bad argument"):
            _softmax(f32, s.view, arg["cols"], arg["ld"], 1.0, 1, arg["tq"])
        torch.cuda.synchronize()
        assert s.unwritten()
    # and the calls next to the refused ones run
    _gemm_raw(f32, a, a2, K, w, 0, o.view, M, N, K + 3, bias=vec, rb=rb, rpb=1, res=res)
    torch.cuda.synchronize()
    assert bool((o.view == K + 3 + 3).all()) and o.untouched()
