"""Every op stays inside its operands (tests/isolation.py): strided inputs in NaN moats, a strided output in a guarded arena, each case run twice
(NaN moats / large finite moats, two output prefills) -- the two results bit-equal and finite, the guard bytes untouched -- and the value against the same
fp32 torch reference, at the same bar, as the op's own test in test_ops_gpu.py / test_fp8_gpu.py (3e-3 GEMM / conv / norms, 4e-3 attention and the
fused conv forms, 2e-3 against the quantised reference for fp8; byte and integer outputs exact).  Every call is one the ABI documents as valid and every
access the moats are sized for stays inside a torch allocation.  Shapes: one full row tile plus three rows, N ragged at 8, K with and without a tail."""
import functools
import math
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import isolation as iso
from isolation import E4M3, flat, isolated, wide
from test_ops_gpu import SHIPPED_CODES, rel_err, rnd

pytestmark = pytest.mark.gpu

DEV = "cuda"
M, N = 259, 200


def q8(x):
    return x.float().clamp(-448.0, 448.0).to(torch.float8_e4m3fn).float()


def f8(t):
    """e4m3 bytes (uint8, any device) as fp32 values on the host."""
    return t.view(torch.float8_e4m3fn).float().cpu()


def e4m3_close(got_bytes, want, frac=0.98):
    """The bar of the e4m3 producers' own tests (test_fp8_gpu.py): a value on a rounding boundary may land one code off."""
    got = f8(got_bytes)
    return (got == want).float().mean().item() > frac and rel_err(got, want) < 0.13


def ran(fie, code, view="gemm"):
    """The kernel the last launch used carries the forced tile code (and the view)."""
    from fie_amd import hip
    kern = hip.last_gemm_kernel(fie)
    assert re.search(rf"\({view}, .*tile code {code % 1000}[,)]", kern), (code, kern)
    return kern


# ------------------------------------------------------------------------------------------------------------------------ references, computed once
@functools.lru_cache(maxsize=None)
def gemm_case(m, n, k):
    a, w, bias = rnd(m, k, seed=1), rnd(n, k, seed=2, scale=k ** -0.5), rnd(n, seed=3)
    return a, w, bias, a.float() @ w.float().T + bias.float()


@functools.lru_cache(maxsize=None)
def epilogue_case(m, n, k):
    a, w, bias, lin = gemm_case(m, n, k)
    res, rb = rnd(m, n, seed=4), rnd(2, n, seed=5)
    rpb = (m + 1) // 2
    return res, rb, rpb, F.silu(lin + rb.float().repeat_interleave(rpb, 0)[:m]) * 0.5 + res.float()


@functools.lru_cache(maxsize=None)
def geglu_case(m, n, k):
    a, w, bias, lin = gemm_case(m, n, k)
    return torch.stack([bias[: n // 2], bias[n // 2:]], 1).reshape(-1).contiguous(), lin[:, : n // 2] * F.gelu(lin[:, n // 2:])


@functools.lru_cache(maxsize=None)
def conv_case(b, h, w, cin, cout, stride, pad_mode, ups):
    x = rnd(b, h, w, cin, seed=1)
    wt = rnd(cout, cin, 3, 3, seed=2, scale=(9 * cin) ** -0.5)
    bias = rnd(cout, seed=3)
    xi = x.float().permute(0, 3, 1, 2)
    if ups:
        xi = F.interpolate(xi, scale_factor=2.0, mode="nearest")
    if pad_mode == 1:
        xi = F.pad(xi, (0, 1, 0, 1))
    ref = F.conv2d(xi, wt.float(), bias.float(), stride=stride, padding=1 if pad_mode == 0 else 0).permute(0, 2, 3, 1).contiguous()
    return x, wt, bias, ref


@functools.lru_cache(maxsize=None)
def attn_case(b, hn, tq, tk, d, causal):
    c = hn * d
    q, k, v = rnd(b * tq, c, seed=1), rnd(b * tk, c, seed=2), rnd(b * tk, c, seed=3)
    sp = lambda x, t: x.float().view(b, t, hn, d).transpose(1, 2)
    ref = F.scaled_dot_product_attention(sp(q, tq), sp(k, tk), sp(v, tk), is_causal=causal).transpose(1, 2).reshape(b * tq, c)
    return q, k, v, ref


@functools.lru_cache(maxsize=None)
def groupnorm_case(b, rows, c1, c2):
    x1 = rnd(b, rows, c1, seed=1) + 0.5
    x2 = rnd(b, rows, c2, seed=2) * 2 if c2 else None
    gamma, beta = rnd(c1 + c2, seed=3), rnd(c1 + c2, seed=4)
    xc = torch.cat([x1, x2], -1) if c2 else x1
    ref = F.silu(F.group_norm(xc.float().transpose(1, 2), 32, gamma.float(), beta.float(), 1e-5).transpose(1, 2))
    return x1, x2, gamma, beta, ref


def dev(*ts):
    out = tuple(None if t is None else t.to(DEV) for t in ts)
    return out if len(out) > 1 else out[0]


# ------------------------------------------------------------------------------------------------------------------------ self-check
def test_the_guard_sees_a_real_kernels_stores(fie):
    """A legal fie.gemm of M rows into an arena whose guard was told the view has M - 1: the write stays inside the arena and check() names row M - 1."""
    a, w, bias, ref = gemm_case(M, N, 200)
    view, guard = iso.guarded((M - 1, N), ld=N + 8, device=DEV)
    whole = torch.as_strided(view, (M, N), (N + 8, 1), view.storage_offset())
    fie.gemm(dev(a), fie.pack_linear(dev(w)), N, bias=dev(bias), out=whole)
    torch.cuda.synchronize()
    with pytest.raises(iso.GuardError, match=rf"first at \(row {M - 1}, col 0\)"):
        guard.check()
    assert rel_err(whole, ref) < 3e-3
    view, guard = iso.guarded((M, N), ld=N + 8, device=DEV)
    fie.gemm(dev(a), fie.pack_linear(dev(w)), N, bias=dev(bias), out=view)
    torch.cuda.synchronize()
    guard.check()


# ------------------------------------------------------------------------------------------------------------------------ GEMM view
@pytest.mark.parametrize("code", SHIPPED_CODES)
def test_gemm_view(fie, code):
    """Every shipped tile code, forced: M = 259 (one 256-row tile + 3; two of every smaller one), N = 200 (ragged at 8), K = 72 / 200 (a K tail) / 192;
    M = 3; bias + row bias + SiLU + scale + a strided residual; the in-place form; GEGLU; split-K where the code asks for it (K = 1032: 17 K-steps)."""
    from fie_amd import hip
    try:
        fie.force_tile(code)
        for m, k in [(M, 72), (M, 200), (M, 192), (3, 200)]:
            a, w, bias, ref = gemm_case(m, N, k)
            wp = fie.pack_linear(dev(w))
            out = isolated(lambda i, o: fie.gemm(i["a"], wp, N, bias=i["bias"], out=o), {"a": dev(a), "bias": dev(bias)}, dict(shape=(m, N), ld=N + 8))
            ran(fie, code)
            assert rel_err(out, ref) < 3e-3, (m, k)
        a, w, bias, _ = gemm_case(M, N, 200)
        res, rb, rpb, ref = epilogue_case(M, N, 200)
        wp = fie.pack_linear(dev(w))
        ins = {"a": dev(a), "bias": dev(bias), "rb": dev(rb), "res": dev(res)}
        full = lambda i, o, r: fie.gemm(i["a"], wp, N, bias=i["bias"], rowbias=i["rb"], rows_per_batch=rpb, residual=r, scale=0.5, act=hip.ACT_SILU, out=o)
        out = isolated(lambda i, o: full(i, o, i["res"]), ins, dict(shape=(M, N), ld=N + 8))
        ran(fie, code)
        assert rel_err(out, ref) < 3e-3
        inplace = isolated(lambda i, o: full(i, o.copy_(i["res"]), o), ins, dict(shape=(M, N), ld=N + 16))      # residual is out
        assert rel_err(inplace, ref) < 3e-3
        a, w, _, _ = gemm_case(M, 640, 200)
        gbias, ref = geglu_case(M, 640, 200)
        wp = fie.pack_linear(dev(w), geglu=True)
        out = isolated(lambda i, o: fie.gemm(i["a"], wp, 640, bias=i["bias"], act=hip.ACT_GEGLU, out=o), {"a": dev(a), "bias": dev(gbias)}, dict(shape=(M, 320), ld=328))
        ran(fie, code)
        assert rel_err(out, ref) < 3e-3
        if code >= 10000:
            a, w, bias, ref = gemm_case(M, N, 1032)
            res = epilogue_case(M, N, 200)[0]
            wp = fie.pack_linear(dev(w))
            out = isolated(lambda i, o: fie.gemm(i["a"], wp, N, bias=i["bias"], residual=i["res"], out=o), {"a": dev(a), "bias": dev(bias), "res": dev(res)},
                           dict(shape=(M, N), ld=N + 8))
            assert f"split-K {code // 10000})" in ran(fie, code)
            assert rel_err(out, ref + res.float()) < 3e-3
            assert fie.splitk_counters_clear()
    finally:
        fie.force_tile(0)


@pytest.mark.parametrize("code,n,geglu", [(42, N, False), (96, N, False), (64, 640, True)])
def test_gemm_with_layernorm_folded_in(fie, code, n, geglu):
    from fie_amd import hip
    k = 640
    x = rnd(M, k, seed=1) * 2 + rnd(M, 1, seed=7) * 6
    w, b = rnd(n, k, seed=2) / math.sqrt(k), rnd(n, seed=3) * 0.1
    g, bta = 1 + 0.2 * rnd(k, seed=4), 0.1 * rnd(k, seed=5)
    y = F.layer_norm(x.float(), (k,), g.float(), bta.float(), 1e-5) @ w.float().t() + b.float()
    ref = y[:, : n // 2] * F.gelu(y[:, n // 2:]) if geglu else y
    wp, tab = fie.fold_layernorm(w, b, g, bta, geglu=geglu)
    nout = n // 2 if geglu else n
    try:
        fie.force_tile(code)
        out = isolated(lambda i, o: fie.gemm_ln(i["x"], wp, n, i["tab"], act=hip.ACT_GEGLU if geglu else hip.ACT_NONE, out=o), {"x": dev(x), "tab": flat(tab)},
                       dict(shape=(M, nout), ld=nout + 8))
        ran(fie, code)
    finally:
        fie.force_tile(0)
    assert rel_err(out, ref) < 3e-3


# ------------------------------------------------------------------------------------------------------------------------ A = [A1 | A2]
CONCAT = [(128, 64), (128, 72), (64, 8), (72, 64)]


@pytest.mark.parametrize("k1,k2", CONCAT)
def test_gemm_concat_a(fie, k1, k2):
    """A = [A1 | A2] with the seam and the end of K on and off the 64-column K-step.  The LDS-DMA kernels issue a partial last K-step from A1's
    descriptor, so they take K1 < K only with K1 % 64 == 0 AND K % 64 == 0; every other pair runs on the generic kernels, and a forced LDS-DMA
    code is refused by name instead of reading A1 where A2's tail is."""
    from fie_amd import hip
    a1, a2, w = rnd(M, k1, seed=1), rnd(M, k2, seed=2), rnd(N, k1 + k2, seed=3, scale=(k1 + k2) ** -0.5)
    ref = torch.cat([a1, a2], 1).float() @ w.float().T
    wp = fie.pack_linear(dev(w))
    fn = lambda i, o: fie.gemm(i["a1"], wp, N, a2=i["a2"], out=o)
    ins = {"a1": wide(dev(a1), 64), "a2": wide(dev(a2), 128)}
    spec = dict(shape=(M, N), ld=N + 8)
    dma = k1 % 64 == 0 and (k1 + k2) % 64 == 0
    out = isolated(fn, ins, spec)
    kern = hip.last_gemm_kernel(fie)
    assert kern.startswith("gemm_kernel<") == (not dma), kern      # the generic family for every pair the LDS-DMA kernels cannot address
    assert rel_err(out, ref) < 3e-3
    try:
        for code in (2, 42, 52, 96, 81):
            fie.force_tile(code)
            if dma or code == 2:
                assert rel_err(isolated(fn, ins, spec), ref) < 3e-3, code
                ran(fie, code)
            else:
                with pytest.raises(hip.FieError, match=r"not eligible for the LDS-DMA kernels .*K1 % 64 != 0 or K % 64 != 0"):
                    fn({"a1": dev(a1), "a2": dev(a2)}, torch.empty(M, N, device=DEV, dtype=torch.float16))
    finally:
        fie.force_tile(0)


@pytest.mark.parametrize("k1,k2", CONCAT)
def test_gemm_concat_a_fp8_weights(fie, k1, k2):
    """The fp8-weight GEMM has LDS-DMA kernels only: the pairs they cannot address are refused by name (FIE_EINVAL), the others match the quantised reference."""
    from fie_amd import hip
    a1, a2, w = rnd(M, k1, seed=1), rnd(M, k2, seed=2), rnd(N, k1 + k2, seed=3, scale=(k1 + k2) ** -0.5)
    fie.w8 = True
    try:
        wp = fie.pack_linear(dev(w))
    finally:
        fie.w8 = False
    fn = lambda i, o: fie.gemm(i["a1"], wp, N, a2=i["a2"], out=o)
    if k1 % 64 == 0 and (k1 + k2) % 64 == 0:
        out = isolated(fn, {"a1": wide(dev(a1), 64), "a2": wide(dev(a2), 128)}, dict(shape=(M, N), ld=N + 8))
        assert "fp8 weights" in hip.last_gemm_kernel(fie)
        assert rel_err(out, q8(torch.cat([a1, a2], 1)) @ f8(wp.q)[:N, :k1 + k2].T * wp.scale[:N].cpu()) < 2e-3
    else:
        with pytest.raises(hip.FieError, match=r"fp8 weights: shape not eligible for the LDS-DMA kernels .*K1 % 64 != 0 or K % 64 != 0"):
            fn({"a1": dev(a1), "a2": dev(a2)}, torch.empty(M, N, device=DEV, dtype=torch.float16))


# ------------------------------------------------------------------------------------------------------------------------ conv view
def conv_isolated(fie, case, cout, ldc=None, **kw):
    x, wt, bias, ref = conv_case(*case)
    wp = kw.pop("wp", None) or fie.pack_conv3x3(dev(wt))
    b, cin = case[0], case[3]
    stride, pad_mode, ups = case[5:]
    out = isolated(lambda i, o: fie.conv3x3(i["x"], wp, cout, out=o, stride=stride, pad_mode=pad_mode, upsample=ups, bias=i["bias"], **kw),
                   {"x": flat(dev(x)), "bias": dev(bias)}, dict(shape=tuple(ref.shape), ld=ldc or cout + 8))
    return out, ref


@pytest.mark.parametrize("code", SHIPPED_CODES)
def test_conv_view(fie, code):
    """Two 9x7 images, 64 -> 72 channels (M = 126 / 40: ragged row tiles; N ragged at 8; the moats directly before image 0 and behind image 1 catch a
    padding tap that addresses a neighbour): stride 1 and 2, the asymmetric pad at both, the fused upsample, Cout = 4; ldc = Cout + 8 throughout.
    The padded-Cin case (8 channels) runs on the generic codes; an LDS-DMA code refuses it by name."""
    from fie_amd import hip
    try:
        fie.force_tile(code)
        for case in [(2, 9, 7, 64, 72, 1, 0, False), (2, 9, 7, 64, 72, 2, 0, False), (2, 9, 7, 64, 72, 2, 1, False), (2, 9, 7, 64, 72, 1, 1, False),
                     (1, 8, 8, 64, 128, 1, 0, True), (2, 9, 7, 64, 4, 1, 0, False)]:
            out, ref = conv_isolated(fie, case, case[4])
            ran(fie, code, "conv3x3")
            assert rel_err(out, ref) < 3e-3, case
        case = (2, 9, 7, 8, 32, 1, 0, False)
        if code % 1000 < 40:
            out, ref = conv_isolated(fie, case, 32)
            ran(fie, code, "conv3x3")
            assert rel_err(out, ref) < 3e-3, case
        else:
            with pytest.raises(hip.FieError, match="not eligible"):
                conv_isolated(fie, case, 32)
    finally:
        fie.force_tile(0)


@pytest.mark.parametrize("code", [0, 77])
def test_conv_by_rule_padded_cin_and_thin(fie, code):
    from fie_amd import hip
    try:
        fie.force_tile(code)
        out, ref = conv_isolated(fie, (2, 9, 7, 64, 4, 1, 0, False), 4)
        if code == 77:
            assert "conv_thin_kernel" in hip.last_gemm_kernel(fie)
        assert rel_err(out, ref) < 3e-3
        out, ref = conv_isolated(fie, (2, 9, 7, 64, 4, 2, 1, False), 4)
        assert rel_err(out, ref) < 3e-3
        if code == 0:
            out, ref = conv_isolated(fie, (2, 9, 7, 8, 32, 1, 0, False), 32)
            assert hip.last_gemm_kernel(fie).startswith("gemm_kernel<") and rel_err(out, ref) < 3e-3
    finally:
        fie.force_tile(0)


@pytest.mark.parametrize("code,case", [(71, (1, 16, 32, 64, 64, 1, 0, False)), (72, (1, 16, 32, 64, 64, 1, 0, False)), (78, (1, 24, 20, 128, 64, 1, 0, False))])
def test_halo_resident_conv(fie, code, case):
    """The halo-resident kernels: every border pixel's halo lies outside the image (above row 0 and below the last row: in the moat).  Tile code 78
    takes Cin >= 128 only: 64 input channels are refused by name, the edge-patch map runs at 128."""
    from fie_amd import hip
    try:
        fie.force_tile(code)
        if code == 78:
            with pytest.raises(hip.FieError, match="edge patches"):
                conv_isolated(fie, (1, 24, 20, 64, 64, 1, 0, False), 64)
        out, ref = conv_isolated(fie, case, case[4])
        assert hip.last_gemm_kernel(fie).startswith("conv_halo") and f"tile code {code}" in hip.last_gemm_kernel(fie)
        assert rel_err(out, ref) < 3e-3
    finally:
        fie.force_tile(0)


def test_groupnorm_fused_into_the_halo_conv(fie):
    """conv3x3_gn: the producer writes x (and its GroupNorm sums) into a moated buffer, the fused conv normalises the resident halo."""
    from fie_amd import hip
    h, w, cin, cout = 16, 32, 128, 128
    x0, w0, b0 = rnd(1, h, w, 64, seed=1), rnd(cin, 64, 3, 3, seed=2, scale=(9 * 64) ** -0.5), rnd(cin, seed=3)
    wt, b1, res = rnd(cout, cin, 3, 3, seed=4, scale=(9 * cin) ** -0.5), rnd(cout, seed=5), rnd(1, h, w, cout, seed=6)
    gam, bet = 1 + 0.3 * rnd(cin, seed=7), 0.2 * rnd(cin, seed=8)
    wp0, wp = fie.pack_conv3x3(dev(w0)), fie.pack_conv3x3(dev(wt))
    x = fie.conv3x3(dev(x0), wp0, cin, bias=dev(b0)).float().cpu()
    y32 = F.silu(F.group_norm(x.permute(0, 3, 1, 2), 32, gam.float(), bet.float(), 1e-6))
    ref = (F.conv2d(y32, wt.float(), b1.float(), padding=1) + res.float().permute(0, 3, 1, 2)).permute(0, 2, 3, 1)

    def fn(i, o):
        xs = fie.conv3x3(i["x0"], wp0, cin, bias=i["b0"], gn_groups=32, out=i["xbuf"])
        coef = fie.groupnorm_coef(xs, i["gam"], i["bet"], 32, 1e-6)
        assert coef is not None
        fie.conv3x3_gn(xs, coef, True, wp, cout, bias=i["b1"], residual=i["res"], gn_groups=32, out=o)
        assert "conv_halo2" in hip.last_gemm_kernel(fie)

    out = isolated(fn, {"x0": flat(dev(x0)), "b0": dev(b0), "xbuf": flat(torch.zeros(1, h, w, cin, device=DEV, dtype=torch.float16)), "gam": dev(gam), "bet": dev(bet),
                        "b1": dev(b1), "res": flat(dev(res))}, dict(shape=(1, h, w, cout), ld=cout + 8))
    assert rel_err(out, ref) < 4e-3


@pytest.mark.parametrize("code,b,h,w,cin,c2,c3,cout", [(0, 2, 9, 7, 64, 64, 64, 72), (52, 2, 9, 7, 64, 64, 64, 72), (72, 1, 16, 32, 128, 128, 64, 128)])
def test_conv3x3_plus_with_strided_side_inputs(fie, code, b, h, w, cin, c2, c3, cout):
    x, x2, x3 = rnd(b, h, w, cin, seed=1), rnd(b * h * w, c2, seed=2), rnd(b * h * w, c3, seed=3)
    wc, wsc, bias = rnd(cout, cin, 3, 3, seed=4, scale=(9 * cin) ** -0.5), rnd(cout, c2 + c3, seed=5, scale=(c2 + c3) ** -0.5), rnd(cout, seed=6)
    wplus = torch.cat([fie.pack_conv3x3(dev(wc))[:, :9 * cin], fie.pack_linear(dev(wsc))[:, :c2 + c3]], 1).contiguous()
    ref = F.conv2d(x.float().permute(0, 3, 1, 2), wc.float(), bias.float(), padding=1).permute(0, 2, 3, 1) \
        + (torch.cat([x2, x3], 1).float() @ wsc.float().T).view(b, h, w, cout)
    try:
        fie.force_tile(code)
        out = isolated(lambda i, o: fie.conv3x3_plus(i["x"], wplus, cout, i["x2"], i["x3"], bias=i["bias"], out=o),
                       {"x": flat(dev(x)), "x2": wide(dev(x2), 64), "x3": wide(dev(x3), 192), "bias": dev(bias)}, dict(shape=(b, h, w, cout), ld=cout + 8))
        if code:
            ran(fie, code, "conv3x3")
    finally:
        fie.force_tile(0)
    assert rel_err(out, ref) < 4e-3


@pytest.mark.parametrize("code", [0, 42, 54])
def test_conv_up2x_parity_scatter(fie, code):
    b, h, w, cin, cout = 1, 8, 12, 64, 72
    x, wt, bias, ref = conv_case(b, h, w, cin, cout, 1, 0, True)
    wp4 = fie.pack_conv_up2x(wt)
    try:
        fie.force_tile(code)
        out = isolated(lambda i, o: fie.conv_up2x(i["x"], wp4, cout, bias=i["bias"], out=o), {"x": flat(dev(x)), "bias": dev(bias)},
                       dict(shape=(b, 2 * h, 2 * w, cout), ld=cout + 8))
    finally:
        fie.force_tile(0)
    assert rel_err(out, ref) < 4e-3


# ------------------------------------------------------------------------------------------------------------------------ fp8
@pytest.fixture
def w8(fie):
    fie.w8 = True
    yield fie
    fie.w8 = False
    fie.force_tile(0)


def test_gemm_w8_strided_a(w8):
    from fie_amd import hip
    a, w, bias, _ = gemm_case(M, N, 72)
    wp = w8.pack_linear(dev(w))
    out = isolated(lambda i, o: w8.gemm(i["a"], wp, N, bias=i["bias"], out=o), {"a": dev(a), "bias": dev(bias)}, dict(shape=(M, N), ld=N + 8))
    assert "fp8 weights" in hip.last_gemm_kernel(w8)
    assert rel_err(out, q8(a) @ f8(wp.q)[:N, :72].T * wp.scale[:N].cpu() + bias.float()) < 2e-3


@pytest.mark.parametrize("k", [272, 128])
def test_gemm_x8_strided_bytes(w8, k):
    """e4m3 activations with lda = K + 64 bytes: f16 output, e4m3 output with ldc = N + 16 bytes, GEGLU with an e4m3 output."""
    from fie_amd import hip
    a, w, bias, _ = gemm_case(M, N, k)
    wp = w8.pack_linear(dev(w))
    a8 = w8.quantize_f8(dev(a), 0.5)
    aq = f8(a8)
    assert torch.equal(aq, q8(a.float() * 0.5))
    lin = (aq @ f8(wp.q)[:N, :k].T) * 2.0 * wp.scale[:N].cpu() + bias.float()
    ins = {"a": a8.view(E4M3), "bias": dev(bias)}
    out = isolated(lambda i, o: w8.gemm(i["a"].view(torch.uint8), wp, N, bias=i["bias"], a_scale=2.0, out=o), ins, dict(shape=(M, N), ld=N + 8))
    assert ins["a"].dtype == E4M3 and "fp8 activations" in hip.last_gemm_kernel(w8)
    assert rel_err(out, lin) < 2e-3
    o8 = isolated(lambda i, o: w8.gemm(i["a"].view(torch.uint8), wp, N, bias=i["bias"], a_scale=2.0, out_f8=True, out_inv_scale=0.25, out=o), ins,
                  dict(shape=(M, N), ld=N + 16, dtype=E4M3))
    assert e4m3_close(o8, q8(lin * 0.25), 0.995)
    ag, wg, _, _ = gemm_case(M, 640, k)
    gbias, _ = geglu_case(M, 640, k)
    wpg = w8.pack_linear(dev(wg), geglu=True)
    ag8 = w8.quantize_f8(dev(ag))
    full = q8(ag) @ w8.pack_linear(dev(wg)).dequant().cpu()[:640, :k].T + gemm_case(M, 640, k)[2].float()
    o8 = isolated(lambda i, o: w8.gemm(i["a"].view(torch.uint8), wpg, 640, bias=i["bias"], act=hip.ACT_GEGLU, out_f8=True, out=o),
                  {"a": ag8.view(E4M3), "bias": dev(gbias)}, dict(shape=(M, 320), ld=336, dtype=E4M3))
    assert e4m3_close(o8, q8(full[:, :320] * F.gelu(full[:, 320:])), 0.99)


def test_conv_x8(w8):
    from fie_amd import hip
    b, h, w, cin, cout = 1, 9, 7, 128, 64
    x, wt, bias, _ = conv_case(b, h, w, cin, cout, 1, 0, False)
    wp = w8.pack_conv3x3(dev(wt))
    x8 = w8.quantize_f8(dev(x).view(-1, cin), 0.5).view(b, h, w, cin)
    wq = f8(wp.q)[:cout, :9 * cin].reshape(cout, 3, 3, cin).permute(0, 3, 1, 2)
    ref = (F.conv2d(f8(x8).permute(0, 3, 1, 2), wq, None, padding=1) * 2.0 * wp.scale[:cout].cpu()[None, :, None, None] + bias.float()[None, :, None, None]).permute(0, 2, 3, 1)
    out = isolated(lambda i, o: w8.conv3x3(i["x"].view(torch.uint8), wp, cout, bias=i["bias"], a_scale=2.0, out=o), {"x": flat(x8.view(E4M3)), "bias": dev(bias)},
                   dict(shape=(b, h, w, cout), ld=cout + 8))
    assert "fp8 activations" in hip.last_gemm_kernel(w8)
    assert rel_err(out, ref) < 2e-3


def test_quantize_f8_and_amax_on_strided_views(fie):
    x = rnd(37, 200, seed=1, scale=3.0)
    out = isolated(lambda i, o: fie.quantize_f8(i["x"], 0.5, out=o), {"x": dev(x)}, dict(shape=(37, 200), ld=216, dtype=E4M3))
    assert torch.equal(f8(out), q8(x.float() * 0.5))
    # the finite moat (1000.0) is larger than anything in the view: a row or a column too many shows in the maximum
    amax = isolated(lambda i, o: fie.amax_into(i["x"], o.zero_()), {"x": dev(x)}, dict(shape=(1,), dtype=torch.float32))
    assert amax.item() == x.float().abs().max().item() < 1000.0


# ------------------------------------------------------------------------------------------------------------------------ attention
ATTN = [(2, 3, 200, 333, 64, False), (2, 2, 100, 77, 64, False), (1, 2, 77, 77, 64, True), (1, 1, 1, 1, 64, False), (1, 1, 100, 100, 512, False),
        (2, 1, 40, 70, 512, False)]


def attn_isolated(fie, case, fused, **kw):
    b, hn, tq, tk, d, causal = case
    q, k, v, ref = attn_case(*case)
    c = hn * d
    e4 = kw.get("out_f8", False)
    spec = dict(shape=(b * tq, c), ld=c + 16 if e4 else c + 8, dtype=E4M3 if e4 else torch.float16)
    if fused:                                                    # one projection buffer, row stride 3C (+ the moat's gap)
        assert tq == tk
        return isolated(lambda i, o: fie.attention(i["qkv"][:, :c], i["qkv"][:, c:2 * c], i["qkv"][:, 2 * c:], hn, d, tq, tk, b, causal=causal, out=o, **kw),
                        {"qkv": dev(torch.cat([q, k, v], 1))}, spec), ref
    return isolated(lambda i, o: fie.attention(i["q"], i["k"], i["v"], hn, d, tq, tk, b, causal=causal, out=o, **kw),
                    {"q": wide(dev(q), 64), "k": wide(dev(k), 128), "v": wide(dev(v), 192)}, spec), ref


@pytest.mark.parametrize("variant", [0, 1, 2, 3, 4, 5, 6])
def test_attention(fie, variant):
    """The default dispatch and the six A/B forms: self-attention shapes through one fused-QKV buffer, the others with three independent strides."""
    from fie_amd import hip
    try:
        assert hip.lib().fie_debug_attn_variant(fie.h, variant) == 0
        for case in ATTN:
            if case[4] == 512 and variant > 1:                   # d = 512 has two kernels: the default and the first-generation one
                continue
            out, ref = attn_isolated(fie, case, fused=case[2] == case[3])
            assert rel_err(out, ref) < 4e-3, case
        out, ref = attn_isolated(fie, ATTN[2], fused=False)
        assert rel_err(out, ref) < 4e-3
    finally:
        hip.lib().fie_debug_attn_variant(fie.h, 0)


@pytest.mark.parametrize("case", ATTN[:4])
def test_attention_e4m3_output(fie, case):
    o16, _ = attn_isolated(fie, case, fused=False)
    o8, _ = attn_isolated(fie, case, fused=False, out_f8=True, out_inv_scale=8.0)
    assert e4m3_close(o8, q8(o16.float().cpu() * 8.0))


# ------------------------------------------------------------------------------------------------------------------------ norms
@pytest.mark.parametrize("rows,c", [(5, 64), (77, 768), (6, 1280), (3, 2048)])
def test_layernorm(fie, rows, c):
    x, g, bta = rnd(rows, c, seed=1) * 3 + 1, rnd(c, seed=2), rnd(c, seed=3)
    ref = F.layer_norm(x.float(), (c,), g.float(), bta.float(), 1e-5)
    ins = {"x": dev(x), "g": dev(g), "b": dev(bta)}                # ldx = C + 64
    out = isolated(lambda i, o: fie.layernorm(i["x"], i["g"], i["b"], out=o), ins, dict(shape=(rows, c), ld=c + 8))
    assert rel_err(out, ref) < 3e-3
    o8 = isolated(lambda i, o: fie.layernorm(i["x"], i["g"], i["b"], out=o, out_f8=True, out_inv_scale=2.0), ins, dict(shape=(rows, c), ld=c + 16, dtype=E4M3))
    assert e4m3_close(o8, q8(out.float().cpu() * 2.0))


@pytest.mark.parametrize("onepass", [1, 0])
@pytest.mark.parametrize("b,rows,c1,c2", [(2, 100, 64, 0), (1, 1000, 1280, 0), (1, 2051, 640, 0), (2, 256, 640, 320)])
def test_groupnorm(fie, b, rows, c1, c2, onepass):
    from fie_amd import hip
    x1, x2, gamma, beta, ref = groupnorm_case(b, rows, c1, c2)
    ins = {"x1": flat(dev(x1)), "x2": flat(dev(x2)) if c2 else None, "g": dev(gamma), "b": dev(beta)}
    try:
        hip.lib().fie_debug_gn_onepass(fie.h, onepass)
        out = isolated(lambda i, o: fie.groupnorm(i["x1"], i["g"], i["b"], 32, 1e-5, True, x2=i["x2"], out=o), ins, dict(shape=(b, rows, c1 + c2), flat=True))
        o8 = isolated(lambda i, o: fie.groupnorm(i["x1"], i["g"], i["b"], 32, 1e-5, True, x2=i["x2"], out=o, out_f8=True, out_inv_scale=2.0), ins,
                      dict(shape=(b, rows, c1 + c2), flat=True, dtype=E4M3))
    finally:
        hip.lib().fie_debug_gn_onepass(fie.h, 1)
    assert rel_err(out, ref) < 3e-3
    assert e4m3_close(o8, q8(out.float().cpu() * 2.0))


@pytest.mark.parametrize("cout,armed", [(640, False), (128, True)])
def test_groupnorm_after_the_producing_conv(fie, cout, armed):
    """conv3x3(..., gn_groups=32) then groupnorm on two 32x32 maps, 128 -> 640 channels (20 per group: below 64x64 maps nothing is armed and the
    single-pass kernel runs) and 128 -> 128 (4 per group: the conv's epilogue leaves the sums and groupnorm takes them)."""
    b, h, w, cin = 2, 32, 32, 128
    x, wt, bias, cref = conv_case(b, h, w, cin, cout, 1, 0, False)
    wp = fie.pack_conv3x3(dev(wt))
    gamma, beta = 1 + 0.1 * rnd(cout, seed=5), 0.1 * rnd(cout, seed=6)

    def fn(i, o):
        y = fie.conv3x3(i["x"], wp, cout, bias=i["bias"], gn_groups=32, out=o[0])
        assert (y._gn_tag is not None) == armed
        fie.groupnorm(y, i["g"], i["b"], 32, 1e-6, True, out=o[1])

    y, gn = isolated(fn, {"x": flat(dev(x)), "bias": dev(bias), "g": dev(gamma), "b": dev(beta)},
                     [dict(shape=(b, h, w, cout), flat=True), dict(shape=(b, h, w, cout), flat=True)])
    assert rel_err(y, cref) < 3e-3
    gref = F.silu(F.group_norm(y.float().cpu().permute(0, 3, 1, 2), 32, gamma.float(), beta.float(), 1e-6)).permute(0, 2, 3, 1)
    assert rel_err(gn, gref) < 4e-3


# ------------------------------------------------------------------------------------------------------------------------ pointwise
def test_copy_rows_add_and_sinusoid(fie):
    from fie_amd import hip
    lib, p = hip.lib(), hip._p
    fie.sync_stream()
    x = rnd(37, 72, seed=1)
    out = isolated(lambda i, o: hip._chk(lib.fie_copy_rows_f16(fie.h, p(i["x"]), i["x"].stride(0), p(o), o.stride(0), 37, 72)), {"x": dev(x)}, dict(shape=(37, 72), ld=80))
    assert torch.equal(out.cpu(), x)
    n = 8 * 37                                                     # fie_add_f16 takes n % 8 == 0: the ragged length next to 8 * 37 + 4
    a, b = rnd(n, seed=2), rnd(n, seed=3)
    with pytest.raises(hip.FieError):
        hip._chk(lib.fie_add_f16(fie.h, p(dev(a)), p(dev(b)), p(torch.empty(n + 8, device=DEV, dtype=torch.float16)), n + 4))
    out = isolated(lambda i, o: hip._chk(lib.fie_add_f16(fie.h, p(i["a"]), p(i["b"]), p(o), n)), {"a": dev(a), "b": dev(b)}, dict(shape=(n,)))
    assert torch.equal(out.cpu(), (a.float() + b.float()).half())
    # six values x 64 columns into columns 64 .. 448 of a 448-wide buffer
    vals = torch.tensor([[499.0, 1024.0, 0.0, 3.0, 768.0, 1.0], [259.0, 512.0, 17.0, 0.5, 1024.0, 999.0]])

    def sinus(i, o):
        base = torch.as_strided(o, (2, 448), (448, 1), o.storage_offset() - 64)
        fie.sinusoid(i["vals"], 64, base, col0=64)

    out = isolated(sinus, {"vals": flat(dev(vals))}, dict(shape=(2, 384), ld=448))
    f = torch.exp(-math.log(10000.0) * torch.arange(32, dtype=torch.float32) / 32)
    arg = vals[:, :, None] * f
    ref = torch.cat([torch.cos(arg), torch.sin(arg)], 2).reshape(2, 384)
    assert torch.allclose(out.float().cpu(), ref, atol=2e-3)


def test_clip_embed_and_pixels(fie):
    tok, pos = rnd(1000, 64, seed=1), rnd(77, 64, seed=2)
    ids = torch.randint(0, 1000, (2, 77), dtype=torch.int32, generator=torch.Generator().manual_seed(0))
    out = isolated(lambda i, o: fie.clip_embed(i["ids"], i["tok"], i["pos"], out=o), {"ids": dev(ids), "tok": flat(dev(tok)), "pos": flat(dev(pos))},
                   dict(shape=(154, 64), flat=True))
    assert rel_err(out, (tok.float()[ids.long()] + pos.float()[None]).reshape(-1, 64)) < 2e-3
    img = torch.from_numpy(np.random.default_rng(0).integers(0, 256, (64, 48, 3), dtype=np.uint8))
    x = isolated(lambda i, o: fie.pixels_in(i["img"], True, copies=2, out=o), {"img": dev(img)}, dict(shape=(2, 64, 48, 8), flat=True))
    assert torch.allclose(x[1, ..., :3].float().cpu(), 2.0 * (img.float() / 255.0) - 1.0, atol=1e-3) and x[..., 3:].abs().max() == 0
    back = isolated(lambda i, o: fie.pixels_out(i["x"], out=o), {"x": flat(x[:1].contiguous())}, dict(shape=(64, 48, 3), flat=True, dtype=torch.uint8))
    assert torch.equal(back.cpu(), img)


def test_latent_prep_and_lcm_steps_with_a_strided_eps(fie):
    from fie_amd import hip
    lib, p = hip.lib(), hip._p
    hw = 16 * 24
    g = torch.Generator().manual_seed(0)
    mom = torch.randn(hw, 8, generator=g).half()
    e1, e2 = torch.randn(4, hw, generator=g), torch.randn(4, hw, generator=g)
    lat, mi = isolated(lambda i, o: fie.latent_prep(i["mom"], i["e1"], i["e2"], hw, 0.13025, 0.5269, 0.8499, o[0], o[1]),
                       {"mom": flat(dev(mom)), "e1": flat(dev(e1)), "e2": flat(dev(e2))},
                       [dict(shape=(hw, 4), flat=True, dtype=torch.float32), dict(shape=(2, hw, 8), flat=True)])
    mean, logvar = mom.float()[:, :4], mom.float()[:, 4:].clamp(-30, 20)
    ref = 0.5269 * (mean + torch.exp(0.5 * logvar) * e1.T) * 0.13025 + 0.8499 * e2.T
    assert torch.allclose(lat.cpu(), ref, atol=1e-5)
    assert torch.allclose(mi[1, :, :4].float().cpu(), ref, atol=2e-3) and mi[..., 4:].abs().max() == 0
    # the step reads eps as [nb * hw, 4] with a row stride of its own (the UNet's output rows are wider than 4)
    eps = torch.randn(2 * hw, 4, generator=g).half()
    z, z0, n_init = torch.randn(4, hw, generator=g), torch.randn(hw, 4, generator=g), torch.randn(4, hw, generator=g)
    m_lat = (torch.rand(hw, generator=g) < 0.5).to(torch.uint8)
    sc = (0.5269, 0.8499, 0.002, 0.998, 0.8118, 0.5840)
    specs = [dict(shape=(hw, 4), flat=True, dtype=torch.float32), dict(shape=(2, hw, 8), flat=True), dict(shape=(hw, 8), flat=True)]
    ins = {"eps": dev(eps), "lat": flat(lat), "z": flat(dev(z)), "z0": flat(dev(z0)), "ni": flat(dev(n_init)), "m": flat(dev(m_lat))}

    def step(i, o, masked):
        fie.sync_stream()
        o[0].copy_(i["lat"])                                       # the latents are updated in place
        args = (fie.h, p(i["eps"]), i["eps"].stride(0), 2, 1.5, p(o[0]), p(i["z"]), hw, *sc, p(o[1]), 2, 1 / 0.13025, p(o[2]))
        hip._chk(lib.fie_lcm_step_masked(*args, p(i["m"]), p(i["z0"]), p(i["ni"])) if masked else lib.fie_lcm_step(*args))

    e = eps[:hw].float() + 1.5 * (eps[hw:].float() - eps[:hw].float())
    x = lat.cpu()
    den = sc[4] * (sc[3] * (x - sc[1] * e) / sc[0] + sc[2] * x) + sc[5] * z.T
    for masked in (False, True):
        lat2, mi2, dec = isolated(lambda i, o: step(i, o, masked), ins, specs)
        want = torch.where(m_lat.bool()[:, None], den, sc[4] * z0 + sc[5] * n_init.T) if masked else den
        assert torch.allclose(lat2.cpu(), want, atol=1e-4)
        assert torch.equal(mi2[0, :, :4].cpu(), lat2.cpu().half()) and torch.equal(mi2[0], mi2[1]) and mi2[..., 4:].abs().max() == 0
        assert torch.allclose(dec[:, :4].float().cpu(), want / 0.13025, rtol=2e-3, atol=2e-3)


def test_time_embed(fie):
    c0, e, b = 64, 256, 2
    t = torch.tensor([499.0, 259.0])
    w1, b1, w2, b2, add = rnd(e, c0, seed=1, scale=c0 ** -0.5), rnd(e, seed=2, scale=0.1), rnd(e, e, seed=3, scale=e ** -0.5), rnd(e, seed=4, scale=0.1), rnd(b, e, seed=5)
    ws = fie.time_embed_workspace(e)
    out = isolated(lambda i, o: fie.time_embed(i["t"], i["w1"], i["b1"], i["w2"], i["b2"], ws, add=i["add"], out=o),
                   {"t": flat(dev(t)), "w1": flat(dev(w1)), "b1": dev(b1), "w2": flat(dev(w2)), "b2": dev(b2), "add": dev(add)}, dict(shape=(b, e), ld=e + 8))
    fie.check_device_errors()
    f = torch.exp(-math.log(10000.0) * torch.arange(c0 // 2, dtype=torch.float32) / (c0 // 2))
    x = torch.cat([torch.cos(t[:, None] * f), torch.sin(t[:, None] * f)], 1)
    h = F.silu(x.half().float() @ w1.float().T + b1.float()).half().float()
    assert rel_err(out, F.silu(h @ w2.float().T + b2.float() + add.float())) < 3e-3


# ------------------------------------------------------------------------------------------------------------------------ u8 image kernels
U8 = dict(flat=True, dtype=torch.uint8)


@pytest.mark.parametrize("h,w,oh,ow", [(64, 48, 96, 80), (97, 131, 64, 64)])
def test_resize_lanczos(fie, h, w, oh, ow):
    from PIL import Image
    img = np.random.default_rng(h).integers(0, 256, (h, w, 3), dtype=np.uint8)
    out = isolated(lambda i, o: fie.resize_lanczos(i["img"], oh, ow, out=o), {"img": dev(torch.from_numpy(img))}, dict(shape=(oh, ow, 3), **U8))
    assert np.array_equal(out.cpu().numpy(), np.asarray(Image.fromarray(img).resize((ow, oh), Image.LANCZOS)))


def test_canny_device(fie):
    from oracle import canny
    rng = np.random.default_rng(1)
    img = np.zeros((97, 131, 3), np.uint8)
    img[:] = rng.integers(0, 255, 3)
    img[20:70, 30:100] = rng.integers(0, 255, 3)
    img[50:90, 10:60] = rng.integers(0, 255, 3)
    img = (img.astype(int) + rng.integers(-8, 8, img.shape)).clip(0, 255).astype(np.uint8)
    out = isolated(lambda i, o: fie.canny_device(i["img"], out=o), {"img": dev(torch.from_numpy(img))}, dict(shape=(97, 131, 3), **U8))
    assert np.array_equal(out.cpu().numpy(), canny.canny_rgb(img))


def test_mask_prep_fill_and_composite(fie):
    import masked_content_oracle as mco
    import masked_oracle
    from fie_amd import mask as hmask
    rng = np.random.default_rng(4)
    lm = (rng.integers(0, 2, (80, 96)) * 255).astype(np.uint8)
    lm[10:30, 20:50] = rng.integers(90, 170, (20, 30))
    binary = (lm >= 128).astype(np.float32)
    for r in (0, 1.0):
        m_px, m_lat = isolated(lambda i, o: fie.mask_prep(i["m"], r, out=(o[0], o[1])), {"m": flat(dev(torch.from_numpy(lm)))},
                               [dict(shape=(80, 96), flat=True, dtype=torch.float32), dict(shape=(120,), **U8)])
        assert np.array_equal(m_lat.cpu().numpy().reshape(10, 12), binary[::8, ::8].astype(np.uint8))
        assert np.abs(m_px.cpu().numpy() - (hmask.feather_numpy(binary, r) if r else binary)).max() <= (1e-5 if r else 0)
    h, w = 72, 88
    src, ctl, mask = mco.case_image(h, w, 1), mco.case_image(h, w, 2), mco.case_masks(h, w, 3)["threshold"]
    filled, cleared = isolated(lambda i, o: fie.mask_fill(i["s"], i["m"], i["c"], out=o[0], cleared=o[1]),
                               {"s": dev(torch.from_numpy(src)), "m": flat(dev(torch.from_numpy(np.ascontiguousarray(mask)))), "c": dev(torch.from_numpy(ctl))},
                               [dict(shape=(h, w, 3), **U8), dict(shape=(h, w, 3), **U8)])
    assert np.array_equal(filled.cpu().numpy(), mco.fill(src, mask)) and np.array_equal(cleared.cpu().numpy(), mco.clear_edges(ctl, mask))
    g = torch.Generator().manual_seed(5)
    h, w = 40, 56
    dec = (torch.randn((1, h, w, 8), generator=g) * 1.2).half()
    s8 = torch.randint(0, 256, (h, w, 3), generator=g, dtype=torch.uint8)
    m = torch.rand((h, w), generator=g)
    m[:, :16], m[:, 16:32] = 0, 1
    got = isolated(lambda i, o: fie.pixels_out_composite(i["d"], i["s"], i["m"], out=o), {"d": flat(dev(dec)), "s": dev(s8), "m": flat(dev(m))},
                   dict(shape=(h, w, 3), **U8)).cpu().numpy()
    want = masked_oracle.composite(dec[..., :3].float().permute(0, 3, 1, 2), s8.numpy(), m.numpy())
    hard = (m.numpy() == 0) | (m.numpy() == 1)
    assert np.array_equal(got[:, :16], s8.numpy()[:, :16]) and np.array_equal(got[hard], want[hard]) and np.abs(got.astype(int) - want.astype(int)).max() <= 1


# ------------------------------------------------------------------------------------------------------------------------ fp32 entries (csrc/f32.hip)
F32 = dict(dtype=torch.float32)


@pytest.fixture(scope="module")
def f32ctx():
    import fie_amd  # noqa: F401
    from fie_amd import hip
    return hip.context(0, torch.float32)


def rnd32(*shape, seed=0, scale=1.0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * scale


@pytest.mark.parametrize("m,n,k1,k2", [(67, 40, 17, 23), (130, 65, 16, 1), (3, 200, 72, 8)])
def test_gemm_f32_strided_operands_and_a_column_range(f32ctx, m, n, k1, k2):
    """fie_gemm_f32 with A1, A2, the weights, the row bias and the residual each inside its own moat (independent row strides) and the output a column
    range of a three times wider tensor; the bar of tests/test_fp32_gpu.py (2e-5)."""
    from fie_amd import hip
    a1, a2, w = rnd32(m, k1, seed=1), rnd32(m, k2, seed=2), rnd32(n, k1 + k2, seed=3, scale=(k1 + k2) ** -0.5)
    bias, res, rpb = rnd32(n, seed=4), rnd32(m, n, seed=5), 7
    rb = rnd32((m + rpb - 1) // rpb, n, seed=6)
    ref = F.relu(torch.cat([a1, a2], 1) @ w.T + bias + rb.repeat_interleave(rpb, 0)[:m]) * 0.5 + res
    out = isolated(lambda i, o: f32ctx.gemm_f32(i["a1"], i["w"], n, out=o, a2=i["a2"], bias=i["bias"], rowbias=i["rb"], rows_per_batch=rpb, residual=i["res"],
                                                scale=0.5, act=hip.ACT_RELU),
                   {"a1": wide(dev(a1), 64), "a2": wide(dev(a2), 128), "w": wide(dev(w), 32), "bias": dev(bias), "rb": wide(dev(rb), 16), "res": wide(dev(res), 96)},
                   dict(shape=(m, n), ld=3 * n + 4, **F32))
    assert rel_err(out, ref) < 2e-5


@pytest.mark.parametrize("case,cout", [((2, 9, 7, 8, 24, 1, 0, False), 24), ((2, 9, 7, 24, 65, 2, 1, False), 65), ((1, 4, 5, 8, 3, 1, 0, True), 3)])
def test_conv3x3_f32_channel_range(f32ctx, case, cout):
    """fie_conv3x3_nhwc_f32 writing channels of a wider NHWC tensor (the Fire modules' expand branch): two images, so that a padding tap that addresses a
    neighbour lands in the other image or in the moat."""
    b, h, w, cin, _, stride, pad_mode, ups = case
    x, wt, bias = rnd32(b, h, w, cin, seed=1), rnd32(cout, cin, 3, 3, seed=2, scale=(9 * cin) ** -0.5), rnd32(cout, seed=3)
    xi = x.permute(0, 3, 1, 2)
    if ups:
        xi = F.interpolate(xi, scale_factor=2.0, mode="nearest")
    if pad_mode == 1:
        xi = F.pad(xi, (0, 1, 0, 1))
    ref = F.conv2d(xi, wt, bias, stride=stride, padding=1 if pad_mode == 0 else 0).permute(0, 2, 3, 1).contiguous()
    wp = wt.permute(0, 2, 3, 1).reshape(cout, 9 * cin).contiguous()
    out = isolated(lambda i, o: f32ctx.conv3x3_f32(i["x"], i["w"], cout, o, stride=stride, pad_mode=pad_mode, upsample=ups, bias=i["bias"]),
                   {"x": flat(dev(x)), "w": wide(dev(wp), 32), "bias": dev(bias)}, dict(shape=tuple(ref.shape), ld=cout + 40, **F32))
    assert rel_err(out, ref) < 2e-5


@pytest.mark.parametrize("rows,cols,causal,tq", [(5, 65, False, 1), (130, 200, True, 77), (7, 1025, True, 7)])
def test_softmax_rows_f32_in_place(f32ctx, rows, cols, causal, tq):
    from fie_amd import hip
    s = rnd32(rows, cols, seed=1, scale=3.0)
    x = s * 0.125
    if causal:
        x = x.masked_fill(torch.arange(cols)[None, :] > (torch.arange(rows) % tq)[:, None], float("-inf"))
    ref = torch.softmax(x, -1)

    def fn(i, o):
        o.copy_(i["s"])
        f32ctx.sync_stream()
        hip._chk(hip.lib().fie_softmax_rows_f32(f32ctx.h, hip._p(o), rows, cols, o.stride(0), 0.125, int(causal), tq))

    out = isolated(fn, {"s": dev(s)}, dict(shape=(rows, cols), ld=cols + 12, **F32))
    assert rel_err(out, ref) < 2e-5


@pytest.mark.parametrize("case", [(2, 3, 77, 77, 64, True), (2, 2, 33, 33, 40, False), (1, 1, 20, 20, 512, False)])
def test_attention_f32_fused_qkv(f32ctx, case):
    """The fp32 composition (Q K^T, softmax, P V) on one fused-QKV buffer inside a moat: three column slices with the row stride 3 C + the gap."""
    b, hn, tq, tk, d, causal = case
    c = hn * d
    q, k, v = rnd32(b * tq, c, seed=1), rnd32(b * tk, c, seed=2), rnd32(b * tk, c, seed=3)
    sp = lambda x, t: x.view(b, t, hn, d).transpose(1, 2)
    ref = F.scaled_dot_product_attention(sp(q, tq), sp(k, tk), sp(v, tk), is_causal=causal).transpose(1, 2).reshape(b * tq, c)
    out = isolated(lambda i, o: f32ctx.attention(i["qkv"][:, :c], i["qkv"][:, c:2 * c], i["qkv"][:, 2 * c:], hn, d, tq, tk, b, causal=causal, out=o),
                   {"qkv": dev(torch.cat([q, k, v], 1))}, dict(shape=(b * tq, c), ld=c + 12, **F32))
    assert rel_err(out, ref) < 2e-5
