"""Checkers and float64 references of tests/test_launch_table_gpu.py (device-agnostic torch; the CPU self-check in
tests/test_launch_check_cpu.py runs them on crafted outputs).

Three comparisons of a kernel's f16 output `out` with a float64 reference `ref` of the same operation:

  exact_mismatches      integer data: every fp32 partial sum is exact, so every tile, split and summation order must give the fp64 result
                        rounded ONCE to f16 (RNE).  No tolerance (+0 and -0 compare equal).
  ulp_mismatches        the same with an ulp bound (fp8 weight scales, activations evaluated in fp32).
  precision_ratio       real-valued data: the rounding error per element, never normalised by a max: the worst of
                        (|out - ref| - 0.5 ulp16) / (sqrt(K) 2^-24 (|A||W|)), which an fp32-accumulating kernel keeps O(1) and an fp16-
                        accumulating one pushes to ~2^13.
"""
import math

import torch

F16_MIN_SUB = 2.0 ** -24


def ulp16(x):
    """Spacing of f16 numbers at |x| (float64 tensor): 2^(e - 10) for normal values, 2^-24 in the subnormal range."""
    a = x.abs().clamp_min(2.0 ** -14)
    return torch.exp2(torch.floor(torch.log2(a)) - 10)


def ulp8(x):
    """Spacing of e4m3 numbers at |x| (3 mantissa bits, smallest normal 2^-6, subnormal step 2^-9)."""
    a = x.abs().clamp_min(2.0 ** -6)
    return torch.exp2(torch.floor(torch.log2(a)) - 3)


def _where(bad, limit=4):
    idx = bad.nonzero()[:limit]
    return [tuple(int(v) for v in i) for i in idx]


def exact_mismatches(out, ref):
    """(count, first positions) of elements where f16 `out` differs from f16(ref) -- the single RNE rounding of the float64 reference."""
    r16 = ref.to(torch.float16)
    bad = (out != r16) & ~(torch.isnan(out) & torch.isnan(r16))
    return int(bad.sum()), _where(bad)


def ulp_mismatches(out, ref, n_ulp, floor=0.0):
    """(count, first positions) of elements with |out - ref| > n_ulp * ulp16(ref) + floor (ref float64, out f16)."""
    o = out.double()
    ulp = torch.maximum(ulp16(ref), ulp16(o))
    bad = ~((o - ref).abs() <= n_ulp * ulp + floor)
    return int(bad.sum()), _where(bad)


def f8_mismatches(out_bytes, ref, n_ulp=1, floor=0.0):
    """e4m3 output bytes against float64 ref (already multiplied by the output's inverse scale, saturated to +-448)."""
    o = out_bytes.view(torch.float8_e4m3fn).double()
    r = ref.clamp(-448.0, 448.0)
    bad = ~((o - r).abs() <= n_ulp * torch.maximum(ulp8(r), ulp8(o)) + floor)
    return int(bad.sum()), _where(bad)


def precision_ratio(out, ref, absref, K):
    """Worst (|out - ref| - 0.5 ulp16) / (sqrt(K) 2^-24 absref) over the elements (0 when every element is within its final rounding)."""
    o = out.double()
    excess = ((o - ref).abs() - 0.5 * torch.maximum(ulp16(ref), ulp16(o))).clamp_min(0.0)
    denom = math.sqrt(K) * 2.0 ** -24 * absref
    ratio = torch.where(excess > 0, excess / denom.clamp_min(1e-300), torch.zeros_like(excess))
    ratio = torch.where(torch.isfinite(o), ratio, torch.full_like(ratio, float("inf")))
    return float(ratio.max())


def precision_mismatches(out, ref, absref, K, c):
    """(count, first positions) of elements outside |out - ref| <= 0.5 ulp16(ref) + c sqrt(K) 2^-24 absref."""
    o = out.double()
    bound = 0.5 * torch.maximum(ulp16(ref), ulp16(o)) + c * math.sqrt(K) * 2.0 ** -24 * absref
    bad = ~((o - ref).abs() <= bound)
    return int(bad.sum()), _where(bad)


# ---------------------------------------------------------------------------------------------------- float64 references
def gelu64(x):
    return 0.5 * x * (1.0 + torch.erf(x / math.sqrt(2.0)))


def act64(h, act):
    """The library's activations (include/fie.h: FIE_ACT_*) in float64; GEGLU on (value, gate) column pairs of the packed order."""
    if act == 0:
        return h
    if act == 1:
        return h * torch.sigmoid(h)
    if act == 2:
        return gelu64(h)
    if act == 3:
        return h * torch.sigmoid(1.702 * h)
    if act == 4:
        return h[:, 0::2] * gelu64(h[:, 1::2])
    raise ValueError(act)


def act_abs64(h, habs, act):
    """A bound on how far act moves an absolute error budget `habs` of its input h (|act'| <= 1.13 for SiLU / GELU / quick-GELU)."""
    if act == 0:
        return habs
    if act in (1, 2, 3):
        return 1.13 * habs
    if act == 4:
        v, g, va, ga = h[:, 0::2], h[:, 1::2], habs[:, 0::2], habs[:, 1::2]
        return va * gelu64(g).abs() + v.abs() * 1.13 * ga
    raise ValueError(act)


def conv_taps64(x, taps, geo):
    """sum over taps of shifted [rows, Cin] x [Cin, N] float64 GEMMs (never an im2col matrix).  x: [B, H, W, Cin] float64 (already up-sampled
    for `ups`); taps: list of (dy, dx, W_t [N, Cin]); output pixel (y, x) of tap (dy, dx) reads input (y * s + dy, x * s + dx) of x padded by
    `geo['pt']` rows / columns at the top / left and zeros below / right.  Returns [B * OH * OW, N]."""
    B, H, W, C = x.shape
    s, pt, OH, OW = geo["stride"], geo["pt"], geo["OH"], geo["OW"]
    xp = x.new_zeros((B, H + 2, W + 2, C))
    xp[:, pt:pt + H, pt:pt + W] = x
    out = None
    for dy, dx, wt in taps:
        sl = xp[:, dy: dy + s * (OH - 1) + 1: s, dx: dx + s * (OW - 1) + 1: s].reshape(-1, C)
        part = sl @ wt.t()
        out = part if out is None else out.add_(part)
    return out
