"""Float64 references, input builders, checkers and defect models of tests/test_attn_norm_gpu.py (device-agnostic torch; the CPU self-check
in tests/test_attn_norm_check_cpu.py runs them on the defect models below).

Attention (csrc/attention.hip), tensors as [B, H, T, D]:

  selector / ramp / uniform   inputs for which softmax(QK^T)V has ONE valid f16 answer: every loser's P flushes to zero in f16 (score gap of at
                              least GAP_MIN in the log2 domain), or every P is exactly 1 and the V sums are integers.  A wrong key count,
                              mask, head / batch offset or V-transpose map changes whole rows; `which_key` names the key that was picked.
  attn_ratio                  real data: worst (|out - ref| - 0.5 ulp16) / (eps_q dev), dev = sum_j w_j |v_jd - ref_d| the spread of V under
                              the row's softmax and eps_q = 2^-10 + ln2 2^-11 max_j sum_d |q_d k_jd| scale log2e the relative error of one
                              weight (P rounded to f16 for numerator and denominator alike; Q pre-scaled into f16).

GroupNorm / LayerNorm (csrc/norm.hip), tensors as [B, rows, C] / [rows, C]:

  norm_ratio                  worst (|out - ref| - 0.5 ulp) / (2^-24 (|x| + |mu| + sigma) |gamma| / sigma A): the fp32 cancellation of
                              x * sc + sh, A = 1.13 behind SiLU (launch_check.act_abs64).
"""
import math

import torch

import launch_check as lc

LOG2E = 1.4426950408889634
GAP_MIN = 40.0            # log2-domain score gap at which a loser's P (<= 2^-40) is zero in f16 whatever reference the lazy rescale holds (THR = 6)
KT = 64                   # key tile of the d = 64 kernels (96 in the one-tile cross-attention form; 32 at d = 512)


def to_f16_rne(x):
    """float64 -> f16 with ONE round-to-nearest-even (a conversion that passes through fp32 rounds twice and misses ties by an fp32 ulp)."""
    c = x.to(torch.float16)
    c64 = c.double()
    u = lc.ulp16(c64)
    best, err = c64, (c64 - x).abs()
    for cand in (c64 - u, c64 + u, c64 - u / 2):          # the neighbours (below a power of two the spacing halves)
        cand16 = cand.to(torch.float16).double()
        e = (cand16 - x).abs()
        better = (e < err) & torch.isfinite(cand16)
        best, err = torch.where(better, cand16, best), torch.where(better, e, err)
    return best.to(torch.float16)


def ulp32(x):
    """Spacing of fp32 numbers at |x| (float64 tensor)."""
    a = x.abs().clamp_min(2.0 ** -126)
    return torch.exp2(torch.floor(torch.log2(a)) - 23)


# ------------------------------------------------------------------------------------------------------------------ attention: reference
def _mask(tq, tk, device):
    return torch.arange(tk, device=device)[None, :] > torch.arange(tq, device=device)[:, None]          # key > query: not visible


def attn_weights64(q, k, scale, causal):
    s = (q.double() @ k.double().transpose(-1, -2)) * scale
    if causal:
        s = s.masked_fill(_mask(q.shape[-2], k.shape[-2], q.device), float("-inf"))
    return torch.softmax(s, -1)


def attn_ref64(q, k, v, scale, causal=False):
    """softmax(scale q k^T [+ causal mask]) v in float64 on the stored (f16) inputs; [B, H, Tq, D]."""
    return attn_weights64(q, k, scale, causal) @ v.double()


def attn_budget64(q, k, v, scale, causal=False):
    """(ref, dev, eps_q): the float64 reference, dev[b, h, q, d] = sum_j w_j |v_jd - ref_d| and eps_q[b, h, q, 1]."""
    w = attn_weights64(q, k, scale, causal)
    v64 = v.double()
    ref = w @ v64
    B, H, Tq, D = ref.shape
    Tk = k.shape[-2]
    dev = torch.empty_like(ref)
    step = max(1, (1 << 22) // (Tk * D))                    # query rows per chunk: the [rows, Tk, D] difference tensor stays small
    for i in range(0, Tq, step):
        diff = (v64[:, :, None, :, :] - ref[:, :, i:i + step, None, :]).abs()                         # [B, H, rows, Tk, D]
        dev[:, :, i:i + step] = (w[:, :, i:i + step, :, None] * diff).sum(3)
    a = (q.double().abs() @ k.double().abs().transpose(-1, -2)) * (scale * LOG2E)
    if causal:
        a = a.masked_fill(_mask(Tq, Tk, q.device), 0.0)
    eps = 2.0 ** -10 + math.log(2.0) * 2.0 ** -11 * a.amax(-1, keepdim=True)
    return ref, dev, eps


def attn_ratio(out, ref, dev, eps):
    """Worst (|out - ref| - 0.5 ulp16) / (eps_q dev) over the elements; 0 when every element is within its final rounding."""
    o = out.double()
    excess = ((o - ref).abs() - 0.5 * torch.maximum(lc.ulp16(ref), lc.ulp16(o))).clamp_min(0.0)
    ratio = torch.where(excess > 0, excess / (eps * dev).clamp_min(1e-300), torch.zeros_like(excess))
    ratio = torch.where(torch.isfinite(o), ratio, torch.full_like(ratio, float("inf")))
    return float(ratio.max())


def attn_mismatches(out, ref, dev, eps, c):
    """(count, first positions) of elements outside |out - ref| <= 0.5 ulp16 + c eps_q dev."""
    o = out.double()
    bound = 0.5 * torch.maximum(lc.ulp16(ref), lc.ulp16(o)) + c * eps * dev
    bad = ~((o - ref).abs() <= bound)
    return int(bad.sum()), lc._where(bad)


def old_metric(out, ref):
    """What tests/test_ops_gpu.py asserts: one number per tensor, max |out - ref| / max |ref|."""
    return float((out.double() - ref.double()).abs().max() / ref.double().abs().max().clamp_min(1e-6))


# ------------------------------------------------------------------------------------------------------------------ attention: builders
def distinct_v(B, H, Tk, D, device):
    """f16 values with |v| in [0.25, 4): the 8192 of them (4 binades x 1024 mantissas x 2 signs) indexed so that within a (b, h) no two
    keys share a value at any d, no two d share one within a key, and heads / batches are shifted against each other."""
    b = torch.arange(B, device=device)[:, None, None, None]
    h = torch.arange(H, device=device)[None, :, None, None]
    j = torch.arange(Tk, device=device)[None, None, :, None]
    d = torch.arange(D, device=device)[None, None, None, :]
    assert Tk <= 8192 and D <= 8192
    idx = (j * 4099 + d * 13 + (b * H + h) * 523) % 8192                     # 4099 and 13 are odd: injective in j and in d (mod 2^13)
    mag = ((idx >> 1) + 0x3400).to(torch.int16)                              # f16 bit patterns 0x3400 (0.25) .. 0x43ff (just below 4)
    bits = torch.where((idx & 1).bool(), mag | torch.tensor(-32768, dtype=torch.int16, device=device), mag)
    v = bits.view(torch.float16)
    assert bool((v.abs() >= 0.25).all()) and bool((v.abs() < 4.0).all())
    return v


def log2_scores(q, k, scale):
    return (q.double() @ k.double().transpose(-1, -2)) * (scale * LOG2E)


def special_keys(Tk, kt=KT):
    """Keys a wrong tile tail, seam or last-tile start would miss: 0, Tk - 1, the first key of the last tile, the seams 63 / 64 and 95 / 96."""
    cand = [0, Tk - 1, (Tk - 1) // kt * kt, 63, 64, 95, 96, 31, 32]
    out = []
    for c in cand:
        if 0 <= c < Tk and c not in out:
            out.append(c)
    return out


def selector_case(B, H, Tq, Tk, D, g, gen, scale=None):
    """Keys are random +-1 vectors, q_i = g k_pi(i): the picked key wins by at least GAP_MIN (asserted), so out[i] = V[pi(i)] exactly."""
    dev = gen.device
    scale = D ** -0.5 if scale is None else scale
    k = (torch.randint(0, 2, (B, H, Tk, D), generator=gen, device=dev) * 2 - 1).to(torch.float16)
    sp = special_keys(Tk, 32 if D == 512 else KT)
    pi = torch.empty((B, H, Tq), dtype=torch.long, device=dev)
    for b in range(B):
        for h in range(H):
            r = (b * H + h) % len(sp)
            head = torch.tensor(sp[r:] + sp[:r], device=dev)
            n = max(0, Tq - len(head))
            perm = torch.cat([torch.randperm(Tk, generator=gen, device=dev) for _ in range(n // Tk + 1)])[:n]
            pi[b, h] = torch.cat([head, perm])[:Tq]
    q = (g * torch.gather(k.double(), 2, pi[..., None].expand(B, H, Tq, D))).to(torch.float16)
    v = distinct_v(B, H, Tk, D, dev)
    s = log2_scores(q, k, scale)
    win = torch.gather(s, 3, pi[..., None])
    rest = s.scatter(3, pi[..., None], float("-inf")).amax(-1, keepdim=True) if Tk > 1 else torch.full_like(win, float("-inf"))
    gap = float((win - rest).min())
    assert gap >= GAP_MIN, f"selector case: winner's log2-domain score leads by {gap:.1f} < {GAP_MIN}"
    expect = torch.gather(v, 2, pi[..., None].expand(B, H, Tq, D))
    return {"q": q, "k": k, "v": v, "scale": scale, "causal": False, "pi": pi, "expect": expect, "gap": gap}


def ramp_case(B, H, Tq, Tk, D, causal, device, g=8.0, delta=0.5, scale=None):
    """q = g ones, k_j = j delta ones: the visible key with the largest index wins by at least GAP_MIN per step (asserted).  Not causal: every
    row is V[Tk - 1]; causal: row i is V[min(i, Tk - 1)] -- a leaked key i + 1 or a masked diagonal returns a neighbour's row."""
    scale = D ** -0.5 if scale is None else scale
    q = torch.full((B, H, Tq, D), g, dtype=torch.float16, device=device)
    kj = torch.arange(Tk, device=device, dtype=torch.float64) * delta
    k = kj.to(torch.float16)[None, None, :, None].expand(B, H, Tk, D).contiguous()
    assert bool((k[0, 0, :, 0].double() == kj).all()), "ramp case: j * delta is not exact in f16"
    step = D * g * delta * scale * LOG2E
    assert step >= GAP_MIN, f"ramp case: one key step is {step:.1f} < {GAP_MIN} in the log2 domain"
    v = distinct_v(B, H, Tk, D, device)
    i = torch.arange(Tq, device=device)
    pick = torch.clamp(i, max=Tk - 1) if causal else torch.full_like(i, Tk - 1)
    pi = pick[None, None, :].expand(B, H, Tq).contiguous()
    expect = torch.gather(v, 2, pi[..., None].expand(B, H, Tq, D))
    return {"q": q, "k": k, "v": v, "scale": scale, "causal": causal, "pi": pi, "expect": expect, "gap": step}


def uniform_case(B, H, Tq, Tk, D, c, causal, device, scale=None):
    """Constant Q rows, K rows = c ones (c in {0, -2^m, +2^m}): every visible key scores the same, every P is 1 in every tile, V holds small
    integers: out = sum(V) / count.  With c < 0 a zero-filled key that is not masked leads by at least GAP_MIN (asserted) and takes the row."""
    scale = D ** -0.5 if scale is None else scale
    qc = torch.tensor([1.0, 2.0, 0.5], device=device)[torch.arange(Tq, device=device) % 3]
    q = qc.to(torch.float16)[None, None, :, None].expand(B, H, Tq, D).contiguous()
    k = torch.full((B, H, Tk, D), c, dtype=torch.float16, device=device)
    assert c == 0 or math.log2(abs(c)) == int(math.log2(abs(c))), "uniform case: c must be 0 or a power of two"
    if c < 0:
        lead = float(-(D * qc.min().double() * c * scale * LOG2E))
        assert lead >= GAP_MIN, f"uniform case: an unmasked zero key leads by only {lead:.1f} < {GAP_MIN}"
    b = torch.arange(B, device=device)[:, None, None, None]
    h = torch.arange(H, device=device)[None, :, None, None]
    j = torch.arange(Tk, device=device)[None, None, :, None]
    d = torch.arange(D, device=device)[None, None, None, :]
    v = (((j * 7 + d * 3 + (b * H + h) * 5 + (j * d) % 5) % 8) - 3).to(torch.float16)          # integers -3 .. 4, mean != 0
    csum = v.double().cumsum(2)
    assert float(v.double().abs().sum(2).max()) < 2.0 ** 24, "uniform case: integer sums must stay exact in fp32"
    i = torch.arange(Tq, device=device)
    last = torch.clamp(i, max=Tk - 1) if causal else torch.full_like(i, Tk - 1)
    count = (last + 1).double()
    ref = csum[:, :, last, :] / count[None, None, :, None]
    return {"q": q, "k": k, "v": v, "scale": scale, "causal": causal, "ref": ref, "count": (last + 1)}


def uniform_mismatches(out, ref, count):
    """Rows whose key count is a power of two: bit-exact (1 / count, the product and the store are exact or one rounding); the others within
    1 ulp16 (fp32 1 / l, the product and the store each round)."""
    pow2 = ((count & (count - 1)) == 0)[None, None, :, None]
    o = out.double()
    exact_bad = (out != to_f16_rne(ref))
    ulp_bad = ~((o - ref).abs() <= torch.maximum(lc.ulp16(ref), lc.ulp16(o)))
    bad = torch.where(pow2, exact_bad, ulp_bad)
    return int(bad.sum()), lc._where(bad)


def real_case(B, H, Tq, Tk, D, peaky, causal, gen, scale=None):
    """Q, K ~ N(0, 1) (x3 when peaky), V ~ N(0.25, 1), and one late key spiked onto a query (the running max jumps mid-sequence)."""
    dev = gen.device
    scale = D ** -0.5 if scale is None else scale
    m = 3.0 if peaky else 1.0
    q = (torch.randn((B, H, Tq, D), generator=gen, device=dev) * m).to(torch.float16)
    k = (torch.randn((B, H, Tk, D), generator=gen, device=dev) * m).to(torch.float16)
    v = (torch.randn((B, H, Tk, D), generator=gen, device=dev) + 0.25).to(torch.float16)
    if Tk > 2:
        k[:, :, (Tk * 3) // 5] = (q[:, :, min(5, Tq - 1)].float() * (4.0 / m)).to(torch.float16)
    return {"q": q, "k": k, "v": v, "scale": scale, "causal": causal}


def which_key(out_row, v_bh):
    """Index of the key whose V row equals out_row bit for bit, or -1."""
    hit = (v_bh == out_row[None, :]).all(-1).nonzero()
    return int(hit[0]) if hit.numel() else -1


def describe_pick(out, case, pos):
    """'(b, h, q): picked key j of (b', h'), wanted key pi' for the first wrong element at `pos`."""
    b, h, i = pos[0], pos[1], pos[2]
    want = int(case["pi"][b, h, i])
    v = case["v"]
    got = which_key(out[b, h, i], v[b, h])
    if got >= 0:
        return f"(b={b}, h={h}, q={i}): wanted key {want}, got key {got} of the same head"
    for bb in range(v.shape[0]):
        for hh in range(v.shape[1]):
            got = which_key(out[b, h, i], v[bb, hh])
            if got >= 0:
                return f"(b={b}, h={h}, q={i}): wanted key {want}, got key {got} of batch {bb} head {hh}"
    return f"(b={b}, h={h}, q={i}): wanted key {want}, got a row that is no key's V (a mixture, or a scrambled d order)"


# ------------------------------------------------------------------------------------------------------------------ attention: defect models
ATTN_DEFECTS = ["phantom_key", "drop_last_key", "causal_leak", "causal_diagonal", "v_head_shift", "k_batch0", "fragment_swap", "pv_f16"]


def attn_model(q, k, v, scale, causal=False, defect=None):
    """A float64 model of the op with one defect built in; returns what the kernel would store (f16)."""
    q64, k64, v64 = q.double(), k.double(), v.double()
    B, H, Tq, D = q.shape
    Tk = k.shape[2]
    if defect == "phantom_key":                  # the zero-filled tail of the last key tile is not masked: one more key with score 0, V = 0
        k64 = torch.cat([k64, torch.zeros_like(k64[:, :, :1])], 2)
        v64 = torch.cat([v64, torch.zeros_like(v64[:, :, :1])], 2)
    if defect == "drop_last_key":
        k64, v64 = k64[:, :, :-1], v64[:, :, :-1]
    if defect == "v_head_shift":                 # head h + 1 reads the V of head h
        v64 = torch.roll(v64, 1, 1)
    if defect == "k_batch0":                     # batch 1 reads batch 0's K
        k64 = k64[:1].expand_as(k64)
    s = (q64 @ k64.transpose(-1, -2)) * scale
    tk = k64.shape[2]
    if causal:
        kk, qq = torch.arange(tk, device=q.device)[None, :], torch.arange(Tq, device=q.device)[:, None]
        hidden = kk > qq + 1 if defect == "causal_leak" else (kk >= qq) & (kk > 0) if defect == "causal_diagonal" else kk > qq
        s = s.masked_fill(hidden, float("-inf"))
    w = torch.softmax(s, -1)
    if defect == "pv_f16":                       # P V summed key by key in an f16 accumulator
        p16 = (w / w.amax(-1, keepdim=True)).to(torch.float16)
        acc = torch.zeros((B, H, Tq, D), dtype=torch.float16, device=q.device)
        for j in range(tk):
            acc = (acc.float() + p16[..., j, None].float() * v[:, :, j, None, :].float()).to(torch.float16)
        out = acc.double() / p16.double().sum(-1, keepdim=True)
    else:
        out = w @ v64
    out = to_f16_rne(out)
    if defect == "fragment_swap" and Tq > 1:     # one 16-query x 4-d output fragment holds the next query's values
        q0 = max(0, min(16, Tq - 17))
        n = min(16, Tq - 1 - q0)
        out[-1, -1, q0:q0 + n, 4:8] = out[-1, -1, q0 + 1:q0 + 1 + n, 4:8].clone()
    return out


# ------------------------------------------------------------------------------------------------------------------ norms: references
def act_factor(silu):
    return 1.13 if silu else 1.0


def gn_ref64(x, groups, gamma, beta, eps, silu):
    """(ref, slack) of GroupNorm(+SiLU) over [B, rows, C] in float64 on the stored inputs; slack = 2^-24 (|x| + |mu| + sigma) |gamma| / sigma A."""
    x64 = x.double()
    B, rows, C = x64.shape
    xg = x64.view(B, rows, groups, C // groups)
    mu = xg.mean((1, 3), keepdim=True)
    var = ((xg - mu) ** 2).mean((1, 3), keepdim=True)
    sigma = torch.sqrt(var + eps)
    z = ((xg - mu) / sigma).view(B, rows, C)
    y = z * gamma.double() + beta.double()
    ref = lc.act64(y, 1 if silu else 0)
    slack = (2.0 ** -24 * (xg.abs() + mu.abs() + sigma) / sigma).view(B, rows, C) * gamma.double().abs() * act_factor(silu)
    return ref, slack


def ln_ref64(x, gamma, beta, eps):
    """(ref, slack) of LayerNorm over the last dim of [rows, C]."""
    x64 = x.double()
    mu = x64.mean(-1, keepdim=True)
    sigma = torch.sqrt(((x64 - mu) ** 2).mean(-1, keepdim=True) + eps)
    ref = (x64 - mu) / sigma * gamma.double() + beta.double()
    slack = 2.0 ** -24 * (x64.abs() + mu.abs() + sigma) / sigma * gamma.double().abs()
    return ref, slack


def norm_ratio(out, ref, slack, f32=False):
    """Worst (|out - ref| - 0.5 ulp) / slack over the elements (ulp: f16 spacing, fp32 spacing for the f32 entry points)."""
    o = out.double()
    ulp = torch.maximum(ulp32(ref), ulp32(o)) if f32 else torch.maximum(lc.ulp16(ref), lc.ulp16(o))
    excess = ((o - ref).abs() - 0.5 * ulp).clamp_min(0.0)
    ratio = torch.where(excess > 0, excess / slack.clamp_min(1e-300), torch.zeros_like(excess))
    ratio = torch.where(torch.isfinite(o), ratio, torch.full_like(ratio, float("inf")))
    return float(ratio.max())


def norm_mismatches(out, ref, slack, c, f32=False):
    """(count, first positions) of elements outside |out - ref| <= 0.5 ulp + c slack."""
    o = out.double()
    ulp = torch.maximum(ulp32(ref), ulp32(o)) if f32 else torch.maximum(lc.ulp16(ref), lc.ulp16(o))
    bad = ~((o - ref).abs() <= 0.5 * ulp + c * slack)
    return int(bad.sum()), lc._where(bad)


# ------------------------------------------------------------------------------------------------------------------ norms: builders
OFFSETS = (0.0, 8.0, 64.0)          # mean / sigma of a group (of a LayerNorm row)


def affine(C, device, dtype=torch.float16):
    """gamma in +-[0.5, 1.5], beta in [-0.5, 0.5]: different at every channel, no symmetry between a channel and its neighbours."""
    c = torch.arange(C, device=device, dtype=torch.float64)
    gamma = (1.0 + 0.5 * torch.sin(0.37 * c + 0.2)) * torch.where(c % 5 == 3, -1.0, 1.0)
    beta = 0.5 * torch.cos(0.91 * c + 1.1)
    return gamma.to(dtype), beta.to(dtype)


def gn_input(B, rows, C, groups, gen, dtype=torch.float16, offsets=OFFSETS):
    """x[b, r, c] = mu_g + sigma_g N(0, 1) with mean / sigma cycling through `offsets` over (b, g) and sigma through {0.5, 1, 2}: |x| < 1000."""
    dev = gen.device
    bg = torch.arange(B * groups, device=dev).view(B, 1, groups, 1)
    off = torch.tensor(offsets, device=dev)[bg % len(offsets)]
    sigma = torch.tensor([0.5, 1.0, 2.0], device=dev)[(bg // len(offsets)) % 3]
    sign = torch.where(bg % 2 == 0, 1.0, -1.0)
    x = (off * sigma * sign + sigma * torch.randn((B, rows, groups, C // groups), generator=gen, device=dev)).view(B, rows, C).to(dtype)
    assert float(x.abs().max()) < 1000.0
    return x


def gn_two_level(B, rows, C, groups, device, mu=64.0, a=1.0):
    """Half of every group's values at mu - a, half at mu + a (n = rows * C / groups must be even): mean = mu and variance = a^2 exactly,
    so a wrong count or an unbiased variance shows at every element."""
    cg = C // groups
    n = rows * cg
    assert n % 2 == 0, "two-level case: a group needs an even number of values"
    idx = torch.arange(n, device=device).view(rows, cg)
    lo = idx % 2 == 0
    bg = torch.arange(B * groups, device=device).view(B, 1, groups, 1)
    m = mu / 4 * torch.exp2((bg % 3).double())                               # mu / 4, mu / 2, mu: another mean in every group
    x = (m + torch.where(lo, -a, a).view(1, rows, 1, cg).double()).view(B, rows, C).to(torch.float16)
    xg = x.double().view(B, rows, groups, cg)
    assert bool((xg.sum((1, 3)) == n * m.view(B, groups)).all()) and bool((((xg - m) ** 2).sum((1, 3)) == n * a * a).all())      # integer sums: exact
    return x


def ln_input(rows, C, gen, dtype=torch.float16, offsets=OFFSETS):
    dev = gen.device
    r = torch.arange(rows, device=dev)[:, None]
    off = torch.tensor(offsets, device=dev)[r % len(offsets)]
    sigma = torch.tensor([0.5, 1.0, 2.0], device=dev)[(r // len(offsets)) % 3]
    sign = torch.where(r % 2 == 0, 1.0, -1.0)
    x = (off * sigma * sign + sigma * torch.randn((rows, C), generator=gen, device=dev)).to(dtype)
    assert float(x.abs().max()) < 1000.0
    return x


# ------------------------------------------------------------------------------------------------------------------ norms: defect models
NORM_DEFECTS = ["unbiased_variance", "row_count_off_by_one", "fp32_single_chain", "group_shift"]


def gn_model(x, groups, gamma, beta, eps, silu, defect=None):
    """A float64 model of GroupNorm(+SiLU) with one defect in its statistics; returns what the kernel would store (f16)."""
    x64 = x.double()
    B, rows, C = x64.shape
    cg = C // groups
    xg = x64.view(B, rows, groups, cg)
    n = rows * cg
    if defect == "fp32_single_chain":            # sum and sum of squares in ONE fp32 chain per group, then E[x^2] - mean^2 in fp32
        flat = xg.permute(0, 2, 1, 3).reshape(B * groups, n).float()
        s = torch.zeros(B * groups, dtype=torch.float32, device=x.device)
        ss = torch.zeros_like(s)
        for i in range(n):
            s = s + flat[:, i]
            ss = ss + flat[:, i] * flat[:, i]
        mean32 = s / n
        var32 = (ss / n - mean32 * mean32).clamp_min(0.0)
        mu = mean32.double().view(B, 1, groups, 1)
        var = var32.double().view(B, 1, groups, 1)
    else:
        if defect == "row_count_off_by_one":
            n = (rows + 1) * cg
        mu = xg.sum((1, 3), keepdim=True) / n
        var = ((xg * xg).sum((1, 3), keepdim=True) / n - mu * mu).clamp_min(0.0)
        if defect == "unbiased_variance":
            var = var * n / max(n - 1, 1)
    if defect == "group_shift":                  # group g + 1 is normalised with the statistics of group g
        mu, var = torch.roll(mu, 1, 2), torch.roll(var, 1, 2)
    z = ((xg - mu) / torch.sqrt(var + eps)).view(B, rows, C)
    y = z * gamma.double() + beta.double()
    return to_f16_rne(lc.act64(y, 1 if silu else 0))
