"""Every tile the tuner can pick, at every GEMM / 3x3-conv problem the product runs (tests/golden/launch_problems.json, written by
tools/launch_problems.py), against float64 references computed on the device.

For each in-scope problem the call is rebuilt with the fixture's geometry and epilogue and run with the rule's code, every code the library's
own candidate list names (include/fie.h: fie_debug_tune_candidates -- exactly what autotune times) and the code tests/golden/tune_table.txt
holds for the problem (printed as stale when today's list no longer has it), each forced through fie_debug_force_tile.  Three passes:

  1  integer data (A, W in {-2..2}, integer bias / row bias / residual): every fp32 partial sum is exact, so every code must give the float64
     result rounded once to f16, bit for bit.  fp8 weights: within 1 ulp (the fp32 per-channel scale multiply); SiLU / GELU / GEGLU: within
     1 ulp of act(exact sum); e4m3 outputs: within 1 e4m3 ulp.  GroupNorm partial sums from the epilogue: per (image, group) totals.
  2  real data with a non-zero mean (A ~ N(0.25, 1), W ~ N(0.25, 1) / sqrt(K)): |out - ref| <= 0.5 ulp16 + C_FP32 sqrt(K) 2^-24 (|A||W|)
     per element.
  3  the pass-2 outputs of the codes that accumulate K in the same order (the im2col ring and phased codes, no split-K) are bit-identical.
"""
import json
import math
import os
import time

import pytest
import torch

import launch_check as lc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "launch_problems.json")
TUNE_TABLE = os.path.join(ROOT, "tests", "golden", "tune_table.txt")

# pass 2's constant: the worst measured (|out - ref| - 0.5 ulp16) / (sqrt(K) 2^-24 |A||W|) over every (problem, code) pair was MEASURED_RATIO
# (one MI355X run of this module: gemm M 8192 x N 640 x K 640, fp8 activations, tile 43); C_FP32 leaves 2x head-room above it.  An fp16-
# accumulating kernel lands near 200 already with 16-wide fp32 MFMA steps (tests/test_launch_check_cpu.py: test_precision_check_flags_fp16_accumulation
# shows where), 25x above C_FP32.
MEASURED_RATIO = 3.81
C_FP32 = 8.0
# fp8-weight flows (w8 = 1) convert each f16 activation to e4m3 in registers (csrc/gemm_w8.hip); the reference models that with torch's
# f16 -> e4m3 conversion, which disagrees with the hardware's in a few elements per problem (measured: worst ratio MEASURED_RATIO_W8 at K = 320,
# 40 of 2.6M elements; every tile agrees with every other): their own constant until the conversion is pinned down (profiles/r05_launch_table.md)
MEASURED_RATIO_W8 = 8.93
C_W8 = 16.0
# pass 1's absolute floor for results that are not a single rounding of the exact sum: the fp32 per-channel scale of the fp8 flows (2^-22 of the
# |.| budget: cancellation against a bias leaves a residue of a few fp32 ulps where the exact result is 0) and the fp32 activations (2^-18: the
# GELU's erf approximation near its tails)
FLOOR_SCALE, FLOOR_ACT = 2.0 ** -22, 2.0 ** -18
# codes that sum K in another order than the im2col tiles: the halo-resident convs (chunk-major), the thin conv, split-K encodings
SAME_ORDER_EXEMPT = {71, 72, 73, 74, 76, 77}
ACT_GEGLU = 4


def _tile_table():
    table = {}
    for line in open(TUNE_TABLE):
        if "->" in line and not line.startswith("#"):
            k, v = line.rsplit("->", 1)
            table[k.strip()] = int(v)
    return table


def _geometry(p):
    if p["kind"] == "gemm":
        return None
    hin, win = p["H"] << p["ups"], p["W"] << p["ups"]
    pads = 2 if p["pad"] == 0 else 1
    s = p["stride"]
    return {"stride": s, "pt": 1 if p["pad"] == 0 else 0, "OH": (hin + pads - 3) // s + 1, "OW": (win + pads - 3) // s + 1}


class Problem:
    """One fixture record, rebuilt: inputs of one pass, the launch of one code, the float64 reference (and its |A||W| twin)."""

    def __init__(self, ctx, p):
        self.ctx, self.p = ctx, p
        self.kind, self.w8 = p["kind"], p["w8"]
        self.N, self.K = p["N"], p["K"]
        self.act = p["act"]
        self.nout = self.N // 2 if self.act == ACT_GEGLU else self.N
        self.geo = _geometry(p)
        if self.kind == "gemm":
            self.M = p["M"]
        elif p["parity"]:
            self.M = p["M"]                       # all four parities: [B, 2H, 2W]
        else:
            self.M = p["b"] * self.geo["OH"] * self.geo["OW"]

    # ---------------------------------------------------------------- data
    def make(self, integer, gen):
        p, dev, K = self.p, self.ctx.device, self.K

        def ints(shape, r):
            return torch.randint(-r, r + 1, shape, generator=gen, device=dev).to(torch.float16)

        def reals(shape, scale=1.0):
            return ((torch.randn(shape, generator=gen, device=dev) + 0.25) * scale).to(torch.float16)

        rw = 1 if self.act == ACT_GEGLU else 2
        A = (lambda s: ints(s, 2)) if integer else reals
        Wf = (lambda s: ints(s, rw)) if integer else (lambda s: reals(s, 1.0 / math.sqrt(K)))
        E = (lambda s: ints(s, 4)) if integer else reals
        d = {}
        if self.kind == "gemm":
            d["a1"] = A((self.M, p["K1"]))
            d["a2"] = A((self.M, K - p["K1"])) if p["K1"] < K else None
            wl = Wf((self.N, K))
        elif p["parity"]:
            d["x"] = A((p["b"], p["H"], p["W"], p["Cin"]))
            wl = Wf((4, self.N, K))              # the four parity matrices, k = (a * 2 + b) * Cin + ci
        else:
            d["x"] = A((p["b"], p["H"], p["W"], p["Cin"]))
            d["x2"] = A((p["b"] * p["H"] * p["W"], p["C2"])) if p["C2"] else None
            d["x3"] = A((p["b"] * p["H"] * p["W"], p["C3"])) if p["C3"] else None
            wl = Wf((self.N, K))                 # k = tap * Cin + ci, then the C2 / C3 side-input columns
        if self.w8 == 2:                         # e4m3 activations, fed directly (dequantisation scale a_scale)
            key = "a1" if self.kind == "gemm" else "x"
            d[key] = d[key].float().to(torch.float8_e4m3fn).view(torch.uint8)
            d["a_scale"] = 0.5
        d["bias"] = E((self.N,)) if p["bias"] else None
        if p["rowbias"]:
            rows = self.M // p["rpb"] if self.kind == "gemm" else p["b"]
            d["rowbias"] = E((rows, self.N))
        else:
            d["rowbias"] = None
        d["res"] = E((self.M, self.nout)) if p["res"] else None
        d["wl"] = wl
        d["wp"] = self._pack(wl)
        return d

    def _pack(self, wl):
        """Packed weights as the kernels read them: f16 [Npad][Kpad] (zero padded; parity: [4][Npad][Kpad]) or the library's fp8 quantisation."""
        ctx, N, K = self.ctx, self.N, self.K
        npad, kpad = (N + 127) // 128 * 128, (K + 63) // 64 * 64
        if self.w8:
            w8, ctx.w8 = ctx.w8, True
            try:
                return ctx.pack_linear(wl, quant=True)
            finally:
                ctx.w8 = w8
        if self.p["parity"]:
            out = torch.zeros((4, npad, kpad), device=ctx.device, dtype=torch.float16)
            out[:, :N, :K] = wl
            return out
        out = torch.zeros((npad, kpad), device=ctx.device, dtype=torch.float16)
        out[:N, :K] = wl
        return out

    def weights64(self, d):
        """[N, K] float64 weights the kernel multiplies with (fp8: the packed bytes read back, dequantised)."""
        if self.w8:                              # (in float64: W8.dequant() multiplies in fp32)
            wp = d["wp"]
            return (wp.q.view(torch.float8_e4m3fn).double() * wp.scale.double()[:, None])[:self.N, :self.K]
        return d["wl"].double()

    # ---------------------------------------------------------------- launch
    def launch(self, d, gn=None):
        from fie_amd import hip
        ctx, p, L = self.ctx, self.p, hip.lib()
        P = hip._p
        ctx.sync_stream()
        ctx._bind_splitk()
        out_dtype = torch.uint8 if p["f8out"] else torch.float16
        if gn is not None:
            hip._chk(L.fie_gn_stats_target(ctx.h, P(gn[0]), gn[1], gn[2]))
        rb, rbld = d["rowbias"], (d["rowbias"].stride(0) if d["rowbias"] is not None else 0)
        res, resld = d["res"], (d["res"].stride(0) if d["res"] is not None else 0)
        if self.kind == "gemm":
            out = torch.empty((self.M, self.nout), device=ctx.device, dtype=out_dtype)
            a1, a2 = d["a1"], d["a2"]
            if self.w8 == 2:
                hip._chk(L.fie_gemm_x8_f16(ctx.h, P(a1), a1.stride(0), P(d["wp"].q), d["wp"].stride(0), P(d["wp"].scale), float(d["a_scale"]), P(out),
                                           out.stride(0), self.M, self.N, self.K, P(d["bias"]), P(rb), rbld, p["rpb"], P(res), resld, float(p["scale"]),
                                           self.act, int(p["f8out"]), 0.25 if p["f8out"] else 1.0))
            elif self.w8 == 1:
                hip._chk(L.fie_gemm_w8_f16(ctx.h, P(a1), a1.stride(0), p["K1"], P(a2), a2.stride(0) if a2 is not None else 0, P(d["wp"].q), d["wp"].stride(0),
                                           P(d["wp"].scale), P(out), out.stride(0), self.M, self.N, self.K, P(d["bias"]), P(rb), rbld, p["rpb"], P(res), resld,
                                           float(p["scale"]), self.act))
            else:
                hip._chk(L.fie_gemm_f16(ctx.h, P(a1), a1.stride(0), p["K1"], P(a2), a2.stride(0) if a2 is not None else 0, P(d["wp"]), d["wp"].stride(0),
                                        P(out), out.stride(0), self.M, self.N, self.K, P(d["bias"]), P(rb), rbld, p["rpb"], P(res), resld,
                                        float(p["scale"]), self.act))
            return out
        x, g = d["x"], self.geo
        b, H, W, C = x.shape
        if p["parity"]:
            out = torch.empty((b, 2 * H, 2 * W, self.N), device=ctx.device, dtype=torch.float16)
            wp = d["wp"]
            hip._chk(L.fie_conv_up2x_nhwc_f16(ctx.h, P(x), b, H, W, C, P(wp), wp.stride(1), wp.shape[1], P(out), out.stride(2), self.N, P(d["bias"]),
                                              P(rb), rbld, float(p["scale"]), self.act))
            return out.view(-1, self.N)
        out = torch.empty((b, g["OH"], g["OW"], self.N), device=ctx.device, dtype=torch.float16)
        resld = d["res"].stride(0) if d["res"] is not None else 0
        if p["C2"]:
            x2, x3 = d["x2"], d["x3"]
            hip._chk(L.fie_conv3x3_plus_nhwc_f16(ctx.h, P(x), b, H, W, C, P(d["wp"]), d["wp"].stride(0), P(out), out.stride(2), self.N, P(d["bias"]), P(rb), rbld,
                                                 float(p["scale"]), self.act, P(x2), x2.stride(0), p["C2"], P(x3), x3.stride(0) if x3 is not None else 0,
                                                 p["C3"]))
        elif self.w8 == 2:
            hip._chk(L.fie_conv3x3_x8_nhwc_f16(ctx.h, P(x), b, H, W, C, p["ups"], p["stride"], p["pad"], P(d["wp"].q), d["wp"].stride(0), P(d["wp"].scale),
                                               float(d["a_scale"]), P(out), out.stride(2), self.N, P(d["bias"]), P(rb), rbld, P(res), resld,
                                               float(p["scale"]), self.act))
        elif self.w8 == 1:
            hip._chk(L.fie_conv3x3_w8_nhwc_f16(ctx.h, P(x), b, H, W, C, p["ups"], p["stride"], p["pad"], P(d["wp"].q), d["wp"].stride(0), P(d["wp"].scale),
                                               P(out), out.stride(2), self.N, P(d["bias"]), P(rb), rbld, P(res), resld, float(p["scale"]), self.act))
        else:
            hip._chk(L.fie_conv3x3_nhwc_f16(ctx.h, P(x), b, H, W, C, p["ups"], p["stride"], p["pad"], P(d["wp"]), d["wp"].stride(0), P(out), out.stride(2),
                                            self.N, P(d["bias"]), P(rb), rbld, P(res), resld, float(p["scale"]), self.act))
        return out.view(-1, self.N)

    # ---------------------------------------------------------------- references
    def _a64(self, t):
        """An activation operand as the MFMA sees it: e4m3 bytes decoded; under fp8 weights (w8 = 1) the kernel converts each f16 activation to
        e4m3 in registers (clamp to +-448, round to nearest even: csrc/gemm_w8.hip), so the reference does the same."""
        if t.dtype == torch.uint8:
            return t.view(torch.float8_e4m3fn).double()
        if self.w8 == 1:
            return t.float().clamp(-448.0, 448.0).to(torch.float8_e4m3fn).double()
        return t.double()

    def accum64(self, d, absolute=False):
        """The accumulator (A W^T, times the fp8 scales) in float64, [M, N]; absolute: |A| |W|."""
        f = (lambda t: t.abs()) if absolute else (lambda t: t)
        w = f(self.weights64(d))
        p, K = self.p, self.K
        if self.kind == "gemm":
            acc = f(self._a64(d["a1"])) @ w[:, :p["K1"]].t()
            if d["a2"] is not None:
                acc += f(self._a64(d["a2"])) @ w[:, p["K1"]:].t()
        elif p["parity"]:
            x = f(d["x"].double())
            b, H, W, C = x.shape
            full = x.new_empty((b, 2 * H, 2 * W, self.N))
            for py in range(2):
                for px in range(2):
                    wq = w[py * 2 + px] if w.dim() == 3 else None
                    taps = [(a + py, bb + px, wq[:, (a * 2 + bb) * C:(a * 2 + bb + 1) * C]) for a in range(2) for bb in range(2)]
                    full[:, py::2, px::2] = lc.conv_taps64(x, taps, {"stride": 1, "pt": 1, "OH": H, "OW": W}).view(b, H, W, self.N)
            acc = full.view(-1, self.N)
        else:
            x = f(self._a64(d["x"]))
            if p["ups"]:
                x = x.repeat_interleave(2, 1).repeat_interleave(2, 2)
            C = p["Cin"]
            taps = [(t // 3, t % 3, w[:, t * C:(t + 1) * C]) for t in range(9)]
            acc = lc.conv_taps64(x, taps, self.geo)
            if p["C2"]:
                acc += f(d["x2"].double()) @ w[:, 9 * C: 9 * C + p["C2"]].t()
            if p["C3"]:
                acc += f(d["x3"].double()) @ w[:, 9 * C + p["C2"]:].t()
        if self.w8 == 2:
            acc *= d["a_scale"]
        return acc

    def reference(self, d, absolute=False):
        """Float64 output [M, nout]: act(acc + bias + row bias) * scale + residual; absolute: the matching |.| error budget."""
        p = self.p
        acc = self.accum64(d, absolute)
        f = (lambda t: t.abs()) if absolute else (lambda t: t)
        if d["bias"] is not None:
            acc += f(d["bias"].double())
        if d["rowbias"] is not None:
            per = p["rpb"] if self.kind == "gemm" else self.M // p["b"]
            acc += f(d["rowbias"].double()).repeat_interleave(per, 0)
        if absolute:
            h = self.reference_pre_act(d) if self.act else None
            y = lc.act_abs64(h, acc, self.act) * p["scale"]
        else:
            y = lc.act64(acc, self.act) * p["scale"]
        if d["res"] is not None:
            y += f(d["res"].double())
        return y

    def reference_pre_act(self, d):
        p = self.p
        acc = self.accum64(d)
        if d["bias"] is not None:
            acc += d["bias"].double()
        if d["rowbias"] is not None:
            per = p["rpb"] if self.kind == "gemm" else self.M // p["b"]
            acc += d["rowbias"].double().repeat_interleave(per, 0)
        return acc


def _decode(v):
    return v % 1000, (v // 10000 if v // 10000 > 1 else 1)


def _ran_code(name):
    """(tile code, split) that fie_debug_last_gemm_kernel names."""
    code = int(name.split("tile code ")[1].split(",")[0].split(")")[0])
    split = int(name.split("split-K ")[1].split(")")[0]) if "split-K" in name else 1
    return code, split


@pytest.mark.gpu
def test_every_candidate_tile_at_every_product_problem(fie):
    from fie_amd import hip
    ctx = fie
    doc = json.load(open(FIXTURE))
    table = _tile_table()
    probs = [p for p in doc["problems"] if p["in_scope"]]
    print(f"\n[launch table] {len(doc['problems'])} problems in the fixture, {len(probs)} in scope "
          f"({len(doc['problems']) - len(probs)} LayerNorm-folded / GroupNorm-applied: out of scope)")
    gen = torch.Generator(device=ctx.device)
    failures, stale, worst, same_order_diff = [], [], {"fp32": (0.0, None), "w8": (0.0, None)}, []
    pairs = expected_pairs = fixture_pairs = 0
    t0 = time.time()
    for pi, p in enumerate(probs):
        prob = Problem(ctx, p)
        tag = f"{p['key']} act={p['act']} C2={p['C2']} bias={p['bias']} rowbias={p['rowbias']} res={p['res']} gn={p['gn']} f8out={p['f8out']}"
        gen.manual_seed(1000 + pi)
        d1 = prob.make(True, gen)
        # what the tuner would time here, from the library itself
        ctx.force_tile(0)
        ctx.tune_candidates(True)
        try:
            prob.launch(d1)
            lines = ctx.tune_candidates_read()
        finally:
            ctx.tune_candidates(False)
        assert len(lines) == 1 and lines[0][0] == p["key"], f"{tag}: candidate query returned {lines}"
        _, rule, cands = lines[0]
        assert rule == p["rule"], f"{tag}: the rule picks {rule} today, the fixture recorded {p['rule']}"
        codes = [rule] + cands
        if cands != p["cands_recorded"]:
            print(f"[launch table] {p['key']}: candidates today {cands}, the fixture recorded {p['cands_recorded']}")
        tv = table.get(p["key"])
        if tv is not None and tv not in codes:
            c, s = _decode(tv)
            if (c + 10000 * s if s > 1 else c) in codes:
                codes.append(tv)                         # the table's forced tile order of a listed code
            else:
                stale.append(f"{p['key']} -> {tv}")
        expected_pairs += len(codes)
        fixture_pairs += 1 + len(p["cands_recorded"])
        # pass 1: integer data, single-rounded exact result
        ref1 = prob.reference(d1)
        floor1 = (FLOOR_ACT if p["act"] else FLOOR_SCALE) * prob.reference(d1, absolute=True) if (prob.w8 or p["act"]) else 0.0
        gnb = None
        if p["gn"]:
            rows = p["gnrows"] * (4 if p["parity"] else 1)
            nb = prob.M // rows
            gnb = (torch.empty(hip.lib().fie_gn_stats_bytes(nb, rows, p["gn"]) // 4, device=ctx.device, dtype=torch.float32), rows, p["gn"], nb)
        for code in codes:
            c, s = _decode(code)
            ctx.force_tile(code)
            try:
                out = prob.launch(d1, gnb)
                name = hip.last_gemm_kernel(ctx)
            finally:
                ctx.force_tile(0)
            ran = _ran_code(name)
            if code != rule or not prob.w8:              # the fp8 flows map the rule's f16 code onto their own tile set
                assert ran == (c, s), f"{tag}: forced {code}, ran {name}"
            pairs += 1
            if p["f8out"]:
                n, where = lc.f8_mismatches(out, ref1 * 0.25, 1, floor1 * 0.25)
            elif prob.w8 or p["act"]:
                n, where = lc.ulp_mismatches(out, ref1, 1, floor1)
            else:
                n, where = lc.exact_mismatches(out, ref1)
            if n:
                i = where[0]
                failures.append(f"pass 1 {tag} code {code} ({name}): {n} elements differ from the single-rounded exact result, first at {where}: "
                                f"out {float(out[i].float()) if not p['f8out'] else int(out[i])} ref {float(ref1[i]):.6f}")
            if gnb is not None:
                o = out.double().view(gnb[3], gnb[1], p["gn"], -1)
                part = gnb[0].double().view(gnb[3], -1, p["gn"], 2).sum(1)
                ref_s, ref_q = o.sum((1, 3)), (o * o).sum((1, 3))
                tol = 1e-5 * (o.abs().sum((1, 3)) + 1)
                if not ((part[..., 0] - ref_s).abs() <= tol).all() or not ((part[..., 1] - ref_q).abs() <= 1e-5 * ref_q + 1).all():
                    failures.append(f"pass 1 {tag} code {code}: GroupNorm partial sums disagree with the stored output")
        del d1, ref1, floor1
        # pass 2: real data, per-element bound; pass 3: bit identity among the same-order codes
        if p["f8out"]:
            continue                                     # e4m3 outputs: pass 1 only (their rounding step is 1/8 of a binade)
        gen.manual_seed(5000 + pi)
        d2 = prob.make(False, gen)
        ref2, abs2 = prob.reference(d2), prob.reference(d2, absolute=True)
        base = None
        for code in codes:
            ctx.force_tile(code)
            try:
                out = prob.launch(d2)
            finally:
                ctx.force_tile(0)
            r = lc.precision_ratio(out, ref2, abs2, prob.K)
            cls = "w8" if prob.w8 == 1 else "fp32"
            if r > worst[cls][0]:
                worst[cls] = (r, f"{tag} code {code}")
            c_max = C_W8 if prob.w8 == 1 else C_FP32
            if r > c_max:
                n, where = lc.precision_mismatches(out, ref2, abs2, prob.K, c_max)
                failures.append(f"pass 2 {tag} code {code}: ratio {r:.2f} > {c_max} at {n} elements, first at {where}")
            c, s = _decode(code)
            ran = _ran_code(hip.last_gemm_kernel(ctx))
            if s == 1 and ran[1] == 1 and ran[0] not in SAME_ORDER_EXEMPT:
                if base is None:
                    base = (ran[0], out)
                elif not torch.equal(out.view(torch.int16), base[1].view(torch.int16)):
                    same_order_diff.append(f"{tag}: code {ran[0]} differs from code {base[0]} in {int((out != base[1]).sum())} elements")
        del d2, ref2, abs2, base
    dt = time.time() - t0
    print(f"[launch table] {len(probs)} problems, {pairs} (problem, code) pairs checked: candidate lists + rules + table entries imply {expected_pairs}, "
          f"the fixture's recorded lists {fixture_pairs}; {dt:.1f} s")
    print(f"[launch table] pass 2: worst ratio {worst['fp32'][0]:.3f} (C_FP32 = {C_FP32}) at {worst['fp32'][1]}")
    print(f"[launch table] pass 2, fp8 weights: worst ratio {worst['w8'][0]:.3f} (C_W8 = {C_W8}) at {worst['w8'][1]}")
    for s in stale:
        print(f"[launch table] stale table entry (not in today's candidate list): {s}")
    for s in same_order_diff:
        print(f"[launch table] pass 3: {s}")
    for f in failures:
        print(f"[launch table] FAIL {f}")
    assert pairs == expected_pairs
    assert not failures, f"{len(failures)} (problem, code) checks failed (printed above)"
    assert not same_order_diff, f"{len(same_order_diff)} problems where same-order codes differ in bits (printed above)"
