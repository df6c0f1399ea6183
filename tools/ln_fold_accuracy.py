#!/usr/bin/env python3
"""Where folding the LayerNorm into its GEMM stops being as accurate as LayerNorm + GEMM (the table of profiles/ln_fold_pins.md): per row class of
tests/ln_fold_check.py (common offset 0 / 3 / 30 / 300 sigma, sigma 0.01, constant rows), the error of the folded launch (fie_gemm_ln_f16) and of the
two-launch sequence (fie_layernorm_f16 -> fie_gemm_f16) against the TRUE LayerNorm -> Linear in float64 (unfolded, unrounded W * gamma), as
max |out - true| / rms(true) over the class.  A table, not a test.  usage: tools/ln_fold_accuracy.py [M=1536] [N=1280] [K=1280] [eps=1e-5]"""
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import fie_amd  # noqa: E402,F401
import ln_fold_check as lf  # noqa: E402
from fie_amd import hip  # noqa: E402

M, N, K = (int(sys.argv[i]) if len(sys.argv) > i else d for i, d in ((1, 1536), (2, 1280), (3, 1280)))
eps = float(sys.argv[4]) if len(sys.argv) > 4 else 1e-5
ctx = hip.context(0)
case = lf.real_case(M, N, K, torch.Generator().manual_seed(1))
dev = lambda t: t.to(ctx.device)
x = dev(case["x"])
wp, tab = ctx.fold_layernorm(case["w"], case["bias"], case["gamma"], case["beta"])
folded = ctx.gemm_ln(x, wp, N, tab, eps=eps)
kern = hip.last_gemm_kernel(ctx)
two = ctx.gemm(ctx.layernorm(x, dev(case["gamma"]), dev(case["beta"]), eps), ctx.pack_linear(dev(case["w"])), N, bias=dev(case["bias"]))
true = lf.layernorm_linear64(x, {k: (dev(v) if torch.is_tensor(v) else v) for k, v in case.items()}, eps)
own = lf.reference(x, wp[:N, :K], tab, eps)
print(f"M={M} N={N} K={K} eps={eps}; folded launch: {kern}")
print("| row class | folded vs true | LayerNorm + GEMM vs true | folded vs its own float64 formula | worst pass-2 ratio |")
print("|---|---|---|---|---|")
cls = dev(case["cls"])
for c, name in enumerate(lf.ROW_CLASSES):
    rows = cls == c
    t = true[rows]
    rms = float(t.pow(2).mean().sqrt())
    err = lambda o: float((o[rows].double() - t).abs().max()) / rms
    e_own = float((folded[rows].double() - own.ref[rows]).abs().max()) / rms
    ratio = lf.pass2_ratio(folded[rows], lf.Ref(own.ref[rows], own.budget[rows], None, None, None), K)
    print(f"| {name} | {err(folded):.2e} | {err(two):.2e} | {e_own:.2e} | {ratio:.3f} |")
