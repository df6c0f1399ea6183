#!/usr/bin/env python3
"""What an aspect-ratio edit costs: one process, one FastEditor (the bench configuration: SSD-1B + full ControlNet, fp16,
live tuner), whole FastEditor.edit() calls at 1024x1024 and at the buckets 1152x896, 1216x832 and 1344x768,
  * once with tile code 78 (the halo-resident conv with edge patches) available,
  * once with it excluded (fie_debug_tune_exclude("78"): the rule and the tuner fall back to the im2col ring kernels),
each size warmed up first (the first edit at a new size tunes its new shapes and captures its graph).  One JSON line per (mode, size): median ms
per edit over `rounds` edits and ms per megapixel; then the share of MFMA work code 78 spends on padding pixels for every off-16 map of each bucket.
Before the edits, one JSON line per conv map of the buckets (MAPS): forced 78 against every im2col code and the rule without 78, device time
with cold caches -- what the rule's choice of 78 rests on -- and, for the VAE's armed convs, what declining GroupNorm sums costs there.

    python tools/resolution_ab.py [--rounds 12] [--out FILE]"""
import argparse
import json
import math
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SIZES = [(1024, 1024), (1152, 896), (1216, 832), (1344, 768)]
PAD_SIZES = [(1152, 896), (1216, 832), (1344, 768), (1536, 640)]
# per-map A/B (batch, OH, OW, Cin, Cout, GroupNorm sums armed): the UNet's same-size convs of each bucket at CFG batch 2 whose maps are off the
# 16-grid, and the VAE's armed 512-channel convs (78 declines sums: what the rule runs there against 78 without sums)
MAPS = [(2, 56, 72, 640, 640, False), (2, 28, 36, 1280, 1280, False),
        (2, 104, 152, 320, 320, False), (2, 52, 76, 640, 640, False), (2, 26, 38, 1280, 1280, False),
        (2, 96, 168, 320, 320, False), (2, 48, 84, 640, 640, False), (2, 24, 42, 1280, 1280, False),
        (2, 40, 96, 640, 640, False), (2, 20, 48, 1280, 1280, False),
        (1, 104, 152, 512, 512, True), (1, 96, 168, 512, 512, True)]
IM2COL = (42, 43, 44, 46, 51, 52, 54, 81, 96)


def padding_fractions(w, h):
    """Maps of an edit at w x h whose sides are not both multiples of 16 -> fraction of code 78's MFMA work spent on pixels outside the image
    (patches are 16x16; the UNet runs at latents / 1, 2, 4, the VAE at latents x 1, 2, 4, 8)."""
    lw, lh = w // 8, h // 8
    out = {}
    maps = [("unet", lw // d, lh // d) for d in (1, 2, 4)] + [("vae", lw * m, lh * m) for m in (1, 2, 4, 8)]
    for tag, mw, mh in maps:
        if mw % 16 == 0 and mh % 16 == 0:
            continue
        padded = math.ceil(mw / 16) * 16 * math.ceil(mh / 16) * 16
        out[f"{tag} {mw}x{mh}"] = round(1 - mw * mh / padded, 4)
    return out


def conv_ab(ctx, reps=15):
    """Device time (median us, weights and activations flushed from the caches before every launch, as the tuner times) of each map in MAPS:
    forced 78, every im2col code, and the built-in rule without 78; for the armed VAE maps the rule's launch carries the GroupNorm sums."""
    import torch
    from fie_amd import hip
    flush = torch.empty(384 << 20, dtype=torch.uint8, device=ctx.device)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    ctx.autotune(0)
    g = torch.Generator().manual_seed(0)
    out = []
    for b, h, w, cin, cout, armed in MAPS:
        x = torch.randn(b, h, w, cin, generator=g).half().to(ctx.device)
        wp = ctx.pack_conv3x3((torch.randn(cout, cin, 3, 3, generator=g) * (9 * cin) ** -0.5).half().to(ctx.device))
        bias = torch.randn(cout, generator=g).half().to(ctx.device)

        def timed(code, gn):
            ctx.force_tile(code)
            ts = []
            try:
                for r in range(reps + 2):
                    flush.fill_(r & 1)
                    e0.record()
                    ctx.conv3x3(x, wp, cout, bias=bias, gn_groups=32 if gn else None)
                    e1.record()
                    e1.synchronize()
                    if r >= 2:
                        ts.append(e0.elapsed_time(e1) * 1e3)
                return round(statistics.median(ts), 1), hip.last_gemm_kernel(ctx)
            except hip.FieError:
                return None, None
            finally:
                ctx.force_tile(0)
        rec = dict(map=f"{b}x{w}x{h}", cin=cin, cout=cout, gn_armed=armed)
        rec["us_78"] = timed(78, False)[0]
        codes = {c: timed(c, False)[0] for c in IM2COL}
        codes = {c: t for c, t in codes.items() if t is not None}
        best = min(codes, key=codes.get)
        rec["us_best_im2col"], rec["best_im2col_code"] = codes[best], best
        rec["us_rule"], rec["rule"] = timed(0, armed)
        ctx.tune_exclude("78")
        rec["us_rule_without_78"], rec["rule_without_78"] = timed(0, armed)
        ctx.tune_exclude("")
        if rec["us_78"]:
            rec["ratio_78_vs_best_im2col"] = round(rec["us_78"] / codes[best], 3)
        out.append(rec)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=12)
    ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
    args = ap.parse_args()
    import torch
    import fie_amd  # noqa: F401
    from bench import synth_item_image
    from src.pipeline import FastEditor

    ed = FastEditor(model_name="ssd-1b", use_full_controlnet=True, enable_cpu_offload=False)
    pipe, ctx = ed.pipe, ed.pipe.ctx
    src = synth_item_image(3)
    kw = dict(prompt="a [red] ball on the table", seed=42)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)

    def emit(rec):
        s = json.dumps(rec)
        print(s, flush=True)
        if args.out:
            with open(args.out, "a") as f:
                f.write(s + "\n")

    for rec in conv_ab(ctx):
        emit(rec)

    for mode, excl in (("with_78", ""), ("without_78", "78")):
        ctx.tune_exclude(excl)                                   # forgets the remembered choices: every shape is tuned again
        pipe._drop_graphs()
        for w, h in SIZES:
            t0 = time.perf_counter()
            ed.edit(src, resolution=(w, h), **kw)                # tunes the new shapes, captures
            ed.edit(src, resolution=(w, h), **kw)
            warm = time.perf_counter() - t0
            ts = []
            for _ in range(args.rounds):
                torch.cuda.synchronize()
                t = time.perf_counter()
                ed.edit(src, resolution=(w, h), **kw)
                ts.append((time.perf_counter() - t) * 1e3)
            ms = statistics.median(ts)
            emit(dict(mode=mode, size=f"{w}x{h}", ms_per_edit=round(ms, 2), ms_per_mpix=round(ms / (w * h / 1e6), 2),
                      min_ms=round(min(ts), 2), warmup_s=round(warm, 1), rounds=args.rounds))
    ctx.tune_exclude("")
    for w, h in PAD_SIZES:
        emit(dict(padding_fraction_78=f"{w}x{h}", maps=padding_fractions(w, h)))


if __name__ == "__main__":
    main()
