#!/usr/bin/env python3
"""What a tiled edit's back end costs: one process, interleaved rounds, the A/A spread reported.

    python tools/tile_blend_ab.py [--rounds 20] [--calls 20] [--model ssd-1b | --no_edit] [--out profiles/tile_blend.md]

(a) the op alone, fie_tile_blend_rgb_u8 at 4000x3000 (the "auto" plan at overlap 128: 5 x 4 tiles of 960 x 896), device events around windows of
    `calls` launches, `rounds` windows per form, the forms taken one after the other inside each round:
      op          the blend (the C entry itself, its arguments prepared once), every call on the next of several operand sets that together
                  exceed the 256 MiB Infinity Cache: HBM traffic
      op (A)      the same again: the A/A spread of this script
      op, hot     the blend on ONE operand set (88 MB: it stays in the Infinity Cache)
      copy        torch's device-to-device copy of as many bytes as the op must move, on rotating buffers: what plain streaming achieves here
    against the op's compulsory traffic, 3 * (sum of the coverage + 1) bytes per output pixel, over the 6.0 - 6.3 TB/s an MI355X achieves.
(b) the whole call, wall clock host in -> host out, alternating: FastEditor.edit(image, tiles="auto") against what the same result costs
    without the feature -- edit_batch on PIL crops, job by job, PIL tiles back, tiles.blend_numpy on the host.
(c) the two outputs of (b), byte for byte."""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ACHIEVABLE = (6.0e12, 6.3e12)          # bytes/s a streaming kernel reaches on an MI355X (of 8 TB/s peak)
CACHE_BYTES = 256 << 20                # Infinity Cache


def quant(v):
    s = sorted(v)
    return statistics.median(s), s[len(s) // 10], s[(len(s) * 9) // 10]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="ssd-1b", choices=["ssd-1b", "sdxl", "tiny"])
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--calls", type=int, default=20, help="launches per timed window")
    ap.add_argument("--edit_rounds", type=int, default=5)
    ap.add_argument("--tile_batch", type=int, default=4)
    ap.add_argument("--no_edit", action="store_true", help="part (a) only")
    ap.add_argument("--out", default=None, help="also write the report there, as markdown")
    args = ap.parse_args()
    import numpy as np
    import torch
    from PIL import Image
    import fie_amd  # noqa: F401
    from bench import synth_item_image
    from fie_amd import hip, tiles

    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    W, H, overlap = 4000, 3000, 128
    tw, th, xs, ys = tiles.plan((W, H), "auto", overlap)
    n = len(xs) * len(ys)
    ctx = hip.context(0)
    dev = ctx.device
    moved = 3 * (n * th * tw + H * W)                   # every tile byte read once, every output byte written once
    sets = CACHE_BYTES // moved + 3                     # operand sets that together exceed the cache, with room
    g = torch.Generator(device="cpu").manual_seed(0)
    tl = [torch.randint(0, 256, (n, th, tw, 3), dtype=torch.uint8, generator=g).to(dev) for _ in range(sets)]
    outs = [torch.empty((H, W, 3), dtype=torch.uint8, device=dev) for _ in range(sets)]
    a = [torch.empty(moved // 2, dtype=torch.uint8, device=dev) for _ in range(sets)]
    b = [torch.empty(moved // 2, dtype=torch.uint8, device=dev) for _ in range(sets)]
    turn = {"i": 0}

    # the C entry itself, arguments prepared once: the Python wrapper's checks cost more host time per call than the kernel runs
    import ctypes
    cx, cy = (ctypes.c_int * len(xs))(*xs), (ctypes.c_int * len(ys))(*ys)
    entry = hip.lib().fie_tile_blend_rgb_u8
    ctx.sync_stream()

    def blend(i):
        hip._chk(entry(ctx.h, tl[i].data_ptr(), len(xs), len(ys), cx, cy, th, tw, H, W, outs[i].data_ptr()))

    def rotating():
        i = turn["i"] = (turn["i"] + 1) % sets
        blend(i)

    def copy():
        i = turn["i"] = (turn["i"] + 1) % sets
        b[i].copy_(a[i])

    forms = {"op": rotating, "op (A)": rotating, "op, hot": lambda: blend(0), "copy": copy}
    say(f"# `tiles=` A/B (`tools/tile_blend_ab.py`)")
    say()
    say(f"{torch.cuda.get_device_name(0)}; {args.rounds} interleaved rounds of windows of {args.calls} calls (op); model {args.model}, "
        f"{args.edit_rounds} alternating rounds (whole call).")
    say()
    say(f"## (a) The op alone: {W} x {H} from {len(xs)} x {len(ys)} tiles of {tw} x {th} (plan \"auto\", overlap {overlap})")
    say()
    want = tiles.blend_numpy(tl[0].cpu().numpy(), xs, ys, H, W)
    differ = int((ctx.tile_blend(tl[0], xs, ys, H, W).cpu().numpy() != want).sum())
    say(f"Against `tiles.blend_numpy` on the same tiles: {differ} differing bytes of {want.size}.")
    say(f"Compulsory traffic 3 * (sum of the coverage + 1) bytes per pixel = {moved / (H * W):.2f} B/pixel = {moved / 1e6:.1f} MB a call "
        f"(coverage {n * th * tw / (H * W):.3f}); at {ACHIEVABLE[0] / 1e12:.1f} - {ACHIEVABLE[1] / 1e12:.1f} TB/s that is "
        f"{moved / ACHIEVABLE[1] * 1e6:.1f} - {moved / ACHIEVABLE[0] * 1e6:.1f} us.  {sets} operand sets in rotation ({sets * moved / 2**20:.0f} MiB).")
    say()
    for f in forms.values():
        for _ in range(2 * sets):
            f()
    torch.cuda.synchronize()
    us = {k: [] for k in forms}
    for _ in range(args.rounds):
        for k, f in forms.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(args.calls):
                f()
            e1.record()
            e1.synchronize()
            us[k].append(e0.elapsed_time(e1) * 1e3 / args.calls)
    say("| form | us per call: median [10 %, 90 %] | GB/s of the compulsory bytes at the median | share of 6.0 - 6.3 TB/s |")
    say("|---|---|---|---|")
    for k in forms:
        med, lo, hi = quant(us[k])
        rate = moved / (med * 1e-6)
        say(f"| {k} | {med:.1f} [{lo:.1f}, {hi:.1f}] | {rate / 1e9:.0f} | {rate / ACHIEVABLE[1]:.0%} - {rate / ACHIEVABLE[0]:.0%} |")
    say()
    say(f"A/A spread (op (A) - op, medians): {quant(us['op (A)'])[0] - quant(us['op'])[0]:+.2f} us.  Device time between events around each window, "
        "launch gaps included.")
    say()
    del tl, outs, a, b
    torch.cuda.empty_cache()
    if not args.no_edit:
        from src.pipeline import FastEditor
        ed = FastEditor(model_name=args.model, use_full_controlnet=True, enable_cpu_offload=False)
        big = synth_item_image(5).resize((W, H), Image.BICUBIC)
        noise = np.random.default_rng(0).integers(-12, 13, (H, W, 3))
        big = Image.fromarray((np.asarray(big).astype(int) + noise).clip(0, 255).astype(np.uint8))
        prompt, kw = "a [red] ball on the table", dict(seed=42)
        boxes = tiles.boxes(tw, th, xs, ys)
        jobs = tiles.chunks(n, args.tile_batch)

        def host_form():
            R = []
            for c in jobs:
                R += ed.edit_batch([big.crop(boxes[j]) for j in c], [prompt] * len(c), resolution=(tw, th), **kw)
            return Image.fromarray(tiles.blend_numpy(np.stack([np.asarray(r) for r in R]), xs, ys, H, W))

        def host_form_no_blend():
            for c in jobs:
                ed.edit_batch([big.crop(boxes[j]) for j in c], [prompt] * len(c), resolution=(tw, th), **kw)

        tiled = lambda: ed.edit(big, prompt, tiles="auto", tile_overlap=overlap, tile_batch=args.tile_batch, **kw)
        forms = {"edit(tiles='auto')": tiled, "edit(tiles='auto') (A)": tiled, "edit_batch on crops + blend_numpy": host_form,
                 "edit_batch on crops, no blend": host_form_no_blend}
        got, ref = tiled(), host_form()                  # warm-up: graphs of both job shapes, staging buffers
        tiled()
        ms = {k: [] for k in forms}
        for _ in range(args.edit_rounds):
            for k, f in forms.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                f()
                ms[k].append((time.perf_counter() - t0) * 1e3)
        say(f"## (b) The whole call on a {W} x {H} source: {n} tiles in jobs of {', '.join(str(len(c)) for c in jobs)}")
        say()
        say("| form | wall ms, host in -> host out: median [min, max] |")
        say("|---|---|")
        for k in forms:
            say(f"| {k} | {statistics.median(ms[k]):.1f} [{min(ms[k]):.1f}, {max(ms[k]):.1f}] |")
        m = {k: statistics.median(v) for k, v in ms.items()}
        say()
        t, ta, hb, hn = (m[k] for k in forms)
        say(f"tiled / host form {t / hb:.4f} ({t - hb:+.1f} ms); the host blend alone {hb - hn:+.1f} ms; A/A spread {ta - t:+.1f} ms.")
        say()
        say("## (c) The two results")
        say()
        d = int((np.asarray(got) != np.asarray(ref)).sum())
        say(f"{d} differing bytes of {np.asarray(ref).size} between `edit(tiles='auto')` and the host form.")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
