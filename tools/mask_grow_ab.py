#!/usr/bin/env python3
"""What `mask_grow` costs: one process, one FastEditor (the bench configuration: SSD-1B + full ControlNet, fp16, 1024^2).
The sibling of tools/multiband_ab.py.

    python tools/mask_grow_ab.py [--rounds 20] [--out profiles/mask_grow_ab.md]

1. the op alone: fie_mask_grow_u8 at 1024 x 1024 and 4000 x 3000 for radius +-8 and +-64, on a box mask over 30 % of the image and on a sparse
   random one (density 0.002: no block leaves early, few pixels leave the row pass early), HIP events around `--calls` back-to-back calls,
   median over `--rounds` windows.  Beside it the yardstick: fie_mask_prep with radius 64 at the same size, which stages the same halo;
2. launches per edit: one eager masked edit with and without mask_grow=16 with the library's launch log on (include/fie.h: fie_debug_oplog);
3. time per edit: FastEditor.edit() wall time (host in, host out) of the same masked edit (512^2 source, 1024^2 edit) without the keyword, with
   mask_grow=16 and without it again, interleaved, median over `--rounds` rounds after a warm-up edit of each side.  The two plain series are
   the A/A pair, their ratio the spread of the measurement.  The grow runs in front of the graph, so the graph replay is the same on both sides.
The report is printed and written to `--out` as markdown."""
import argparse
import collections
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SIDES = ("plain", "grow", "plain_again")
SIZES = ((1024, 1024), (3000, 4000))                 # (H, W): the edit size, a 12 MP source
RADII = (8, -8, 64, -64)


def kernels(lines):
    return [l.split("|")[0] for l in lines if not l.startswith("#")]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="ssd-1b", choices=["ssd-1b", "sdxl", "tiny"])
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--calls", type=int, default=20, help="back-to-back calls of the op per timed window")
    ap.add_argument("--grow", type=int, default=16)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mask_grow_ab.md"))
    args = ap.parse_args()
    import numpy as np
    import torch
    from PIL import Image
    import fie_amd  # noqa: F401
    from bench import synth_item_image
    from src.pipeline import FastEditor

    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    ed = FastEditor(model_name=args.model, use_full_controlnet=True, enable_cpu_offload=False)
    pipe, ctx = ed.pipe, ed.pipe.ctx
    med = statistics.median
    st = pipe.slot_stream(0)

    def timed(op):
        """Median and minimum microseconds per call: `calls` calls between two events, `rounds` windows, after three warm-up calls."""
        with torch.cuda.stream(st):
            for _ in range(3):
                op()
            ts = []
            for _ in range(args.rounds):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(args.calls):
                    op()
                e1.record()
                st.synchronize()
                ts.append(e0.elapsed_time(e1) * 1e3 / args.calls)
        return med(ts), min(ts)

    # 1. the op alone
    say(f"# `mask_grow` A/B (`tools/mask_grow_ab.py`)")
    say()
    say(f"{torch.cuda.get_device_name(0)}; model {args.model}; {args.rounds} windows of {args.calls} calls (op), {args.rounds} rounds (edit).")
    say()
    say("## The op alone: `fie_mask_grow_u8`, microseconds per call (median, minimum)")
    say()
    say("| size (H x W) | mask | " + " | ".join(f"r = {r}" for r in RADII) + " | `fie_mask_prep`, radius 64 |")
    say("|---|---|" + "---|" * (len(RADII) + 1))
    for h, w in SIZES:
        box = np.zeros((h, w), np.uint8)
        box[h // 4:h // 4 + int(h * 0.55), w // 4:w // 4 + int(w * 0.55)] = 255           # 0.55^2 = 30 % of the image
        sparse = (np.random.default_rng(h).random((h, w)) < 0.002).astype(np.uint8) * 255
        for name, m in (("box, 30 %", box), ("random, 0.2 %", sparse)):
            mdev = torch.from_numpy(m).to(ctx.device)
            out = torch.empty_like(mdev)
            cells = []
            for r in RADII:
                t, lo = timed(lambda: ctx.mask_grow(mdev, r, out=out))
                cells.append(f"{t:.1f} ({lo:.1f})")
            m_px = torch.empty((h, w), device=ctx.device, dtype=torch.float32)
            m_lat = torch.empty(((h // 8) * (w // 8),), device=ctx.device, dtype=torch.uint8)
            t, lo = timed(lambda: ctx.mask_prep(mdev, 21.3, out=(m_px, m_lat)))                # ceil(3 * 21.3) = 64
            say(f"| {h} x {w} | {name} | " + " | ".join(cells) + f" | {t:.1f} ({lo:.1f}) |")
    say()

    # 2. launches per edit (eager, log on)
    img = synth_item_image(3)
    m = np.zeros((512, 512), np.uint8)
    m[128:384, 128:384] = 255
    mask = Image.fromarray(m)
    kw = dict(prompt="an [empty] table", seed=42, mask=mask)
    side_kw = {"plain": {}, "grow": dict(mask_grow=args.grow), "plain_again": {}}
    pipe.use_graph = False
    counts = {}
    for side in SIDES[:2]:
        ed.edit(img, **side_kw[side], **kw)
        torch.cuda.synchronize()
        ctx.oplog(True)
        ed.edit(img, **side_kw[side], **kw)
        torch.cuda.synchronize()
        counts[side] = kernels(ctx.oplog_read())
        ctx.oplog(False)
    pipe.use_graph = True
    base, c = collections.Counter(counts["plain"]), collections.Counter(counts["grow"])
    say("## A masked edit with and without `mask_grow=%d`" % args.grow)
    say()
    say(f"Launches per edit: plain {len(counts['plain'])}, grown {len(counts['grow'])} (+{len(counts['grow']) - len(counts['plain'])}):")
    say()
    for k in sorted(set(base) | set(c)):
        if base[k] != c[k]:
            say(f"- `{k}`: {base[k]} -> {c[k]}")
    say()

    # 3. time per edit, interleaved
    for side in SIDES[:2]:                              # captures + warm-up
        ed.edit(img, **side_kw[side], **kw)
    wall = {side: [] for side in SIDES}
    for _ in range(args.rounds):
        for side in SIDES:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            ed.edit(img, **side_kw[side], **kw)
            wall[side].append((time.perf_counter() - t0) * 1e3)
    say(f"`FastEditor.edit` wall ms (median of {args.rounds}, interleaved): " + ", ".join(f"{side} {med(wall[side]):.3f}" for side in SIDES) + ".")
    say(f"grow / plain {med(wall['grow']) / med(wall['plain']):.4f} ({med(wall['grow']) - med(wall['plain']):+.3f} ms); "
        f"A/A plain_again / plain {med(wall['plain_again']) / med(wall['plain']):.4f}.")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
