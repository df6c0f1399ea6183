#!/usr/bin/env python3
"""What a soft mask costs: one process, one FastEditor (the bench configuration: SSD-1B + full ControlNet, fp16, 1024^2).
The sibling of tools/mask_grow_ab.py.

    python tools/mask_levels_ab.py [--rounds 20] [--out profiles/mask_levels_ab.md]

1. the ramp op alone: fie_mask_ramp_u8 at 1024 x 1024 and 4000 x 3000 for radius 8, 32 and 64, on a box mask over 30 % of the image and on a
   dense random one (density 0.998: no block leaves early), HIP events around `--calls` back-to-back calls, median over `--rounds` windows.
   Beside it fie_mask_grow_u8 at radius -r (the erosion: it stages the same complement and the same halo) and the ramp once more: the two ramp
   series are the A/A pair, their ratio the spread of the measurement;
2. launches per edit: one eager masked edit and one with mask_ramp, with the library's launch log on (include/fie.h: fie_debug_oplog);
3. time per edit: FastEditor.edit() wall time (host in, host out) of the masked edit (512^2 source and mask, 1024^2 edit) with the binary mask,
   with mask_ramp on the same mask and with the binary mask again, interleaved, median over `--rounds` rounds after a warm-up edit of each side;
4. the graph replay alone: the binary masked job, the levels job of the same mask and the binary job again, HIP events around each replay,
   interleaved.  Inside the job a levels edit launches what a masked edit launches, fie_lcm_step_levels in place of fie_lcm_step_masked.
The report is printed and written to `--out` as markdown."""
import argparse
import collections
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SIDES = ("binary", "levels", "binary_again")
SIZES = ((1024, 1024), (3000, 4000))                 # (H, W): the edit size, a 12 MP source
RADII = (8, 32, 64)


def kernels(lines):
    return [l.split("|")[0] for l in lines if not l.startswith("#")]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="ssd-1b", choices=["ssd-1b", "sdxl", "tiny"])
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--calls", type=int, default=20, help="back-to-back calls of the op per timed window")
    ap.add_argument("--ramp", type=int, default=32)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mask_levels_ab.md"))
    args = ap.parse_args()
    import numpy as np
    import torch
    from PIL import Image
    import fie_amd  # noqa: F401
    from fie_amd.mask import MaskSpec
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
    say("# Soft masks A/B (`tools/mask_levels_ab.py`)")
    say()
    say(f"{torch.cuda.get_device_name(0)}; model {args.model}; {args.rounds} windows of {args.calls} calls (op), {args.rounds} rounds (edit).")
    say()
    say("## The ramp op alone: microseconds per call, median (minimum)")
    say()
    say("| size (H x W) | mask | r | `fie_mask_ramp_u8` | `fie_mask_grow_u8`, radius -r | ramp again | ramp / grow | A/A ramp again / ramp |")
    say("|---|---|---|---|---|---|---|---|")
    for h, w in SIZES:
        box = np.zeros((h, w), np.uint8)
        box[h // 4:h // 4 + int(h * 0.55), w // 4:w // 4 + int(w * 0.55)] = 255           # 0.55^2 = 30 % of the image
        dense = (np.random.default_rng(h).random((h, w)) < 0.998).astype(np.uint8) * 255
        for name, m in (("box, 30 %", box), ("random, 99.8 %", dense)):
            mdev = torch.from_numpy(m).to(ctx.device)
            out = torch.empty_like(mdev)
            for r in RADII:
                a, alo = timed(lambda: ctx.mask_ramp(mdev, r, out=out))
                g, glo = timed(lambda: ctx.mask_grow(mdev, -r, out=out))
                b, blo = timed(lambda: ctx.mask_ramp(mdev, r, out=out))
                say(f"| {h} x {w} | {name} | {r} | {a:.1f} ({alo:.1f}) | {g:.1f} ({glo:.1f}) | {b:.1f} ({blo:.1f}) | {a / g:.3f} | {b / a:.3f} |")
    say()

    # 2. launches per edit (eager, log on)
    img = synth_item_image(3)
    m = np.zeros((512, 512), np.uint8)
    m[128:384, 128:384] = 255
    mask = Image.fromarray(m)
    kw = dict(prompt="a [red] ball on the table", seed=42, mask=mask)
    side_kw = {"binary": {}, "levels": dict(mask_ramp=args.ramp), "binary_again": {}}
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
    base, c = collections.Counter(counts["binary"]), collections.Counter(counts["levels"])
    say("## A masked edit with the binary mask and with `mask_ramp=%d` (512^2 mask, 1024^2 edit)" % args.ramp)
    say()
    say(f"Launches per edit: binary {len(counts['binary'])}, levels {len(counts['levels'])} (+{len(counts['levels']) - len(counts['binary'])}):")
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
    say(f"levels / binary {med(wall['levels']) / med(wall['binary']):.4f} ({med(wall['levels']) - med(wall['binary']):+.3f} ms); "
        f"A/A binary_again / binary {med(wall['binary_again']) / med(wall['binary']):.4f}.")
    say()

    # 4. the graph replay alone, interleaved
    with torch.cuda.stream(st):
        src = ctx.resize_lanczos(torch.from_numpy(np.array(img)).to(ctx.device), 1024, 1024)
        ctl = ctx.canny_device(src)
        mdev = {"binary": ed._mask_device(m, (1024, 1024)), "levels": ed._mask_device(m, (1024, 1024), MaskSpec(ramp=args.ramp))}
        gen = lambda: torch.Generator("cpu").manual_seed(42)
        jobs = {"binary": pipe.prepare(kw["prompt"], "", src, ctl, 0.8, 4, 1.5, 0.5, gen(), mdev["binary"], 0, True),
                "levels": pipe.prepare(kw["prompt"], "", src, ctl, 0.8, 4, 1.5, 0.5, gen(), mdev["levels"], 0, True, mask_mode="levels")}
        jobs["binary_again"] = jobs["binary"]
        replay = {side: [] for side in SIDES}
        for side in SIDES[:2]:
            pipe.run_device_graphed(jobs[side])
        st.synchronize()
        for _ in range(args.rounds):
            for side in SIDES:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                pipe.run_device_graphed(jobs[side])
                e1.record()
                st.synchronize()
                replay[side].append(e0.elapsed_time(e1))
    say(f"Graph replay device ms (median of {args.rounds}, interleaved): " + ", ".join(f"{side} {med(replay[side]):.3f}" for side in SIDES) + ".")
    say(f"levels / binary {med(replay['levels']) / med(replay['binary']):.4f} ({med(replay['levels']) - med(replay['binary']):+.3f} ms); "
        f"A/A binary_again / binary {med(replay['binary_again']) / med(replay['binary']):.4f}.")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
