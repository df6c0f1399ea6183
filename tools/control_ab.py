#!/usr/bin/env python3
"""What control weights cost and save: one FastEditor in the bench configuration (SSD-1B + full ControlNet, fp16, 1024^2,
nominal 4 steps at strength 0.5, CFG).  The sibling of tools/emphasis_ab.py.

    python tools/control_ab.py [--rounds 20] [--parent DIR] [--out profiles/control_weights_ab.md]

Arms, one edit each per round, interleaved in one process after a warm-up edit (and graph capture) of every arm:
    none, none_again   the setting None, twice: the A/A pair whose spread every other figure is read against
    prompt             layers="prompt": the same kernels with other scales
    steps              steps=(0, 0.5): the second of the two loop steps runs no ControlNet
    in_mask            in_mask=0 with a centred 512^2 mask, against `masked`: the same mask under the setting None
1. launches per edit: one eager edit of each arm with the library's launch log on (include/fie.h: fie_debug_oplog), and the kernels whose count changes;
2. the two ops alone at the bench size: HIP events around back-to-back calls;
3. time per edit: FastEditor.edit() wall time (host in, host out), median over `--rounds` rounds, every arm against `none` (or `masked`) and the A/A pair;
4. with `--parent DIR` (a built checkout of the parent commit): a child process runs `none` in that tree and takes its turn in every round, timed
   the same way, so that this commit's None and the parent's are measured in one call, alternating.
The report is printed and written to `--out` as markdown."""
import argparse
import collections
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PROMPT = "a red ball on the wooden table"
ARMS = ("none", "prompt", "steps", "masked", "in_mask", "none_again")
SETTINGS = {"none": {}, "none_again": {}, "masked": {}, "prompt": dict(layers="prompt"), "steps": dict(steps=(0, 0.5)), "in_mask": dict(in_mask=0.0)}

CHILD = r"""
import sys, time
sys.path.insert(0, sys.argv[1])
import torch
import fie_amd  # noqa: F401
from bench import synth_item_image
from src.pipeline import FastEditor
ed = FastEditor(model_name=sys.argv[2], use_full_controlnet=True, enable_cpu_offload=False)
img = synth_item_image(3)
for _ in range(3):
    ed.edit(img, sys.argv[3], seed=42, strength=0.5)
print("ready", flush=True)
for line in sys.stdin:
    if line.strip() != "go":
        break
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    ed.edit(img, sys.argv[3], seed=42, strength=0.5)
    print((time.perf_counter() - t0) * 1e3, flush=True)
"""


def kernels(lines):
    return [l.split("|")[0] for l in lines if not l.startswith("#")]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="ssd-1b", choices=["ssd-1b", "sdxl", "tiny"])
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--calls", type=int, default=20, help="back-to-back calls of an op per timed window")
    ap.add_argument("--parent", default=None, help="a built checkout of the parent commit: its None edit joins every round from a child process")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "control_weights_ab.md"))
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
    img = synth_item_image(3)
    sw, sh = img.size                                    # the mask has the source's size; at the 1024^2 edit its hole is the centred 512^2
    ms = np.zeros((sh, sw), np.uint8)
    ms[sh // 4:sh - sh // 4, sw // 4:sw - sw // 4] = 255
    mask = Image.fromarray(ms)
    m = np.zeros((1024, 1024), np.uint8)
    m[256:768, 256:768] = 255

    def edit(arm):
        ed.set_control_weights(**SETTINGS[arm])
        return ed.edit(img, PROMPT, seed=42, strength=0.5, mask=mask if arm in ("masked", "in_mask") else None)

    say("# Control weights A/B (`tools/control_ab.py`)")
    say()
    say(f"{torch.cuda.get_device_name(0)}; model {args.model} + full ControlNet, fp16, 1024^2, 4 nominal steps at strength 0.5 (2 loop steps), CFG; "
        f"{args.rounds} rounds.")
    say()

    # 1. launches per edit (eager, log on)
    pipe.use_graph = False
    counts, outs = {}, {}
    for arm in ARMS[:-1]:
        edit(arm)
        torch.cuda.synchronize()
        ctx.oplog(True)
        outs[arm] = np.asarray(edit(arm))
        torch.cuda.synchronize()
        counts[arm] = kernels(ctx.oplog_read())
        ctx.oplog(False)
    pipe.use_graph = True
    say("## Launches of the library per edit (eager, counted from its launch log)")
    say()
    say("| arm | launches | against | difference | bytes of the output that differ (largest difference) |")
    say("|---|---|---|---|---|")
    for arm in ARMS[:-1]:
        ref = "masked" if arm == "in_mask" else "none"
        d = np.abs(outs[arm].astype(int) - outs[ref].astype(int))
        say(f"| {arm} | {len(counts[arm])} | {ref} | {len(counts[arm]) - len(counts[ref]):+d} | {int((d > 0).sum())} of {d.size} ({int(d.max())}) |")
    say()
    for arm in ("prompt", "steps", "in_mask"):
        ref = "masked" if arm == "in_mask" else "none"
        base, c = collections.Counter(counts[ref]), collections.Counter(counts[arm])
        changed = [f"`{k.split('(')[0][:60]}` {base[k]} -> {c[k]}" for k in sorted(set(base) | set(c)) if base[k] != c[k]]
        say(f"- {arm} against {ref}: {len(changed)} kernels change their count" + (": " + "; ".join(changed[:12]) + (" ..." if len(changed) > 12 else "") if changed else ""))
    say()

    # 2. the two ops alone
    st = pipe.slot_stream(0)

    def timed(op):
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

    from fie_amd import control
    with torch.cuda.stream(st):
        m_dev = torch.from_numpy(m).to(ctx.device)
        w = ctx.control_pyramid(m_dev, 0, True)[None].contiguous()
        dims = control.level_dims(1024, 1024)
        offs = [0, dims[0][0] * dims[0][1], dims[0][0] * dims[0][1] + dims[1][0] * dims[1][1]]
        segs, nbytes = [], 0
        for lvl, c in zip([0, 0, 0, 1, 1, 1, 2, 2, 2, 2], [320, 320, 320, 320, 640, 640, 640, 1280, 1280, 1280]):
            h, ww = dims[lvl]
            u = torch.randn(2, h, ww, c, device=ctx.device, dtype=torch.float16)
            segs.append((u, torch.randn_like(u), h * ww, offs[lvl], 0.5))
            nbytes += 3 * u.numel() * 2
    t, lo = timed(lambda: ctx.control_pyramid(m_dev, 0, True))
    say("## The ops alone: microseconds per call, median (minimum) of back-to-back calls on a stream (the launch gap included)")
    say()
    say(f"- `fie_control_pyramid_u8` on a 1024^2 mask, three levels: {t:.1f} ({lo:.1f}) us")
    with torch.cuda.stream(st):
        outs = [torch.empty_like(s[0]) for s in segs]    # written again by every call: the timed calls allocate nothing
    t, lo = timed(lambda: ctx.control_add(segs, w, 2, outs=outs))
    say(f"- `fie_control_add` on ten residuals of SDXL's shapes at 1024^2, CFG batch 2, the centred 512^2 hole at weight 0: {t:.1f} ({lo:.1f}) us for "
        f"{nbytes / 1e6:.0f} MB of u, t and out ({nbytes / t * 1e-3:.0f} GB/s if every t were read; inside the hole, a quarter of the positions, t is not)")
    with torch.cuda.stream(st):
        ones = torch.ones_like(w)
    t, lo = timed(lambda: ctx.control_add(segs, ones, 2, outs=outs))
    say(f"- the same under weights of all ones (every t read): {t:.1f} ({lo:.1f}) us, {nbytes / t * 1e-3:.0f} GB/s")
    say()
    del outs
    del segs

    # 3. time per edit, interleaved; 4. the parent's None from a child process
    child = None
    if args.parent:
        child = subprocess.Popen([sys.executable, "-c", CHILD, os.path.abspath(args.parent), args.model, PROMPT], stdin=subprocess.PIPE, stdout=subprocess.PIPE,
                                 text=True, cwd=os.path.abspath(args.parent))
        while True:
            line = child.stdout.readline()
            if not line:
                raise RuntimeError("the parent's process ended before it was ready")
            if line.strip() == "ready":
                break
    for arm in ARMS:
        edit(arm)
        edit(arm)
    wall = {arm: [] for arm in ARMS + (("parent",) if child else ())}
    for _ in range(args.rounds):
        for arm in ARMS:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            edit(arm)
            wall[arm].append((time.perf_counter() - t0) * 1e3)
        if child:
            torch.cuda.synchronize()
            child.stdin.write("go\n")
            child.stdin.flush()
            wall["parent"].append(float(child.stdout.readline()))
    if child:
        child.stdin.write("end\n")
        child.stdin.flush()
        child.wait(timeout=60)
    ed.set_control_weights()
    say(f"## `FastEditor.edit` wall ms (host in, host out; median of {args.rounds} rounds, the arms interleaved)")
    say()
    say("| arm | median | min | against | difference of the medians |")
    say("|---|---|---|---|---|")
    for arm in wall:
        ref = "masked" if arm == "in_mask" else "none"
        say(f"| {arm} | {med(wall[arm]):.3f} | {min(wall[arm]):.3f} | {ref} | {med(wall[arm]) - med(wall[ref]):+.3f} |")
    say()
    say(f"A/A spread: none_again - none = {med(wall['none_again']) - med(wall['none']):+.3f} ms of {med(wall['none']):.3f}.")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
