#!/usr/bin/env python3
"""What an edge-budget Canny costs: one process, one FastEditor (the bench configuration: SSD-1B + full ControlNet, fp16,
1024^2).  The sibling of tools/mask_levels_ab.py.

    python tools/canny_auto_ab.py [--rounds 20] [--density 0.002] [--out profiles/canny_auto_ab.md]

The two arms hand the Canny the same thresholds: the fixed arm is `edit(..., canny_low_threshold=low, canny_high_threshold=high)` with the pair
the auto arm's `set_canny_density(d)` picks on that image, so both draw the same edge map, replay the same graph on the same bytes and differ in the
Canny stage alone -- the NMS kernel against ridge + histogram, select and classify.
1. the Canny stage alone at 1024 x 1024 and 3000 x 4000: `canny_begin` (all kernels of the first half, 4 rounds of hysteresis, no wait) with the
   fixed pair, with the budget and with the fixed pair again, HIP events around `--calls` back-to-back calls, median over `--rounds` windows; the
   two fixed series are the A/A pair.  Beside it the thresholds alone (`fie_canny_thresholds_device_u8`: ridge + select, without the read-back);
2. launches per edit: one eager edit of each arm with the library's launch log on (include/fie.h: fie_debug_oplog);
3. time per edit: FastEditor.edit() wall time (host in, host out) of fixed, auto and fixed again, interleaved, median over `--rounds` rounds after
   a warm-up edit of each side.
The report is printed and written to `--out` as markdown."""
import argparse
import collections
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SIDES = ("fixed", "auto", "fixed_again")
SIZES = ((1024, 1024), (3000, 4000))                 # (H, W): the edit size, a 12 MP source (what a tiled edit takes its pair from)
LAUNCH_US = 6.0                                      # per launch, DESIGN.md section 7


def kernels(lines):
    return [l.split("|")[0] for l in lines if not l.startswith("#")]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="ssd-1b", choices=["ssd-1b", "sdxl", "tiny"])
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--calls", type=int, default=20, help="back-to-back calls of the stage per timed window")
    ap.add_argument("--density", type=float, default=0.002, help="0.002 picks 99 / 198 on the bench image at 1024^2: the fixed arm is Canny(100, 200) but for a unit")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "canny_auto_ab.md"))
    args = ap.parse_args()
    import numpy as np
    import torch
    import fie_amd  # noqa: F401
    from fie_amd import canny_auto as hcanny, hip
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

    # 1. the stage alone
    say("# Edge-budget Canny A/B (`tools/canny_auto_ab.py`)")
    say()
    say(f"{torch.cuda.get_device_name(0)}; model {args.model}; density {args.density:g}; {args.rounds} windows of {args.calls} calls (stage), "
        f"{args.rounds} rounds (edit).")
    say()
    say("## The Canny stage alone (`canny_begin`, 4 rounds of hysteresis, no wait): microseconds per call, median (minimum)")
    say()
    say("| size (H x W) | pair picked | fixed pair | budget | fixed pair again | budget - fixed | A/A fixed again / fixed | thresholds alone |")
    say("|---|---|---|---|---|---|---|---|")
    img = synth_item_image(3)
    for h, w in SIZES:
        with torch.cuda.stream(st):
            src = ctx.resize_lanczos(torch.from_numpy(np.array(img)).to(ctx.device), h, w)
            seeds = hcanny.budget(h * w, args.density)
            low, high = ctx.canny_thresholds(src, seeds)
            ws = torch.empty(hip.lib().fie_canny_auto_workspace_bytes(h, w), device=ctx.device, dtype=torch.uint8)
            out = torch.empty((h, w, 3), device=ctx.device, dtype=torch.uint8)
            pair = torch.empty(2, device=ctx.device, dtype=torch.int32)
        a, alo = timed(lambda: ctx.canny_begin(src, low, high, rounds=4, out=out))
        b, blo = timed(lambda: ctx.canny_begin(src, 100, 200, rounds=4, budget=seeds, out=out, workspace=ws))
        c, clo = timed(lambda: ctx.canny_begin(src, low, high, rounds=4, out=out))
        t, tlo = timed(lambda: hip._chk(hip.lib().fie_canny_thresholds_device_u8(ctx.h, hip._p(src), h, w, seeds, 100, 200, hip._p(ws), hip._p(pair))))
        say(f"| {h} x {w} | {low} / {high} | {a:.1f} ({alo:.1f}) | {b:.1f} ({blo:.1f}) | {c:.1f} ({clo:.1f}) | {b - a:+.1f} | {c / a:.3f} | {t:.1f} ({tlo:.1f}) |")
    say()

    # 2. launches per edit (eager, log on)
    low, high = ed.canny_thresholds(img, args.density)
    kw = dict(prompt="a [red] ball on the table", seed=42)
    side_kw = {"fixed": dict(canny_low_threshold=low, canny_high_threshold=high), "auto": {}}
    side_kw["fixed_again"] = side_kw["fixed"]

    def edit(side):
        ed.set_canny_density(args.density if side == "auto" else None)
        return ed.edit(img, **side_kw[side], **kw)
    pipe.use_graph = False
    counts, outs = {}, {}
    for side in SIDES[:2]:
        edit(side)
        torch.cuda.synchronize()
        ctx.oplog(True)
        outs[side] = np.asarray(edit(side))
        torch.cuda.synchronize()
        counts[side] = kernels(ctx.oplog_read())
        ctx.oplog(False)
    pipe.use_graph = True
    base, c = collections.Counter(counts["fixed"]), collections.Counter(counts["auto"])
    more = len(counts["auto"]) - len(counts["fixed"])
    say(f"## An edit at 1024^2 with the pair {low} / {high} given and with `set_canny_density({args.density:g})` picking it")
    say()
    say(f"The two outputs are {'byte-identical' if np.array_equal(outs['fixed'], outs['auto']) else 'DIFFERENT'}.")
    say(f"Launches per edit: fixed {len(counts['fixed'])}, auto {len(counts['auto'])} ({more:+d}):")
    say()
    for k in sorted(set(base) | set(c)):
        if base[k] != c[k]:
            say(f"- `{k}`: {base[k]} -> {c[k]}")
    say()

    # 3. time per edit, interleaved
    for side in SIDES[:2]:                              # captures + warm-up
        edit(side)
    wall = {side: [] for side in SIDES}
    for _ in range(args.rounds):
        for side in SIDES:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            edit(side)
            wall[side].append((time.perf_counter() - t0) * 1e3)
    diff = med(wall["auto"]) - med(wall["fixed"])
    spread = abs(med(wall["fixed_again"]) - med(wall["fixed"]))
    say(f"`FastEditor.edit` wall ms (median of {args.rounds}, interleaved): " + ", ".join(f"{side} {med(wall[side]):.3f}" for side in SIDES) + ".")
    say(f"auto / fixed {med(wall['auto']) / med(wall['fixed']):.4f} ({diff:+.3f} ms); A/A fixed_again / fixed "
        f"{med(wall['fixed_again']) / med(wall['fixed']):.4f} ({med(wall['fixed_again']) - med(wall['fixed']):+.3f} ms).")
    bound = spread + more * LAUNCH_US * 1e-3
    say(f"Acceptance (the difference within the A/A spread plus {more} launches at {LAUNCH_US:g} us): {diff:+.3f} ms against {bound:.3f} ms: "
        f"{'inside' if diff <= bound else 'OUTSIDE'}.")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
