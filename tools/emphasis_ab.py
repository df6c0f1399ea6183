#!/usr/bin/env python3
"""What prompt emphasis costs: one process, one FastEditor (the bench configuration: SSD-1B + full ControlNet, fp16, 1024^2).
The sibling of tools/canny_auto_ab.py.

    python tools/emphasis_ab.py [--rounds 20] [--weight 1.5] [--out profiles/emphasis_ab.md]

Both arms run under `set_prompt_emphasis(w)`: the plain arm's prompt has no marks (no weight differs from 1: the un-emphasised job and graph), the
weighted arm's prompt is the same words with two marks.  Both tokenise to the same ids, so the arms differ in the weights alone.
1. the op alone at SDXL's width: `fie_kv_emphasis` on f16 [154, 166 400] (the UNet's grouped K | V result: 10 blocks of 640, 60 of 1280) with 3 and
   with 10 weighted rows and with none, HIP events around `--calls` back-to-back calls, median and minimum over `--rounds` windows;
2. launches per edit: one eager edit of each arm with the library's launch log on (include/fie.h: fie_debug_oplog);
3. the host side: `pipe.prepare()` of each arm (tokenisation, parsing, the one packed upload) and whether the weights share that upload;
4. time per edit: FastEditor.edit() wall time (host in, host out) of plain, weighted and plain again, interleaved, median over `--rounds` rounds
   after a warm-up edit of each side; the two plain series are the A/A pair.
The report is printed and written to `--out` as markdown."""
import argparse
import collections
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SIDES = ("plain", "weighted", "plain_again")
PROMPTS = {"plain": "a red ball on the wooden table", "weighted": "a [red] ball on the [wooden table]"}
PROMPTS["plain_again"] = PROMPTS["plain"]
LAUNCH_US = 6.0                                      # per launch, DESIGN.md section 7


def kernels(lines):
    return [l.split("|")[0] for l in lines if not l.startswith("#")]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="ssd-1b", choices=["ssd-1b", "sdxl", "tiny"])
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--calls", type=int, default=20, help="back-to-back calls of the op per timed window")
    ap.add_argument("--weight", type=float, default=1.5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "emphasis_ab.md"))
    args = ap.parse_args()
    import numpy as np
    import torch
    import fie_amd  # noqa: F401
    from fie_amd import emphasis
    from bench import synth_item_image
    from src.pipeline import FastEditor

    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    ed = FastEditor(model_name=args.model, use_full_controlnet=True, enable_cpu_offload=False, prompt_emphasis=args.weight)
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
    say("# Prompt emphasis A/B (`tools/emphasis_ab.py`)")
    say()
    say(f"{torch.cuda.get_device_name(0)}; model {args.model}; weight {args.weight:g}; {args.rounds} windows of {args.calls} calls (op), "
        f"{args.rounds} rounds (edit).")
    say()
    say("## `fie_kv_emphasis` alone on f16 [154, 166 400] (SDXL's grouped K | V): microseconds per call, median (minimum)")
    say()
    say("| weighted rows | us per call | V bytes read + written | GB/s at the median |")
    say("|---|---|---|---|")
    rows, cs = 154, [640] * 10 + [1280] * 60
    with torch.cuda.stream(st):
        x = torch.randn(rows, 2 * sum(cs), device=ctx.device, dtype=torch.float16)
        flags = torch.from_numpy(emphasis.v_flags(cs)).to(ctx.device)
    for picked in ((), (79, 80, 153), tuple(range(78, 88))):
        w = torch.ones(rows, dtype=torch.float32)
        w[list(picked)] = 1.0 if not picked else 0.999                # close to 1: the timed calls repeat on the same buffer and must not overflow it
        with torch.cuda.stream(st):
            w = w.to(ctx.device)
        t, lo = timed(lambda: ctx.kv_emphasis(x, w, flags))
        nbytes = 2 * len(picked) * sum(cs) * 2
        say(f"| {len(picked)} | {t:.1f} ({lo:.1f}) | {nbytes} | {nbytes / t * 1e-3 if nbytes else 0:.0f} |")
    say()
    say("The calls of a window run back to back on a stream, so a figure holds the launch gap; an all-ones call is what the skipped rows cost.")
    say()
    del x

    # 2. launches per edit (eager, log on)
    img = synth_item_image(3)
    kw = dict(seed=42)

    def edit(side):
        return ed.edit(img, PROMPTS[side], **kw)
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
    base, c = collections.Counter(counts["plain"]), collections.Counter(counts["weighted"])
    more = len(counts["weighted"]) - len(counts["plain"])
    d = np.abs(outs["plain"].astype(int) - outs["weighted"].astype(int))
    say(f"## An edit at 1024^2: `{PROMPTS['plain']}` against `{PROMPTS['weighted']}` under `set_prompt_emphasis({args.weight:g})`")
    say()
    say(f"Synthetic weights: the two outputs differ in {int((d > 0).sum())} of {d.size} bytes, by at most {int(d.max())}.")
    say(f"Launches of the library per edit (eager, counted from its launch log): plain {len(counts['plain'])}, weighted {len(counts['weighted'])} ({more:+d}):")
    say()
    for k in sorted(set(base) | set(c)):
        if base[k] != c[k]:
            say(f"- `{k}`: {base[k]} -> {c[k]}")
    say()

    # 3. the host side
    ctl = ed.preprocess_image(img.resize((1024, 1024)))
    host = {}
    for side in SIDES[:2]:
        ts = []
        for _ in range(args.rounds + 3):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            job = pipe.prepare(PROMPTS[side], "", img.resize((1024, 1024)), ctl, generator=torch.Generator("cpu").manual_seed(1))
            ts.append((time.perf_counter() - t0) * 1e3)
        host[side] = med(ts[3:])
        if side == "weighted":
            one = job["emph"].untyped_storage().data_ptr() == job["ids_l"].untyped_storage().data_ptr()
            say(f"The weights of the job are a view of the packed prompt upload (one storage with the ids): {one}.  No copy, no synchronisation and "
                f"no read-back is added; the graph replay copies {job['emph'].numel() * 4} more bytes device to device.")
    say(f"`pipe.prepare` host ms (median of {args.rounds}): plain {host['plain']:.3f}, weighted {host['weighted']:.3f} "
        f"({host['weighted'] - host['plain']:+.3f}).")
    say()

    # 4. time per edit, interleaved
    for side in SIDES[:2]:                              # captures + warm-up
        edit(side)
    wall = {side: [] for side in SIDES}
    for _ in range(args.rounds):
        for side in SIDES:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            edit(side)
            wall[side].append((time.perf_counter() - t0) * 1e3)
    diff = med(wall["weighted"]) - med(wall["plain"])
    say(f"`FastEditor.edit` wall ms (median of {args.rounds}, interleaved): " + ", ".join(f"{side} {med(wall[side]):.3f}" for side in SIDES) + ".")
    say(f"weighted / plain {med(wall['weighted']) / med(wall['plain']):.4f} ({diff:+.3f} ms); A/A plain_again / plain "
        f"{med(wall['plain_again']) / med(wall['plain']):.4f} ({med(wall['plain_again']) - med(wall['plain']):+.3f} ms).")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
