#!/usr/bin/env python3
"""What LPIPS on the device costs: one process, seeded SqueezeNet weights (tests/lpips_oracle.py), profiler off.

    python tools/lpips_cost.py [--rounds 15] [--out profiles/lpips_device.md]

1. `MetricsCalculator.calculate_lpipses` for 8 pairs of 512x512 images in one call against the same pairs one call each, and one pair alone:
   host timer around the call (uploads and its one synchronisation included), alternating rounds, medians after 3 warm-up rounds;
2. launches of one pass of the tower (16 images) with the library's launch log on (include/fie.h: fie_debug_oplog), by kernel, and the peak of
   torch's allocator over that pass above what was allocated before it (the transient memory);
3. the tower's passes by size: 2 / 4 / 8 / 16 images, HIP events around `--calls` back-to-back scorer calls;
4. `FastEditor("tiny").edit(metrics=True)` with `lpips_dir` against an editor without it in the same process, alternating rounds, medians; the two
   series of the plain editor (before / after the other in each round) are the A/A pair, their ratio the spread of the measurement.
The report is printed and written to `--out` as markdown."""
import argparse
import collections
import os
import re
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--calls", type=int, default=5, help="back-to-back scorer calls per timed window")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lpips_device.md"))
    args = ap.parse_args()
    import numpy as np
    import torch
    from PIL import Image
    import fie_amd  # noqa: F401
    import lpips_oracle as lo
    from bench import synth_item_image
    from src.metrics import MetricsCalculator
    from src.pipeline import FastEditor

    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    med = statistics.median
    wdir = lo.write_dir(tempfile.mkdtemp(prefix="lpips_w"), "safetensors")
    calc = MetricsCalculator("cuda", lpips_dir=wdir)
    ctx, sc = calc._ctx, calc._lpips
    rng = np.random.default_rng(0)
    srcs = [synth_item_image(i) for i in range(8)]
    edts = [Image.fromarray(np.clip(np.asarray(im).astype(np.int16) + rng.integers(-20, 21, (512, 512, 3)), 0, 255).astype(np.uint8)) for im in srcs]

    def wall(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3

    say("# LPIPS on the device: measured cost\n")
    say(f"One MI355X, seeded SqueezeNet 1.1 weights (tests/lpips_oracle.py) loaded through `fie_amd.lpips.load`; fp32 in every context.  Medians of "
        f"{args.rounds} alternating rounds after 3 warm-up rounds, profiler off.  Definition, kernels and accuracy: DESIGN.md section 19.\n")
    sides = {"8 pairs, one `calculate_lpipses` call (one pass of 16 images)": lambda: calc.calculate_lpipses(srcs, edts),
             "the same 8 pairs, one `calculate_lpips` call each": lambda: [calc.calculate_lpips(a, b) for a, b in zip(srcs, edts)],
             "one pair": lambda: calc.calculate_lpips(srcs[0], edts[0])}
    times = collections.defaultdict(list)
    for r in range(args.rounds + 3):
        for name, fn in sides.items():
            t = wall(fn)
            if r >= 3:
                times[name].append(t)
    say("| `MetricsCalculator` on 512x512 PIL images (uploads and the one synchronisation included) | time |\n|---|---|")
    for name in sides:
        say(f"| {name} | {med(times[name]):.2f} ms (min {min(times[name]):.2f}, max {max(times[name]):.2f}) |")

    dev = lambda im: torch.from_numpy(np.array(im)).to(ctx.device)
    a, b = [dev(im) for im in srcs], [dev(im) for im in edts]
    sc.scores(a, b)
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    ctx.oplog(True)
    sc.scores(a, b)
    torch.cuda.synchronize()
    def short(name):                        # the kernel's own name out of the (mangled) symbol, with its integer template argument
        m = re.search(r"([a-z][a-z0-9_]*_kernel)(?:ILi(\d+)E|<(\d+)>)?", name)
        return name if m is None else m.group(1) + (f"<{m.group(2) or m.group(3)}>" if m.group(2) or m.group(3) else "")
    log = [short(l.split("|")[0]) for l in ctx.oplog_read() if not l.startswith("#")]
    ctx.oplog(False)
    peak = torch.cuda.max_memory_allocated() - base
    say(f"\nOne pass of 16 images (8 pairs, no mask): {len(log)} launches; peak transient memory {peak / 2 ** 20:.0f} MiB above the "
        f"{base / 2 ** 20:.0f} MiB allocated before the pass.\n")
    say("| kernel | launches |\n|---|---|")
    for k, n in collections.Counter(log).most_common():
        say(f"| `{k}` | {n} |")

    say("\n| `LpipsScorer.scores` on device tensors, HIP events | per call | per pair |\n|---|---|---|")
    for n in (1, 2, 4, 8):
        ws = []
        for r in range(args.rounds + 3):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(args.calls):
                sc.scores(a[:n], b[:n])
            e1.record()
            torch.cuda.synchronize()
            if r >= 3:
                ws.append(e0.elapsed_time(e1) / args.calls)
        say(f"| {n} pair(s): one pass of {2 * n} images | {med(ws):.3f} ms | {med(ws) / n:.3f} ms |")

    plain, with_dir = FastEditor(model_name="tiny", enable_cpu_offload=False), FastEditor(model_name="tiny", enable_cpu_offload=False, lpips_dir=wdir)
    img = srcs[0]
    series = collections.defaultdict(list)
    order = (("plain", plain), ("lpips", with_dir), ("plain_again", plain))
    for r in range(args.rounds + 3):
        for name, ed in order:
            t = wall(lambda: ed.edit(img, "a red kite", seed=42, metrics=True))
            if r >= 3:
                series[name].append(t)
    m = {k: med(v) for k, v in series.items()}
    say(f"\n`edit(metrics=True)` at the tiny preset, 512x512 source, 1024x1024 edit, {args.rounds} alternating rounds of (editor without `lpips_dir`, editor "
        "with it, the first again) in ONE process, medians:\n")
    say("| without | with `lpips_dir` | without, again | difference | A/A spread |\n|---|---|---|---|---|")
    say(f"| {m['plain']:.2f} ms | {m['lpips']:.2f} ms | {m['plain_again']:.2f} ms | {m['lpips'] - (m['plain'] + m['plain_again']) / 2:+.2f} ms per edit | "
        f"{abs(m['plain'] - m['plain_again']):.2f} ms |")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
