#!/usr/bin/env python3
"""What a masked-content mode costs: one process, one FastEditor (the bench configuration: SSD-1B + full ControlNet, fp16,
1024^2), the same 512^2 image edited with a 512^2-pixel mask at the edit size under masked_content="original" and under each new mode,
interleaved, graph-replayed.  The sibling of tools/masked_edit_ab.py, whose "masked" side is this tool's "original".

    python tools/masked_content_ab.py [--rounds 20] [--mask_blur 0]

1. launches per edit: one eager edit of each mode with the library's launch log on (include/fie.h: fie_debug_oplog), kernel launches counted
   ('#' stage marks excluded) and the launches each mode adds to "original" listed by kernel;
2. time per edit: FastEditor.edit() wall time (host in, host out), and the device time of the graph replay alone (HIP events around the replay
   of a prepared job), median over `rounds` rounds after one warm-up edit of each mode; every round runs the four modes in turn."""
import argparse
import collections
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

MODES = ("original", "fill", "latent_noise", "latent_nothing")


def kernels(lines):
    return [l.split("|")[0] for l in lines if not l.startswith("#")]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="ssd-1b", choices=["ssd-1b", "sdxl", "tiny"])
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--mask_blur", type=float, default=0.0)
    args = ap.parse_args()
    import numpy as np
    import torch
    from PIL import Image
    import fie_amd  # noqa: F401
    from bench import synth_item_image
    from src.pipeline import FastEditor

    ed = FastEditor(model_name=args.model, use_full_controlnet=True, enable_cpu_offload=False)
    pipe, ctx = ed.pipe, ed.pipe.ctx
    img = synth_item_image(3)
    m = np.zeros((512, 512), np.uint8)
    m[128:384, 128:384] = 255                          # 256^2 of the 512^2 source: 512^2 pixels at the 1024^2 edit size
    mask = Image.fromarray(m)
    kw = dict(prompt="an [empty] table", seed=42, mask=mask, mask_blur=args.mask_blur)

    # 1. launches per edit (eager, log on)
    pipe.use_graph = False
    counts = {}
    for mode in MODES:
        ed.edit(img, masked_content=mode, **kw)
        torch.cuda.synchronize()
        ctx.oplog(True)
        ed.edit(img, masked_content=mode, **kw)
        torch.cuda.synchronize()
        counts[mode] = kernels(ctx.oplog_read())
        ctx.oplog(False)
    pipe.use_graph = True
    base = collections.Counter(counts["original"])
    for mode in MODES[1:]:
        c = collections.Counter(counts[mode])
        print(f"launches per edit: original {len(counts['original'])}, {mode} {len(counts[mode])} (+{len(counts[mode]) - len(counts['original'])})")
        for k in sorted(set(base) | set(c)):
            if base[k] != c[k]:
                print(f"  {k}: {base[k]} -> {c[k]}")

    # 2. time per edit, interleaved
    for mode in MODES:                                  # captures + warm-up
        ed.edit(img, masked_content=mode, **kw)
    wall = {mode: [] for mode in MODES}
    for _ in range(args.rounds):
        for mode in MODES:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            ed.edit(img, masked_content=mode, **kw)
            wall[mode].append((time.perf_counter() - t0) * 1e3)
    src = ctx.resize_lanczos(torch.from_numpy(np.array(img)).to(ctx.device), 1024, 1024)
    ctl = ctx.canny_device(src)
    mdev = ed._mask_device(np.array(mask), (1024, 1024))
    gen = lambda: torch.Generator("cpu").manual_seed(42)
    jobs = {mode: pipe.prepare(kw["prompt"], "", src, ctl, 0.8, 4, 1.5, 0.5, gen(), mdev, args.mask_blur, True, masked_content=mode) for mode in MODES}
    replay = {mode: [] for mode in MODES}
    st = pipe.slot_stream(0)
    st.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(st):
        for _ in range(args.rounds):
            for mode in MODES:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                pipe.run_device_graphed(jobs[mode])
                e1.record()
                st.synchronize()
                replay[mode].append(e0.elapsed_time(e1))
    med = statistics.median
    for name, t, unit in (("FastEditor.edit wall", wall, "ms"), ("graph replay device", replay, "ms")):
        print(f"{name} {unit} (median of {args.rounds}): " + ", ".join(f"{mode} {med(t[mode]):.3f}" for mode in MODES))
        print("  ratio to original: " + ", ".join(f"{mode} {med(t[mode]) / med(t['original']):.4f}" for mode in MODES[1:]))


if __name__ == "__main__":
    main()
