#!/usr/bin/env python3
"""What a mask-restricted edit costs: one process, one FastEditor (the bench configuration: SSD-1B + full ControlNet,
fp16, 1024^2), the same 512^2 image edited without and with a 512^2 mask (paste-back on), alternating, graph-replayed.

    python tools/masked_edit_ab.py [--rounds 20] [--mask_blur 0]

1. launches per edit: one eager edit of each kind with the library's launch log on (include/fie.h: fie_debug_oplog), kernel launches counted
   ('#' stage marks excluded) and the launches the masked edit adds or swaps listed by kernel;
2. time per edit: FastEditor.edit() wall time (host in, host out: mask upload, resize and prep included), and the device time of the graph
   replay alone (HIP events around the replay of a prepared job), median over `rounds` alternations after one warm-up edit of each kind."""
import argparse
import collections
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


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
    m[128:384, 96:352] = 255
    mask = Image.fromarray(m)
    kw = dict(prompt="a [red] ball on the table", seed=42)
    masked_kw = dict(mask=mask, mask_blur=args.mask_blur)

    # 1. launches per edit (eager, log on)
    pipe.use_graph = False
    counts = {}
    for tag, extra in (("unmasked", {}), ("masked", masked_kw)):
        ed.edit(img, **kw, **extra)
        torch.cuda.synchronize()
        ctx.oplog(True)
        ed.edit(img, **kw, **extra)
        torch.cuda.synchronize()
        counts[tag] = kernels(ctx.oplog_read())
        ctx.oplog(False)
    pipe.use_graph = True
    a, b = collections.Counter(counts["unmasked"]), collections.Counter(counts["masked"])
    print(f"launches per edit: unmasked {len(counts['unmasked'])}, masked {len(counts['masked'])} "
          f"(+{len(counts['masked']) - len(counts['unmasked'])})")
    for k in sorted(set(a) | set(b)):
        if a[k] != b[k]:
            print(f"  {k}: {a[k]} -> {b[k]}")

    # 2. time per edit, alternating
    for extra in ({}, masked_kw):                       # captures + warm-up
        ed.edit(img, **kw, **extra)
    wall = {"unmasked": [], "masked": []}
    for _ in range(args.rounds):
        for tag, extra in (("unmasked", {}), ("masked", masked_kw)):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            ed.edit(img, **kw, **extra)
            wall[tag].append((time.perf_counter() - t0) * 1e3)
    src = ctx.resize_lanczos(torch.from_numpy(np.array(img)).to(ctx.device), 1024, 1024)
    ctl = ctx.canny_device(src)
    mdev = ed._mask_device(np.asarray(mask), (1024, 1024))
    gen = lambda: torch.Generator("cpu").manual_seed(42)
    jobs = {"unmasked": pipe.prepare(kw["prompt"], "", src, ctl, 0.8, 4, 1.5, 0.5, gen()),
            "masked": pipe.prepare(kw["prompt"], "", src, ctl, 0.8, 4, 1.5, 0.5, gen(), mdev, args.mask_blur, True)}
    replay = {"unmasked": [], "masked": []}
    st = pipe.slot_stream(0)
    st.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(st):
        for _ in range(args.rounds):
            for tag in ("unmasked", "masked"):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                pipe.run_device_graphed(jobs[tag])
                e1.record()
                st.synchronize()
                replay[tag].append(e0.elapsed_time(e1))
    med = lambda v: statistics.median(v)
    print(f"FastEditor.edit wall ms (median of {args.rounds}): unmasked {med(wall['unmasked']):.2f}, masked {med(wall['masked']):.2f}, "
          f"ratio {med(wall['masked']) / med(wall['unmasked']):.4f}")
    print(f"graph replay device ms (median of {args.rounds}): unmasked {med(replay['unmasked']):.3f}, masked {med(replay['masked']):.3f}, "
          f"ratio {med(replay['masked']) / med(replay['unmasked']):.4f}")


if __name__ == "__main__":
    main()
