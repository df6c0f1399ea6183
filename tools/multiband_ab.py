#!/usr/bin/env python3
"""What blend="multiband" costs: one process, one FastEditor (the bench configuration: SSD-1B + full ControlNet, fp16,
1024^2), the same 512^2 image edited with a 512^2-pixel mask at the edit size under blend="alpha" (the masked edit as it was) and under
blend="multiband" at `--levels` levels, interleaved, graph-replayed.  The sibling of tools/masked_content_ab.py.

    python tools/multiband_ab.py [--rounds 20] [--levels 4] [--mask_blur 0]

1. launches per edit: one eager edit of each side with the library's launch log on (include/fie.h: fie_debug_oplog), kernel launches counted
   ('#' stage marks excluded) and the launches "multiband" adds listed by kernel;
2. time per edit: FastEditor.edit() wall time (host in, host out), and the device time of the graph replay alone (HIP events around the replay
   of a prepared job), median over `rounds` rounds after one warm-up edit of each side.  Every round runs alpha, multiband, alpha: the two
   alpha series are the A/A pair, their ratio the spread of the measurement;
3. the op alone: HIP events around fie_multiband_blend_rgb_u8 on the job's own 1024^2 tensors (and around fie_pixels_out_* in front of it, the
   launch the alpha path fuses with its composite), median over `rounds` calls."""
import argparse
import collections
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SIDES = ("alpha", "multiband", "alpha_again")


def kernels(lines):
    return [l.split("|")[0] for l in lines if not l.startswith("#")]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="ssd-1b", choices=["ssd-1b", "sdxl", "tiny"])
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--levels", type=int, default=4)
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
    blend = {"alpha": dict(blend="alpha"), "multiband": dict(blend="multiband", blend_levels=args.levels), "alpha_again": dict(blend="alpha")}

    # 1. launches per edit (eager, log on)
    pipe.use_graph = False
    counts = {}
    for side in SIDES[:2]:
        ed.edit(img, **blend[side], **kw)
        torch.cuda.synchronize()
        ctx.oplog(True)
        ed.edit(img, **blend[side], **kw)
        torch.cuda.synchronize()
        counts[side] = kernels(ctx.oplog_read())
        ctx.oplog(False)
    pipe.use_graph = True
    base, c = collections.Counter(counts["alpha"]), collections.Counter(counts["multiband"])
    print(f"launches per edit: alpha {len(counts['alpha'])}, multiband {len(counts['multiband'])} (+{len(counts['multiband']) - len(counts['alpha'])})")
    for k in sorted(set(base) | set(c)):
        if base[k] != c[k]:
            print(f"  {k}: {base[k]} -> {c[k]}")

    # 2. time per edit, interleaved
    for side in SIDES[:2]:                              # captures + warm-up
        ed.edit(img, **blend[side], **kw)
    wall = {side: [] for side in SIDES}
    for _ in range(args.rounds):
        for side in SIDES:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            ed.edit(img, **blend[side], **kw)
            wall[side].append((time.perf_counter() - t0) * 1e3)
    src = ctx.resize_lanczos(torch.from_numpy(np.array(img)).to(ctx.device), 1024, 1024)
    ctl = ctx.canny_device(src)
    mdev = ed._mask_device(np.array(mask), (1024, 1024))
    gen = lambda: torch.Generator("cpu").manual_seed(42)
    jobs = {side: pipe.prepare(kw["prompt"], "", src, ctl, 0.8, 4, 1.5, 0.5, gen(), mdev, args.mask_blur, True, **blend[side]) for side in SIDES}
    replay = {side: [] for side in SIDES}
    st = pipe.slot_stream(0)
    st.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(st):
        for _ in range(args.rounds):
            for side in SIDES:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                pipe.run_device_graphed(jobs[side])
                e1.record()
                st.synchronize()
                replay[side].append(e0.elapsed_time(e1))
    med = statistics.median
    for name, t in (("FastEditor.edit wall", wall), ("graph replay device", replay)):
        print(f"{name} ms (median of {args.rounds}): " + ", ".join(f"{side} {med(t[side]):.3f}" for side in SIDES))
        print(f"  multiband / alpha {med(t['multiband']) / med(t['alpha']):.4f} ({med(t['multiband']) - med(t['alpha']):+.3f} ms); "
              f"A/A alpha_again / alpha {med(t['alpha_again']) / med(t['alpha']):.4f}")

    # 3. the op alone, on the job's tensors
    job = jobs["multiband"]
    decoded = torch.randint(0, 256, (1024, 1024, 3), dtype=torch.uint8, device=ctx.device)
    x = (decoded.to(ctx.dtype) / 127.5 - 1.0)
    x8 = torch.zeros((1, 1024, 1024, 8), dtype=ctx.dtype, device=ctx.device)
    x8[0, ..., :3] = x
    out = torch.empty_like(decoded)
    ws = ctx.multiband_workspace(1024, 1024, args.levels)
    ops = {"multiband_blend": lambda: ctx.multiband_blend(decoded, job["img_u8"], job["blend_l"][0], job["mask_px"][0], args.levels, out=out, workspace=ws),
           "pixels_out": lambda: ctx.pixels_out(x8),
           "pixels_out_composite": lambda: ctx.pixels_out_composite(x8, job["img_u8"], job["mask_px"][0])}
    with torch.cuda.stream(st):
        for name, op in ops.items():
            for _ in range(3):
                op()
            ts = []
            for _ in range(args.rounds):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                op()
                e1.record()
                st.synchronize()
                ts.append(e0.elapsed_time(e1) * 1e3)
            print(f"{name} alone, 1024^2 (median of {args.rounds}): {med(ts):.1f} us (min {min(ts):.1f})")
    print(f"workspace: {ws.numel() * ws.element_size() / 2 ** 20:.2f} MiB at {args.levels} levels")


if __name__ == "__main__":
    main()
