#!/usr/bin/env python3
"""What the full-resolution back end costs: one process, interleaved runs, device events.

    python tools/fullres_ab.py [--rounds 30] [--blurs 0,4] [--model ssd-1b | --no_edit]

1. the back end alone, a 1024x1024 result -> a 4000x3000 source with a box mask over 30 % of the image, per feather sigma:
     fused      fie_fullres_paste_rgb_u8 (two launches)
     fused (A)  the same again: the A/A spread of this script
     parts      the existing entries an unfused form starts with, fie_resize_rgb_u8 to 4000x3000 and fie_mask_prep at 4000x3000 -- WITHOUT any
                composite.  The library has no composite of two u8 images through an f32 mask (fie_pixels_out_composite_* reads the decoder's
                NHWC floats), so this is a lower bound of every unfused sequence
     unfused    parts + the composite written with torch ops (several launches: an upper bound of what one hand-written composite would cost)
   The four are run one after the other inside each round, `rounds` times; medians and the 10 % / 90 % quantiles of the device time are
   printed, with the bytes each form moves per output pixel (counted from the shapes) and the fused form's share of the HBM roof.
2. the whole call: FastEditor.edit(image, mask=..., output_size="source") against today's edit() followed by the caller's Pillow resize and
   Image.composite on the host (host in, host out, wall clock), alternating."""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_BYTES_PER_S = 8.0e12          # MI355X peak


def quant(v):
    s = sorted(v)
    return statistics.median(s), s[len(s) // 10], s[(len(s) * 9) // 10]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="ssd-1b", choices=["ssd-1b", "sdxl", "tiny"])
    ap.add_argument("--rounds", type=int, default=30)
    ap.add_argument("--blurs", default="0,4")
    ap.add_argument("--no_edit", action="store_true", help="part 1 only")
    args = ap.parse_args()
    import numpy as np
    import torch
    from PIL import Image, ImageFilter
    import fie_amd  # noqa: F401
    from bench import synth_item_image
    from fie_amd import hip
    from fie_amd import mask as hmask

    blurs = [float(b) for b in args.blurs.split(",")]
    H, W, h, w = 3000, 4000, 1024, 1024
    big = synth_item_image(5).resize((W, H), Image.BICUBIC)
    noise = np.random.default_rng(0).integers(-12, 13, (H, W, 3))
    big = Image.fromarray((np.asarray(big).astype(int) + noise).clip(0, 255).astype(np.uint8))
    m = np.zeros((H, W), np.uint8)
    m[600:2400, 1000:3000] = 255                       # 1800 x 2000 = 30 % of 12 MP
    ctx = hip.context(0)
    dev = ctx.device
    res = torch.from_numpy(np.asarray(synth_item_image(6).resize((w, h), Image.BICUBIC))).to(dev)
    src, mk = torch.from_numpy(np.asarray(big)).to(dev), torch.from_numpy(m).to(dev)
    out = torch.empty_like(src)

    def torch_composite(up, m_px):
        mm = m_px[..., None]
        mix = torch.round(mm * up.float() + (1.0 - mm) * src.float()).to(torch.uint8)
        return torch.where(mm <= 0, src, torch.where(mm >= 1, up, mix))

    def parts(r):
        return ctx.resize_lanczos(res, H, W), ctx.mask_prep(mk, r)[0]

    print(f"back end alone: {h}x{w} -> {H}x{W}, mask over {float((m > 0).mean()):.0%}, {args.rounds} interleaved rounds, device ms: median [10 %, 90 %]")
    for r in blurs:
        forms = {"fused": lambda: ctx.fullres_paste(res, src, mk, r, out=out),
                 "fused (A)": lambda: ctx.fullres_paste(res, src, mk, r, out=out),
                 "parts": lambda: parts(r),
                 "unfused": lambda: torch_composite(*parts(r))}
        for f in forms.values():                        # warm-up: tables, taps, code objects, allocator
            for _ in range(3):
                f()
        torch.cuda.synchronize()
        want = torch_composite(*parts(r))
        diff = (ctx.fullres_paste(res, src, mk, r).int() - want.int()).abs()
        print(f"  r = {r:g}: fused vs unfused output: max |diff| {int(diff.max())}, differing bytes {int((diff > 0).sum())} of {diff.numel()}")
        ms = {k: [] for k in forms}
        for _ in range(args.rounds):
            for k, f in forms.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                f()
                e1.record()
                e1.synchronize()
                ms[k].append(e0.elapsed_time(e1))
        R = hmask.blur_radius(r)
        # bytes per output pixel, from the shapes: the horizontal pass (reads the result once, writes tmp [h, W, 3]) is common to all forms
        common = (h * w * 3 + h * W * 3) / (H * W)
        bpp = {"fused": common + 1 + 3 + 3 + 3 * h / H, "parts": common + 3 * h / H + 3 + 1 + 4}
        bpp["fused (A)"] = bpp["fused"]
        bpp["unfused"] = bpp["parts"] + 3 + 4 + 3 + 3
        for k in forms:
            med, lo, hi = quant(ms[k])
            roof = bpp[k] * H * W / HBM_BYTES_PER_S * 1e3
            print(f"    {k:<10} {med:7.3f} [{lo:7.3f}, {hi:7.3f}]   >= {bpp[k]:5.2f} B/pixel compulsory -> {roof / med:5.1%} of the HBM roof (R = {R})")
        aa = abs(quant(ms["fused"])[0] - quant(ms["fused (A)"])[0])
        print(f"    A/A spread {aa:.3f} ms; fused - parts = {quant(ms['fused'])[0] - quant(ms['parts'])[0]:+.3f} ms; "
              f"fused - unfused = {quant(ms['fused'])[0] - quant(ms['unfused'])[0]:+.3f} ms")
    if args.no_edit:
        return

    from src.pipeline import FastEditor
    ed = FastEditor(model_name=args.model, use_full_controlnet=True, enable_cpu_offload=False)
    mask = Image.fromarray(m)
    kw = dict(prompt="a [red] ball on the table", seed=42)
    print(f"whole call on a {W}x{H} source ({args.model}), wall ms host in -> host out: median [10 %, 90 %]")
    for r in blurs:
        def host_form():
            e = ed.edit(big, mask=mask, paste_back=False, **kw)
            up = e.resize(big.size, Image.LANCZOS)
            mb = mask.point(lambda v: 255 if v >= 128 else 0)
            if r > 0:
                mb = mb.filter(ImageFilter.GaussianBlur(r))
            return Image.composite(up, big, mb)
        forms = {"edit(output_size='source')": lambda: ed.edit(big, mask=mask, mask_blur=r, output_size="source", **kw),
                 "edit() + Pillow on the host": host_form,
                 "edit() alone (1024x1024 out)": lambda: ed.edit(big, mask=mask, mask_blur=r, **kw)}
        for f in forms.values():
            f()
            f()
        ms = {k: [] for k in forms}
        for _ in range(max(5, args.rounds // 3)):
            for k, f in forms.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                f()
                ms[k].append((time.perf_counter() - t0) * 1e3)
        for k in forms:
            med, lo, hi = quant(ms[k])
            print(f"  r = {r:g}  {k:<30} {med:8.2f} [{lo:8.2f}, {hi:8.2f}]")


if __name__ == "__main__":
    main()
