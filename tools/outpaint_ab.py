#!/usr/bin/env python3
"""What `outpaint` costs: one process, one FastEditor (the bench configuration: SSD-1B + full ControlNet, fp16, 1024^2).
The sibling of tools/mask_grow_ab.py.

    python tools/outpaint_ab.py [--rounds 20] [--out profiles/outpaint_ab.md]

1. the op alone: fie_outpaint_canvas_rgb_u8 at 1024 x 1024 + 256 on every side and at 4000 x 3000 + 512 on the right, with a mask, HIP events
   around `--calls` back-to-back calls, median and minimum over `--rounds` windows, and the bytes it moves per second (source and mask read
   once, both outputs written once).  Beside it the yardstick: the same canvas and mask made with torch on the device in the same process -- a
   strided copy_ of the interior, the four edge expansions, the mask's fill and interior copy -- checked equal to the op's before it is timed;
2. time per edit: FastEditor.edit() wall time (host in, host out) of `edit(image, outpaint=o, masked_content="fill", output_size="source")`
   against the same edit on a canvas the host builds inside the timed span (np.pad(mode="edge"), the mask, the larger upload), interleaved,
   bracketed by two series of the edit on a canvas built beforehand: those two are the A/A pair, their ratio the spread of the measurement.
The report is printed and written to `--out` as markdown."""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SIDES = ("prebuilt", "host", "device", "prebuilt_again")
OP_CASES = (((1024, 1024), (256, 256, 256, 256)), ((3000, 4000), (0, 0, 512, 0)))      # (H, W), (left, top, right, bottom)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="ssd-1b", choices=["ssd-1b", "sdxl", "tiny"])
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--calls", type=int, default=20, help="back-to-back calls of the op per timed window")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "outpaint_ab.md"))
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

    def torch_canvas(src, mask, margins, canvas, cmask):
        """The yardstick: the op's two outputs composed from torch's own kernels."""
        l, t, r, b = margins
        h, w, _ = src.shape
        canvas[t:t + h, l:l + w].copy_(src)
        if l:
            canvas[t:t + h, :l] = src[:, :1]
        if r:
            canvas[t:t + h, l + w:] = src[:, -1:]
        if t:
            canvas[:t] = canvas[t:t + 1]
        if b:
            canvas[t + h:] = canvas[t + h - 1:t + h]
        cmask.fill_(255)
        cmask[t:t + h, l:l + w].copy_(mask)

    # 1. the op alone
    say("# `outpaint` A/B (`tools/outpaint_ab.py`)")
    say()
    say(f"{torch.cuda.get_device_name(0)}; model {args.model}; {args.rounds} windows of {args.calls} calls (op), {args.rounds} rounds (edit).")
    say()
    say("## The op alone: `fie_outpaint_canvas_rgb_u8` against the same canvas composed with torch, microseconds per call (median, minimum)")
    say()
    say("| source (H x W) | margins (l, t, r, b) | canvas | bytes moved | op | op, GB/s at the median | torch composition | torch / op |")
    say("|---|---|---|---|---|---|---|---|")
    for (h, w), margins in OP_CASES:
        l, t, r, b = margins
        hc, wc = t + h + b, l + w + r
        rng = np.random.default_rng(h)
        src = torch.from_numpy(rng.integers(0, 256, (h, w, 3), dtype=np.uint8)).to(ctx.device)
        mask = torch.from_numpy(rng.integers(0, 256, (h, w), dtype=np.uint8)).to(ctx.device)
        out = torch.empty((hc, wc, 3), dtype=torch.uint8, device=ctx.device), torch.empty((hc, wc), dtype=torch.uint8, device=ctx.device)
        ref = torch.empty_like(out[0]), torch.empty_like(out[1])
        with torch.cuda.stream(st):
            ctx.outpaint_canvas(src, mask, margins, out=out)
            torch_canvas(src, mask, margins, *ref)
            st.synchronize()
        assert torch.equal(out[0], ref[0]) and torch.equal(out[1], ref[1]), "the torch composition is not the op's canvas"
        t_op, lo_op = timed(lambda: ctx.outpaint_canvas(src, mask, margins, out=out))
        t_th, lo_th = timed(lambda: torch_canvas(src, mask, margins, *ref))
        nbytes = 4 * h * w + 4 * hc * wc
        say(f"| {h} x {w} | {margins} | {hc} x {wc} | {nbytes / 1e6:.1f} MB | {t_op:.1f} ({lo_op:.1f}) | {nbytes / t_op / 1e3:.0f} | "
            f"{t_th:.1f} ({lo_th:.1f}) | {t_th / t_op:.2f} |")
    say()

    # 2. time per edit, interleaved
    small = synth_item_image(3)
    big = small.resize((4000, 3000), Image.BICUBIC)
    for name, img, margins in (("512 x 512 source", small, (0, 0, 256, 0)), ("4000 x 3000 source", big, (0, 0, 512, 0))):
        l, t, r, b = margins
        kw = dict(prompt="a [wide] beach", seed=42, masked_content="fill", output_size="source")

        def host_canvas():
            a = np.asarray(img)
            m = np.full((t + a.shape[0] + b, l + a.shape[1] + r), 255, np.uint8)
            m[t:t + a.shape[0], l:l + a.shape[1]] = 0
            return Image.fromarray(np.pad(a, ((t, b), (l, r), (0, 0)), mode="edge")), m

        pre = host_canvas()
        run = {"prebuilt": lambda: ed.edit(pre[0], mask=pre[1], **kw),
               "host": lambda: (lambda cm: ed.edit(cm[0], mask=cm[1], **kw))(host_canvas()),
               "device": lambda: ed.edit(img, outpaint=margins, **kw)}
        run["prebuilt_again"] = run["prebuilt"]
        outs = {side: np.asarray(run[side]()) for side in SIDES[:3]}            # captures + warm-up
        assert np.array_equal(outs["device"], outs["host"]) and np.array_equal(outs["device"], outs["prebuilt"]), "the identity does not hold"
        wall = {side: [] for side in SIDES}
        for _ in range(args.rounds):
            for side in SIDES:
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                run[side]()
                wall[side].append((time.perf_counter() - t0) * 1e3)
        say(f"## A whole edit, {name}, outpaint={margins}, masked_content=\"fill\", output_size=\"source\"")
        say()
        say(f"`FastEditor.edit` wall ms (median of {args.rounds}, interleaved): " + ", ".join(f"{side} {med(wall[side]):.3f}" for side in SIDES) + ".")
        spread = abs(med(wall["prebuilt_again"]) - med(wall["prebuilt"]))
        say(f"device / host {med(wall['device']) / med(wall['host']):.4f} ({med(wall['device']) - med(wall['host']):+.3f} ms); "
            f"device - prebuilt {med(wall['device']) - med(wall['prebuilt']):+.3f} ms, host - prebuilt {med(wall['host']) - med(wall['prebuilt']):+.3f} ms; "
            f"A/A prebuilt_again / prebuilt {med(wall['prebuilt_again']) / med(wall['prebuilt']):.4f} (spread {spread:.3f} ms).")
        say()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
