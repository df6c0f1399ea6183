#!/usr/bin/env python3
"""What a strength sweep costs against the serial calls it replaces: one process, one FastEditor (the bench configuration:
SSD-1B + full ControlNet, fp16, 1024^2, 4 steps, CFG 1.5), strengths="all".  The sibling of tools/tile_blend_ab.py.

    python tools/sweep_ab.py [--rounds 20] [--out profiles/sweep_ab.md]

1. the selector alone: fie_sweep_select_u8 over k = 4 images of 3 MB (1024 x 1024 x 3) and 36 MB (4000 x 3000 x 3), sources congruent to the
   output mod 16 and one byte off, HIP events around `--calls` back-to-back calls, median over `--rounds` windows; bytes copied per second and
   bytes moved (read + written) against the float4 copy rate of the chip.  Back-to-back calls re-read the same buffers: at these sizes they sit in
   the Infinity Cache, as the k images of a sweep do when the selector runs right behind the scorer;
2. outputs: the four serial edits and the sweep's four variants on one seed, max |du8| and SSIM of each pair at the timed size (the bound of
   tests/test_sweep_gpu.py: <= 2 and > 0.999);
3. time: (A) four serial edit(strength=s, metrics=True) calls and the pick on the host -- what a caller does without the sweep --, (B)
   edit_sweep(select="strongest", min_ssim=...) with the floor between two variants' SSIM, (A2) A again.  Wall time host in, host out,
   interleaved A, B, A2 per round, median over `--rounds` rounds after warming every graph.  A2 / A is the spread of the measurement;
4. stage times of one eager pass of each side (HipImg2ImgPipeline.stage_ms; A: summed over its four edits);
5. 3 once more with output_size="source" on a 4000 x 3000 source: A copies four 36 MB images to the host, B one.
The report is printed and written to `--out` as markdown."""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

COPY_RATE = 6.29e12          # bytes moved per second by a float4 copy kernel on the MI355X (measured; 79 % of the HBM3E peak)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="ssd-1b", choices=["ssd-1b", "sdxl", "tiny"])
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--big_rounds", type=int, default=20, help="rounds of the 4000 x 3000 pair")
    ap.add_argument("--calls", type=int, default=20, help="back-to-back calls of the op per timed window")
    ap.add_argument("--steps", type=int, default=4)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sweep_ab.md"))
    args = ap.parse_args()
    import numpy as np
    import torch
    from PIL import Image
    import fie_amd  # noqa: F401
    from bench import synth_item_image
    from fie_amd import metrics as hmetrics
    from fie_amd import sweep as hsweep
    from src.pipeline import FastEditor

    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    ed = FastEditor(model_name=args.model, use_full_controlnet=True, enable_cpu_offload=False)
    pipe, ctx = ed.pipe, ed.pipe.ctx
    med = statistics.median
    st = pipe.slot_stream(0)
    say("# Strength sweep A/B (`tools/sweep_ab.py`)")
    say()
    say(f"{torch.cuda.get_device_name(0)}; model {args.model} + full ControlNet, fp16, 1024 x 1024, {args.steps} steps, CFG 1.5, strengths=\"all\"; "
        f"{args.rounds} rounds ({args.big_rounds} at 4000 x 3000), {args.rounds} windows of {args.calls} calls (op).")
    say()

    # 1. the selector alone
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

    say("## The selector alone: `fie_sweep_select_u8`, k = 4")
    say()
    say("| image | sources | us per call (median, minimum) | copied, GB/s | moved (read + written), TB/s | of the 6.29 TB/s copy rate |")
    say("|---|---|---|---|---|---|")
    rows = torch.from_numpy(np.array([[0, 0, 0, 0]] * 4, np.int64)).to(ctx.device)
    rows.view(torch.float64)[:, 1] = torch.tensor([1.0, 2.0, 3.0, 4.0], dtype=torch.float64)       # floor 2.5: the winner is image 2
    for name, nbytes in (("1024 x 1024 x 3 (3.1 MB)", 1024 * 1024 * 3), ("4000 x 3000 x 3 (36 MB)", 4000 * 3000 * 3)):
        for what, off in (("congruent mod 16", 0), ("one byte off", 1)):
            bases = [torch.randint(0, 256, (nbytes + 16,), device=ctx.device, dtype=torch.uint8) for _ in range(4)]
            srcs = [b[off:off + nbytes] for b in bases]
            out = torch.empty(nbytes, device=ctx.device, dtype=torch.uint8)
            idx = torch.empty(1, device=ctx.device, dtype=torch.int32)
            t, lo = timed(lambda: ctx.sweep_select(srcs, rows, None, "strongest", 2.5, False, out=out, out_idx=idx))
            torch.cuda.synchronize()
            assert int(idx.cpu()[0]) == 2 and torch.equal(out, srcs[2])
            say(f"| {name} | {what} | {t:.1f} ({lo:.1f}) | {nbytes / t / 1e3:.0f} | {2 * nbytes / t / 1e6:.2f} | {2 * nbytes / (t * 1e-6) / COPY_RATE:.2f} |")
            del bases, srcs, out
    say()

    # 2 - 4. the edit-size pair
    vs = hsweep.variants(args.steps, "all")
    strengths = [v[1][0] for v in vs]
    kw = dict(prompt="a [red] bicycle", num_inference_steps=args.steps, seed=42)
    img = synth_item_image(3)

    def side_a(image, floor, **more):
        """What a caller does without the sweep: one edit per strength, each scored, the rule on the host."""
        res = [ed.edit(image, strength=s, metrics=True, **kw, **more) for s in strengths]
        ok = [i for i, (_, m) in enumerate(res) if m["ssim"] >= floor]
        pick = ok[0] if ok else max(range(len(res)), key=lambda i: (res[i][1]["ssim"], i))
        return res, pick

    def side_b(image, floor, **more):
        return ed.edit_sweep(image, strengths="all", select="strongest", min_ssim=floor, **kw, **more)

    def compare(serial, imgs, variants, bound):
        """The table of serial edit against sweep variant; with `bound` the pairs must meet the bound of tests/test_sweep_gpu.py."""
        say("| steps | max du8 | SSIM of the pair | SSIM to the source, serial | SSIM to the source, sweep |")
        say("|---|---|---|---|---|")
        for (a, am), b, v in zip(serial, imgs, variants):
            a8, b8 = np.asarray(a), np.asarray(b)
            d = int(np.abs(a8.astype(int) - b8.astype(int)).max())
            with torch.cuda.stream(st):
                r = ctx.metrics_pairs(torch.from_numpy(a8.copy()).to(ctx.device), torch.from_numpy(b8.copy()).to(ctx.device)).cpu().numpy()
            s = hmetrics.rows_to_dicts(r, a8.shape[0], a8.shape[1])[0]["ssim"]
            say(f"| {v['steps']} | {d} | {s:.6f} | {am['ssim']:.6f} | {v['ssim']:.6f} |")
            assert s > 0.999 and (d <= 2 or not bound), (v["steps"], d, s)
        say()

    def pair(image, rounds, title, resampled=False, **more):
        serial, _ = side_a(image, 0.0, **more)                    # captures + warm-up of both sides; the floor comes from the variants themselves
        imgs, variants = ed.edit_sweep(image, strengths="all", **kw, **more)
        ss = sorted(v["ssim"] for v in variants)
        floor = (ss[len(ss) // 2 - 1] + ss[len(ss) // 2]) / 2
        say(f"## {title}")
        say()
        if resampled:
            # the bound is one on what the device job computes: the same jobs' edit-size results (the back end is queued behind the job, outside it)
            plain = {k: v for k, v in more.items() if k != "output_size"}
            say("Outputs on one seed at the edit size (the same device jobs without the back end), serial edit against the sweep's variant:")
            say()
            compare(side_a(image, 0.0, **plain)[0], *ed.edit_sweep(image, strengths="all", **kw, **plain), bound=True)
            say("The same at the source's size.  Pillow's LANCZOS filter has negative lobes: half way between two samples its six taps are 0.024, -0.136, "
                "0.611, 0.611, -0.136, 0.024, absolute sum 1.54 per axis, so the two passes of an upscale can turn a difference of one level between "
                "two inputs into three levels between the outputs.  Reported, not bounded:")
            say()
        else:
            say("Outputs on one seed, serial edit against the sweep's variant:")
            say()
        compare(serial, imgs, variants, bound=not resampled)
        _, pick_a = side_a(image, floor, **more)
        _, info = side_b(image, floor, **more)
        assert pick_a == info["index"], (pick_a, info["index"])
        wall = {"A": [], "B": [], "A2": []}
        for _ in range(rounds):
            for side in ("A", "B", "A2"):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                side_b(image, floor, **more) if side == "B" else side_a(image, floor, **more)
                wall[side].append((time.perf_counter() - t0) * 1e3)
        a, b, a2 = med(wall["A"]), med(wall["B"]), med(wall["A2"])
        say(f"`min_ssim` {floor:.4f} (between two variants): both sides pick variant {pick_a} ({variants[pick_a]['steps']} steps).")
        say()
        say(f"Wall ms, host in, host out (median of {rounds}, interleaved; minimum in brackets): A {a:.2f} ({min(wall['A']):.2f}), B {b:.2f} "
            f"({min(wall['B']):.2f}), A2 {a2:.2f} ({min(wall['A2']):.2f}).")
        say(f"B / A {b / a:.4f} ({b - a:+.2f} ms); A/A spread A2 / A {a2 / a:.4f} ({a2 - a:+.2f} ms).")
        say()
        return floor

    floor = pair(img, args.rounds, "1024 x 1024: four serial edits and the pick on the host (A) against `edit_sweep(select=\"strongest\")` (B)")

    pipe.use_graph = False
    try:
        stages = {}
        for side in ("A", "B"):
            acc = {}
            for s in (strengths if side == "A" else [None]):
                pipe.timing = []
                if side == "A":
                    ed.edit(img, strength=s, metrics=True, **kw)
                else:
                    side_b(img, floor)
                for name, ms in pipe.stage_ms().items():
                    acc[name] = acc.get(name, 0.0) + ms
            stages[side] = acc
    finally:
        pipe.timing = None
        pipe.use_graph = True
    say("Stage times of one eager pass, device ms (A: summed over its four edits):")
    say()
    say("| stage | A | B |")
    say("|---|---|---|")
    for name in stages["A"]:
        say(f"| {name} | {stages['A'][name]:.2f} | {stages['B'].get(name, 0.0):.2f} |")
    say(f"| sum | {sum(stages['A'].values()):.2f} | {sum(stages['B'].values()):.2f} |")
    say()

    # 5. the source-size pair
    big = synth_item_image(5).resize((4000, 3000), Image.BICUBIC)
    pair(big, args.big_rounds, "4000 x 3000 source, `output_size=\"source\"`: A copies four 36 MB images to the host, B one", resampled=True,
         output_size="source")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
