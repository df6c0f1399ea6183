#!/usr/bin/env python3
"""Single-image driver -- drop-in for /root/reference/run_single_image.py (same flags and output layout) on the
MI355X-native `FastEditor`.

    python run_single_image.py --image path/to/image.jpg --prompt "a rusty bicycle"

`--compute_metrics` reports the metrics this build restates (SSIM, PSNR, MSE); LPIPS / CLIP score / DINO need
checkpoints that cannot be fetched offline: each is computed on the device from a local directory (`--lpips_dir`,
`--clip_score_dir`, `--dino_dir`) and reported as unavailable, instead of silently skipped, without one."""
import argparse
import os

os.environ.setdefault("GPU_MAX_HW_QUEUES", "16")    # before HIP initialises; see fie_amd.py
import sys
import time
from datetime import datetime

from PIL import Image

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))


def outpaint_arg(text):
    """argparse type of --outpaint: 'L,T,R,B' -> (left, top, right, bottom) (fie_amd/mask.py: parse_outpaint)."""
    import fie_amd  # noqa: F401
    from fie_amd import mask as hmask
    try:
        return hmask.parse_outpaint(text)
    except ValueError as e:
        raise argparse.ArgumentTypeError(str(e)) from None


def build_parser():
    p = argparse.ArgumentParser(description="Fast image editing on a single image")
    a = p.add_argument
    a("--image", type=str, required=True, help="Path to input image")
    a("--prompt", type=str, required=True, help="Editing prompt")
    a("--model", type=str, default="sdxl", choices=["sdxl", "ssd-1b"],
      help="Model to use: sdxl (full quality, ~6GB) or ssd-1b (faster, ~4GB)")
    a("--negative_prompt", type=str, default="", help="Negative prompt")
    a("--steps", type=int, default=4, help="Number of inference steps")
    a("--guidance", type=float, default=1.5, help="Guidance scale")
    a("--control_scale", type=float, default=0.5, help="ControlNet conditioning scale")
    a("--canny_low", type=int, default=100, help="Canny low threshold")
    a("--canny_high", type=int, default=200, help="Canny high threshold")
    a("--seed", type=int, default=None, help="Random seed")
    a("--output_dir", type=str, default="outputs", help="Output directory")
    a("--no_cpu_offload", action="store_true", help="Disable CPU offloading (faster but needs more VRAM)")
    a("--quality_mode", action="store_true", help="Maximum quality mode (fp32, full ControlNet) - A100 recommended")
    a("--full_precision", action="store_true", help="Use fp32 instead of fp16 (better quality, 2x VRAM)")
    a("--full_controlnet", action="store_true", help="Use full-size ControlNet instead of small variant")
    a("--compute_metrics", action="store_true", help="Compute metrics")
    a("--show_plot", action="store_true", help="Show comparison plot")
    a("--strength", type=float, default=None, help="[additive] img2img strength (default: FastEditor.edit's 0.80)")
    a("--weights_dir", type=str, default=None, help="[additive] local diffusers-layout weights directory")
    a("--mask", type=str, default=None, help="[additive] mask image (white = edit): only that region changes")
    a("--mask_blur", type=float, default=0, help="[additive] with --mask: Gaussian feather (sigma, pixels) of the paste-back seam")
    a("--no_paste_back", action="store_true", help="[additive] with --mask: blend in latent space only, no paste-back of the source")
    a("--masked_content", type=str, default="original", choices=["original", "fill", "latent_noise", "latent_nothing"],
      help="[additive] with --mask: what the model starts from inside the mask -- 'original' the source, 'fill' a smooth continuation of the "
           "surroundings (object removal), 'latent_noise' pure noise, 'latent_nothing' the zero latent plus noise; the three new modes also clear "
           "the edge map inside the mask")
    a("--blend", type=str, default="alpha", choices=["alpha", "multiband"],
      help="[additive] with --mask: how the edited region meets the source -- 'alpha' the paste-back as ever (one ramp, --mask_blur), 'multiband' a "
           "one-sided multi-band blend: the edit keeps its detail, its brightness / colour difference to the source fades out towards the seam, "
           "and outside the mask the output stays the source's bytes")
    a("--blend_levels", type=int, default=4, choices=range(1, 7), metavar="N",
      help="[additive] with --blend multiband: pyramid levels, 1..6; the difference fades over about 2^N pixels")
    a("--mask_grow", type=int, default=0, choices=range(-64, 65), metavar="N",
      help="[additive] with --mask: grow (N > 0) or shrink (N < 0) the mask by an exact disk of N pixels of the mask (the input image's pixels), "
           "-64..64, before anything else reads it")
    a("--mask_mode", type=str, default="binary", choices=["binary", "levels"],
      help="[additive] with --mask: 'levels' reads the mask's greys as a per-pixel strength (255 edited as white, lower levels released into the "
           "edit for the last steps only, 0 never); not with --mask_ramp or --mask_grow")
    a("--mask_ramp", type=int, default=0, choices=range(0, 65), metavar="N",
      help="[additive] with --mask: a soft mask from the binary mask's outline: the strength ramps up over N pixels of the mask (the input image's "
           "pixels) inward from its outline, 0..64; --mask_grow N in front moves the ramp outward")
    a("--outpaint", type=outpaint_arg, default=None, metavar="L,T,R,B",
      help="[additive] outpainting: make the picture larger by L, T, R, B pixels (left, top, right, bottom; each 0..4096, not all 0) and let the "
           "model invent the new border.  The border is the mask (a --mask is carried into it), so --mask_grow, --mask_blur, --masked_content, "
           "--blend and --region mask work without --mask; recommended: --masked_content fill --mask_grow 16 --blend multiband --output_size source")
    a("--resolution", type=str, default="square",
      help="[additive] output size: 'square' (1024x1024, the reference's), 'auto' (the SDXL aspect-ratio bucket nearest the source's) or WxH "
           "(multiples of 64, 512..2048, at most 1024^2 pixels)")
    a("--output_size", type=str, default="edit", choices=["edit", "source"],
      help="[additive] 'edit': the output at the size the edit ran at (--resolution); 'source': the output at the input image's own size, "
           "composited there against the input's own pixels (with --mask)")
    a("--region", type=str, default="none", choices=["none", "mask"],
      help="[additive] 'mask' (needs --mask): edit only a crop around the mask at the model's native size and return the source-size image with "
           "the crop composited in (implies --output_size source)")
    a("--region_padding", type=int, default=32, help="[additive] with --region mask: pixels of context around the mask's bounding box")
    a("--clip_score_dir", type=str, default=None,
      help="[additive] with --compute_metrics: a local transformers CLIPModel directory (openai/clip-vit-base-patch16 is the reference's): fills the "
           "CLIP score.  Default: FIE_CLIP_SCORE_DIR, else <FIE_WEIGHTS_DIR>/clip_score when it exists")
    a("--dino_dir", type=str, default=None,
      help="[additive] with --compute_metrics: a local transformers ViTModel directory (facebook/dino-vitb8 is the reference's): fills the DINO "
           "structure distance of a square pair.  Default: FIE_DINO_DIR, else <FIE_WEIGHTS_DIR>/dino when it exists")
    a("--lpips_dir", type=str, default=None,
      help="[additive] with --compute_metrics: a local directory with the LPIPS SqueezeNet weights (model.safetensors, or torchvision's "
           "squeezenet1_1*.pth beside the lpips package's squeeze.pth): fills LPIPS.  Default: FIE_LPIPS_DIR, else <FIE_WEIGHTS_DIR>/lpips when it exists")
    return p


def tiles_arg(text):
    """argparse type of --tiles: 'auto' or 'WxH' -> "auto" or (tw, th) (fie_amd/tiles.py: parse)."""
    import fie_amd  # noqa: F401
    from fie_amd import tiles as htiles
    try:
        return htiles.parse(text)
    except ValueError as e:
        raise argparse.ArgumentTypeError(str(e)) from None


def add_tile_args(p):
    """[additive] tiled edits, kept apart from build_parser() like run_batch.py's additive groups."""
    p.add_argument("--tiles", type=tiles_arg, default=None, metavar="{auto,WxH}",
                   help="[additive] tiled edit, for an image above 1024^2 pixels: cover it with overlapping tiles of one edit size ('auto': per axis "
                        "the smallest legal size that still overlaps by --tile_overlap; WxH: multiples of 64, 512..2048, at most 1024^2 pixels), edit "
                        "every tile at its native size and crossfade the results on the device into one image of the input's size.  Not with "
                        "--resolution, --region mask, --outpaint")
    p.add_argument("--tile_overlap", type=int, default=128, choices=range(0, 257), metavar="N",
                   help="[additive] with --tiles: pixels neighbouring tiles share at least, 0..256")
    p.add_argument("--tile_batch", type=int, default=4, choices=range(1, 17), metavar="N",
                   help="[additive] with --tiles: tiles per device job, 1..16")
    return p


def strengths_arg(text):
    """argparse type of --strengths: 'all' or 'a,b,c' -> "all" or a list of floats (fie_amd/sweep.py: variants checks the values)."""
    if text.strip() == "all":
        return "all"
    try:
        vals = [float(v) for v in text.split(",")]
    except ValueError:
        raise argparse.ArgumentTypeError(f"--strengths {text!r}: 'all' or comma-separated numbers in [0, 1]") from None
    if not vals or any(not 0.0 <= v <= 1.0 for v in vals):
        raise argparse.ArgumentTypeError(f"--strengths {text!r}: 'all' or comma-separated numbers in [0, 1]")
    return vals


def add_sweep_args(p):
    """[additive] strength sweeps, kept apart from build_parser() like add_tile_args."""
    p.add_argument("--sweep", action="store_true",
                   help="[additive] edit the image at several strengths in ONE device job (every distinct step count of --strengths), scored on "
                        "the device.  Not with --tiles, --region mask; --strength is ignored")
    p.add_argument("--strengths", type=strengths_arg, default="all", metavar="{all,a,b,c}",
                   help="[additive] with --sweep: the strengths to try, 'all' (one per step count 1..--steps) or comma-separated numbers")
    p.add_argument("--select", type=str, default="none", choices=["none", "clip_score", "strongest"],
                   help="[additive] with --sweep: 'none' saves every variant as <name>_steps<m>.jpg; 'strongest' keeps the strongest edit whose SSIM "
                        "against the source (the background's with --mask) stays at or above --min_ssim; 'clip_score' the edit with the best CLIP "
                        "score (needs --clip_score_dir).  The choice is made on the device and only the chosen image leaves it")
    p.add_argument("--min_ssim", type=float, default=None, help="[additive] with --sweep --select: the SSIM every candidate must keep, -1..1")
    return p


def add_canny_args(p):
    """[additive] edge-budget Canny, kept apart from build_parser() like add_tile_args."""
    p.add_argument("--canny_density", type=float, default=None, metavar="D",
                   help="[additive] pick the Canny thresholds for this image, on the device, so that about this fraction of the pixels (0.001..0.25; "
                        "0.01..0.03 on the synthetic images this was tried on) are strong edge seeds: a hazy image still gets an edge map, a noisy "
                        "one is not nailed to its noise.  --canny_low / --canny_high then give only the ratio low / high; the pair is printed")
    return p


def add_emphasis_args(p):
    """[additive] prompt emphasis, kept apart from build_parser() like add_tile_args."""
    p.add_argument("--prompt_emphasis", type=float, default=None, metavar="W",
                   help="[additive] read the marks of --prompt and --negative_prompt: '[words]' (how PIE-Bench writes the words an edit changes) "
                        "weighs its words by W, 0..8, in every cross-attention, '(words:1.3)' by the written number; the marks are stripped before "
                        "tokenisation.  Prompt-to-Prompt and front ends use 1.1..2; no weight has been tried on real checkpoints.  Without the "
                        "flag a prompt is tokenised as it is, brackets included")
    return p


def add_control_args(p):
    """[additive] control weights, kept apart from build_parser() like add_emphasis_args."""
    p.add_argument("--control_layers", default=None, metavar="PRESET|N,N,...",
                   help="[additive] a factor on --control_scale for each of the ControlNet's residuals (SDXL / SSD-1B: 10, the mid block's last): "
                        "'balanced', 'prompt' (0.825 ** (9 - i): the prompt matters more), 'guess' (diffusers' guess_mode ramp), or comma-separated "
                        "numbers in [0, 2]")
    p.add_argument("--control_steps", default=None, metavar="A:B",
                   help="[additive] diffusers' control_guidance_start:control_guidance_end in [0, 1], over the steps that run after --strength; a "
                        "step outside the window runs no ControlNet")
    p.add_argument("--control_in_mask", type=float, default=None, metavar="X",
                   help="[additive] scale the ControlNet's residuals inside --mask by X in [0, 1] relative to outside: 0 lets go of the edge map "
                        "where the edit happens.  No preset, window or value has been tried on real checkpoints.  Without the three flags nothing changes")
    return p


def control_keywords(args):
    """The keywords of FastEditor.set_control_weights from the three flags, checked for a 10-residual ControlNet; {} without them.  ValueError."""
    from fie_amd import control as hctl
    parts = [f"{k}={v}" for k, v in (("layers", args.control_layers), ("steps", args.control_steps), ("in_mask", args.control_in_mask)) if v is not None]
    if not parts:
        return {}
    kw = hctl.parse_env(";".join(parts))
    hctl.check(kw.get("layers"), kw.get("steps"), kw.get("in_mask"), 10)
    return kw


def full_parser():
    """The parser main() reads: build_parser() and every additive group."""
    return add_control_args(add_emphasis_args(add_canny_args(add_sweep_args(add_tile_args(build_parser())))))


def save_plot(path, source_img, edited_img, model, prompt):
    import matplotlib
    matplotlib.use("Agg")
    import matplotlib.pyplot as plt
    fig, axes = plt.subplots(1, 2, figsize=(12, 6))
    axes[0].imshow(source_img)
    axes[0].set_title("Source Image")
    axes[1].imshow(edited_img)
    axes[1].set_title(f'Edited Image ({model.upper()})\n"{prompt}"')
    for ax in axes:
        ax.axis("off")
    plt.tight_layout()
    plt.savefig(path, dpi=150, bbox_inches="tight")
    plt.close(fig)
    print(f"      Saved comparison plot to: {path}")


def main(argv=None):
    parser = full_parser()
    args = parser.parse_args(argv)
    if not args.sweep and (args.select != "none" or args.min_ssim is not None):
        parser.error("--select and --min_ssim need --sweep")
    if args.sweep:
        if args.tiles is not None or args.region != "none":
            parser.error("--sweep does not go with --tiles or --region mask: a sweep is one device job on the whole image")
        if args.select == "strongest" and args.min_ssim is None:
            parser.error("--select strongest needs --min_ssim")
        if args.select == "none" and args.min_ssim is not None:
            parser.error("--min_ssim needs --select")
        if args.min_ssim is not None and not -1.0 <= args.min_ssim <= 1.0:
            parser.error("--min_ssim: a number in -1..1")
        if args.select == "clip_score":
            import fie_amd  # noqa: F401
            from fie_amd import clip_score as hclip
            args.clip_score_dir = hclip.resolve_dir(args.clip_score_dir)
            if args.clip_score_dir is None:
                parser.error("--select clip_score needs --clip_score_dir")
    masked = args.mask is not None or args.outpaint is not None        # --outpaint: the new border is a mask
    if args.tiles is not None and (args.resolution != "square" or args.region != "none" or args.outpaint is not None):
        parser.error("--tiles does not go with --resolution, --region mask or --outpaint: the tile size is the edit size and the output has the "
                     "input's size")
    if args.region == "mask" and not masked:
        parser.error("--region mask needs --mask")
    import fie_amd  # noqa: F401
    from fie_amd import buckets, canny_auto as hcanny, emphasis as hemph, mask as hmask
    try:
        mask_kw = hmask.cli_keywords(args, masked, "--mask")
        hcanny.check(args.canny_density, args.canny_low, args.canny_high)
        if args.prompt_emphasis is not None:                            # the marks of both prompts, read before the models load
            for text in (args.prompt, args.negative_prompt or ""):
                hemph.parse(text, args.prompt_emphasis)
        control_kw = control_keywords(args)                             # the three control flags, read before the models load
    except ValueError as e:
        parser.error(str(e))
    if args.resolution != "square":
        args.resolution = buckets.parse(args.resolution)
    if args.quality_mode:
        args.full_precision = args.full_controlnet = args.no_cpu_offload = True
        print("[Quality Mode] Enabled: fp32 + full ControlNet + no CPU offload")
    if not os.path.exists(args.image):
        print(f"Error: Image not found at {args.image}")
        return
    model_suffix = f"{args.model}_{'fp32' if args.full_precision else 'fp16'}"
    edited_dir = os.path.join(args.output_dir, "single", "edited", model_suffix)
    comparisons_dir = os.path.join(args.output_dir, "single", "comparisons", model_suffix)
    os.makedirs(edited_dir, exist_ok=True)
    os.makedirs(comparisons_dir, exist_ok=True)

    print(f"\n[1/4] Loading image from {args.image}")
    source_img = Image.open(args.image).convert("RGB")
    print(f"      Image size: {source_img.size}")

    print("\n[2/4] Initializing FastEditor...")
    from src.pipeline import FastEditor
    editor = FastEditor(model_name=args.model, device="cuda", enable_cpu_offload=not args.no_cpu_offload,
                        use_full_precision=args.full_precision, use_full_controlnet=args.full_controlnet,
                        weights_dir=args.weights_dir, **(dict(clip_score_dir=args.clip_score_dir) if args.sweep and args.select == "clip_score" else {}))
    mem = editor.get_memory_usage()
    print(f"      GPU Memory: {mem['allocated_gb']:.2f}GB allocated, {mem['reserved_gb']:.2f}GB reserved")

    print("\n[3/4] Running image editing...")
    print(f"      Prompt: {args.prompt}")
    print(f"      Steps: {args.steps}, Guidance: {args.guidance}, Control Scale: {args.control_scale}")
    extra = {} if args.strength is None else {"strength": args.strength}
    if args.mask is not None and not os.path.exists(args.mask):
        print(f"Error: Mask not found at {args.mask}")
        return
    if args.outpaint is not None:
        extra.update(outpaint=args.outpaint)
        print("      Outpaint: left %d, top %d, right %d, bottom %d px" % args.outpaint)
    if masked:
        if args.mask is not None:
            extra.update(mask=Image.open(args.mask))
        extra.update(mask_blur=args.mask_blur, paste_back=not args.no_paste_back)
        print(f"      Mask: {args.mask or 'the new border'} (blur {args.mask_blur}, paste-back {'off' if args.no_paste_back else 'on'})")
        extra.update(mask_kw)
        if "masked_content" in mask_kw:
            print(f"      Masked content: {args.masked_content}")
        if "blend" in mask_kw:
            print(f"      Blend: {args.blend}, {args.blend_levels} levels")
        if "mask_grow" in mask_kw:
            print(f"      Mask grown by: {args.mask_grow} px")
        if "mask_mode" in mask_kw:
            print(f"      Soft mask: {'the greys as levels' if args.mask_mode == 'levels' else f'ramp over {args.mask_ramp} px'}")
    if args.resolution != "square":
        extra.update(resolution=args.resolution)
    if args.region == "mask":
        extra.update(region="mask", region_padding=args.region_padding)
        print(f"      Region: the mask's box + {args.region_padding} px, output at the source's size")
    elif args.output_size == "source":
        extra.update(output_size="source")
    if args.tiles is not None:
        extra.update(tiles=args.tiles, tile_overlap=args.tile_overlap, tile_batch=args.tile_batch)
        extra.pop("output_size", None)
        print(f"      Tiles: {args.tiles if args.tiles == 'auto' else '%dx%d' % args.tiles}, overlap {args.tile_overlap} px, {args.tile_batch} per device job")
    if args.canny_density is not None:
        editor.set_canny_density(args.canny_density)
    if args.prompt_emphasis is not None:
        editor.set_prompt_emphasis(args.prompt_emphasis)
        print(f"      Prompt emphasis: [...] weighs {args.prompt_emphasis:g}; the prompt is tokenised as {hemph.parse(args.prompt, args.prompt_emphasis)[0]!r}")
    if control_kw:
        editor.set_control_weights(**control_kw)
        print(f"      Control weights: {editor.control_weights}")
    t0 = time.time()
    variants = None
    if args.sweep:
        extra.pop("strength", None)
        if args.select != "none":
            extra.update(select=args.select, **({} if args.min_ssim is None else dict(min_ssim=args.min_ssim)))
        edited_img, info = editor.edit_sweep(image=source_img, prompt=args.prompt, negative_prompt=args.negative_prompt, strengths=args.strengths,
                                             num_inference_steps=args.steps, guidance_scale=args.guidance,
                                             controlnet_conditioning_scale=args.control_scale, canny_low_threshold=args.canny_low,
                                             canny_high_threshold=args.canny_high, seed=args.seed, **extra)
        variants = info if args.select == "none" else info["variants"]
        for v in variants:
            print(f"      {v['steps']} steps (strength {', '.join(format(s, 'g') for s in v['strength'])}): SSIM {v['ssim']:.4f}"
                  + (f", background SSIM {v['bg_ssim']:.4f}" if "bg_ssim" in v else "") + (f", CLIP score {v['clip_score']:.2f}" if "clip_score" in v else ""))
        if args.select != "none":
            print(f"      Chosen by '{args.select}': {info['steps']} steps (variant {info['index']})")
    else:
        edited_img = editor.edit(image=source_img, prompt=args.prompt, negative_prompt=args.negative_prompt,
                                 num_inference_steps=args.steps, guidance_scale=args.guidance,
                                 controlnet_conditioning_scale=args.control_scale, canny_low_threshold=args.canny_low,
                                 canny_high_threshold=args.canny_high, seed=args.seed, **extra)
    elapsed = time.time() - t0
    print(f"      Editing completed in {elapsed:.2f} seconds")
    if args.canny_density is not None:
        for low, high in filter(None, editor.last_canny_thresholds()):
            print(f"      Canny thresholds picked at density {args.canny_density:g}: low={low}, high={high}")
    mem = editor.get_memory_usage()
    print(f"      GPU Memory: {mem['allocated_gb']:.2f}GB allocated, {mem['reserved_gb']:.2f}GB reserved")

    stamp = datetime.now().strftime("%Y%m%d_%H%M%S")
    output_path = os.path.join(edited_dir, f"edited_{stamp}.jpg")
    if isinstance(edited_img, list):                 # --sweep --select none: every variant, named by its step count; the strongest goes on below
        for im, v in zip(edited_img, variants):
            path = os.path.join(edited_dir, f"edited_{stamp}_steps{v['steps']}.jpg")
            im.save(path)
            print(f"\n      Saved the {v['steps']}-step variant to: {path}")
        edited_img = edited_img[0]
    else:
        edited_img.save(output_path)
        print(f"\n      Saved edited image to: {output_path}")

    if args.compute_metrics:
        print("\n[4/4] Computing metrics...")
        from src.metrics import MetricsCalculator
        calc = MetricsCalculator(device="cuda", clip_dir=args.clip_score_dir, dino_dir=args.dino_dir, lpips_dir=args.lpips_dir)
        metrics = calc.calculate_all_metrics(source_img=source_img, edited_img=edited_img, prompt=args.prompt)
        labels = [("ssim", "SSIM (structure preservation):  ", ".4f", ""), ("lpips", "LPIPS (perceptual distance):    ", ".4f", ""),
                  ("psnr", "PSNR (signal quality):          ", ".2f", " dB"), ("mse", "MSE (pixel difference):         ", ".6f", ""),
                  ("clip_score", "CLIP Score (text alignment):    ", ".2f", ""), ("dino_distance", "DINO distance (structure):      ", ".6f", "")]
        fmt = lambda k, f: "unavailable offline" if metrics.get(k) is None else format(metrics[k], f)
        print("\n      Metrics:")
        for k, label, f, unit in labels:
            print(f"        {label}{fmt(k, f)}{unit if metrics.get(k) is not None else ''}")
        metrics_path = os.path.join(edited_dir, f"metrics_{stamp}.txt")
        with open(metrics_path, "w") as fh:
            fh.write(f"Image: {args.image}\nPrompt: {args.prompt}\nModel: {args.model}\nTime: {elapsed:.2f}s\n\nMetrics:\n")
            for k, label, f, unit in labels:
                fh.write(f"  {k}: {fmt(k, f)}\n")
        print(f"      Saved metrics to: {metrics_path}")
        print("\n      Saving comparison plot...")
        save_plot(os.path.join(comparisons_dir, f"comparison_{stamp}.png"), source_img, edited_img, args.model, args.prompt)
        calc.clear_memory()
    elif args.show_plot:
        print("\n      Saving comparison plot...")
        save_plot(os.path.join(comparisons_dir, f"comparison_{stamp}.png"), source_img, edited_img, args.model, args.prompt)
    editor.clear_memory()
    print("\nDone!")


if __name__ == "__main__":
    main()
