#!/usr/bin/env python3
"""PIE-Bench batch driver -- drop-in for /root/reference/run_batch.py (same flags, defaults, output layout and
summary), running the MI355X-native `FastEditor`.  New: launched under `torch.distributed.run` with N processes it
shards the selected entries image-parallel over N GPUs (fie_amd.dist) and rank 0 prints the merged summary.

    python run_batch.py --num_images 50 --editing_types 0 1 2
    python -m torch.distributed.run --nnodes=1 --nproc-per-node 8 --master-addr 127.0.0.1 run_batch.py --model ssd-1b

Additive flags (the reference has none of them): --strength, --weights_dir, --device, --results_json, --metrics, --clip_score_dir, --dino_dir, --lpips_dir,
--auto_strength, --min_ssim, --strengths.  FIE_CANNY_DENSITY=d in the environment runs every edit with an edge-budget Canny (FastEditor.set_canny_density;
DESIGN.md section 22): the pair picked for each image goes into --results_json as canny_low / canny_high.  FIE_PROMPT_EMPHASIS=w in the environment
reads the [...] marks of the PIE-Bench editing prompts as prompt emphasis of weight w (FastEditor.set_prompt_emphasis).
FIE_CONTROL_WEIGHTS="layers=prompt;steps=0:0.5;in_mask=0" (any subset of the three) runs every edit under those control weights
(FastEditor.set_control_weights).
"""
import argparse
import json
import os

os.environ.setdefault("GPU_MAX_HW_QUEUES", "16")    # before HIP initialises; see fie_amd.py
import sys
import time

from PIL import Image

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))


def load_mapping_file(mapping_path):
    with open(mapping_path, "r") as fh:
        return json.load(fh)


def safe_join(base_dir, user_path):
    """Join `user_path` under `base_dir`; absolute paths and `..` escapes raise ValueError (reference :25-41,
    including its string-prefix containment check)."""
    rel = os.path.normpath(user_path)
    if os.path.isabs(rel) or rel.startswith(".."):
        raise ValueError(f"Invalid path: {rel}")
    root = os.path.abspath(base_dir)
    joined = os.path.abspath(os.path.join(base_dir, rel))
    if not joined.startswith(root):
        raise ValueError(f"Path traversal detected: {rel}")
    return joined


def build_parser():
    p = argparse.ArgumentParser(description="Batch image editing on PIE-Bench")
    a = p.add_argument
    a("--mapping_file", type=str, default="data/PIE-Bench_v1/mapping_file.json", help="Path to PIE-Bench mapping file")
    a("--source_dir", type=str, default="data/PIE-Bench_v1/annotation_images", help="Directory containing source images")
    a("--output_dir", type=str, default="outputs", help="Output directory")
    a("--model", type=str, default="sdxl", choices=["sdxl", "ssd-1b"],
      help="Model to use: sdxl (full quality, ~6GB) or ssd-1b (faster, ~4GB)")
    a("--num_images", type=int, default=None, help="Number of images to process (default: all)")
    a("--editing_types", nargs="+", type=str, default=None, help="Filter by editing type IDs (e.g., 0 1 2)")
    a("--image_ids", nargs="+", type=str, default=None, help="Process specific image IDs")
    a("--steps", type=int, default=4, help="Number of inference steps")
    a("--guidance", type=float, default=1.5, help="Guidance scale")
    a("--control_scale", type=float, default=0.5, help="ControlNet conditioning scale")
    a("--canny_low", type=int, default=100, help="Canny low threshold")
    a("--canny_high", type=int, default=200, help="Canny high threshold")
    a("--seed", type=int, default=None, help="Random seed")
    a("--negative_prompt", type=str, default="", help="Negative prompt")
    a("--no_cpu_offload", action="store_true", help="Disable CPU offloading (faster but needs more VRAM)")
    a("--quality_mode", action="store_true", help="Maximum quality mode (fp32, full ControlNet) - A100 recommended")
    a("--full_precision", action="store_true", help="Use fp32 instead of fp16 (better quality, 2x VRAM)")
    a("--full_controlnet", action="store_true", help="Use full-size ControlNet instead of small variant")
    a("--skip_existing", action="store_true", help="Skip images that already have outputs")
    a("--save_comparisons", action="store_true", help="Save side-by-side comparison images")
    # additive
    a("--strength", type=float, default=None, help="[additive] img2img strength (default: FastEditor.edit's 0.80)")
    a("--weights_dir", type=str, default=None, help="[additive] local diffusers-layout weights directory")
    a("--results_json", type=str, default=None, help="[additive] write the merged per-image rows + summary here")
    a("--batch_size", type=int, default=1, help="[additive] images per device job (UNet / ControlNet / CLIP batched; the reference "
                                                  "is serial = 1); per-image time = job time / batch")
    a("--in_flight", type=int, default=1, help="[additive] edits in flight per GPU (worker threads, one hipGraph slot each); "
                                                 "per-image times then overlap, throughput is the summary's wall-clock rate")
    return p


def add_mask_args(p):
    """[additive] mask-restricted edits.  Kept apart from build_parser(), whose flag set is the reference's plus the additive ones above."""
    p.add_argument("--use_mask", action="store_true",
                   help="[additive] restrict each edit to the item's PIE-Bench `mask` (run-length code over the 512x512 image); the "
                        "background is pasted back from the source.  An item without a mask fails loudly")
    p.add_argument("--masked_content", type=str, default="original", choices=["original", "fill", "latent_noise", "latent_nothing"],
                   help="[additive] with --use_mask: what the model starts from inside the mask -- 'original' the source, 'fill' a smooth continuation "
                        "of the surroundings (object removal), 'latent_noise' pure noise, 'latent_nothing' the zero latent plus noise; the three new "
                        "modes also clear the edge map inside the mask")
    return p


def add_blend_args(p):
    """[additive] the one-sided multi-band paste-back.  Kept apart from build_parser() for the same reason as add_mask_args."""
    p.add_argument("--blend", type=str, default="alpha", choices=["alpha", "multiband"],
                   help="[additive] with --use_mask: how the edited region meets the source -- 'alpha' the paste-back as ever, 'multiband' a one-sided "
                        "multi-band blend: the edit keeps its detail, its brightness / colour difference to the source fades out towards the seam, "
                        "and outside the mask the output stays the source's bytes")
    p.add_argument("--blend_levels", type=int, default=4, choices=range(1, 7), metavar="N",
                   help="[additive] with --blend multiband: pyramid levels, 1..6; the difference fades over about 2^N pixels")
    return p


def add_grow_args(p):
    """[additive] growing / shrinking the mask.  Kept apart from build_parser() for the same reason as add_mask_args."""
    p.add_argument("--mask_grow", type=int, default=0, choices=range(-64, 65), metavar="N",
                   help="[additive] with --use_mask: grow (N > 0) or shrink (N < 0) each mask by an exact disk of N pixels of the mask (the 512x512 "
                        "benchmark image), -64..64, before anything else reads it.  PIE-Bench's decoder sets the mask's 1-pixel frame, so a grown "
                        "benchmark mask has an N-pixel frame")
    return p


def add_levels_args(p):
    """[additive] soft masks.  Kept apart from build_parser() for the same reason as add_mask_args."""
    p.add_argument("--mask_mode", type=str, default="binary", choices=["binary", "levels"],
                   help="[additive] with --use_mask: 'levels' reads each mask's greys as a per-pixel strength (255 edited as white, lower levels "
                        "released into the edit for the last steps only, 0 never); not with --mask_ramp or --mask_grow")
    p.add_argument("--mask_ramp", type=int, default=0, choices=range(0, 65), metavar="N",
                   help="[additive] with --use_mask: a soft mask from each binary mask's outline: the strength ramps up over N pixels of the mask "
                        "(the 512x512 benchmark image) inward from its outline, 0..64; --mask_grow N in front moves the ramp outward")
    return p


def outpaint_arg(text):
    """argparse type of --outpaint: 'L,T,R,B' -> (left, top, right, bottom) (fie_amd/mask.py: parse_outpaint)."""
    import fie_amd  # noqa: F401
    from fie_amd import mask as hmask
    try:
        return hmask.parse_outpaint(text)
    except ValueError as e:
        raise argparse.ArgumentTypeError(str(e)) from None


def add_outpaint_args(p):
    """[additive] outpainting.  Kept apart from build_parser() for the same reason as add_mask_args."""
    p.add_argument("--outpaint", type=outpaint_arg, default=None, metavar="L,T,R,B",
                   help="[additive] outpainting, for every image: make it larger by L, T, R, B pixels (left, top, right, bottom; each 0..4096, not "
                        "all 0) and let the model invent the new border.  The border is the mask: with --use_mask the item's mask is carried into "
                        "it, without it the border alone is edited, and --mask_grow, --masked_content, --blend and --region mask work without "
                        "--use_mask")
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
    """[additive] tiled edits.  Kept apart from build_parser() for the same reason as add_mask_args."""
    p.add_argument("--tiles", type=tiles_arg, default=None, metavar="{auto,WxH}",
                   help="[additive] tiled edits, for images above 1024^2 pixels: cover each image with overlapping tiles of one edit size ('auto': "
                        "per axis the smallest legal size that still overlaps by --tile_overlap; WxH: multiples of 64, 512..2048, at most 1024^2 "
                        "pixels), edit every tile at its native size and crossfade the results on the device into one image of the source's size.  "
                        "Not with --resolution, --region mask, --outpaint")
    p.add_argument("--tile_overlap", type=int, default=128, choices=range(0, 257), metavar="N",
                   help="[additive] with --tiles: pixels neighbouring tiles share at least, 0..256")
    p.add_argument("--tile_batch", type=int, default=4, choices=range(1, 17), metavar="N",
                   help="[additive] with --tiles: tiles per device job, 1..16")
    return p


def tile_kwargs(args):
    """The --tiles / --tile_overlap / --tile_batch flags (absent on a parser without add_tile_args) -> edit()'s keyword arguments."""
    if getattr(args, "tiles", None) is None:
        return {}
    for flag, off in (("resolution", "square"), ("region", "none"), ("outpaint", None)):
        if getattr(args, flag, off) != off:
            raise ValueError(f"--tiles with --{flag}: the tile size is the edit size and the output is the source's size")
    return dict(tiles=args.tiles, tile_overlap=getattr(args, "tile_overlap", 128), tile_batch=getattr(args, "tile_batch", 4))


def add_resolution_args(p):
    """[additive] aspect-ratio edits.  Kept apart from build_parser() for the same reason as add_mask_args."""
    p.add_argument("--resolution", type=str, default="square",
                   help="[additive] output size: 'square' (1024x1024, the reference's), 'auto' (the SDXL bucket nearest each source's aspect "
                        "ratio; a batch is split into one device job per size) or WxH (multiples of 64, 512..2048, at most 1024^2 pixels)")
    return p


def add_region_args(p):
    """[additive] full-resolution output and mask-region crops.  Kept apart from build_parser() for the same reason as
    add_mask_args."""
    p.add_argument("--output_size", type=str, default="edit", choices=["edit", "source"],
                   help="[additive] 'edit': outputs at the size the edit ran at (--resolution); 'source': outputs at each source image's own size, "
                        "composited there against the source's own pixels (with --use_mask)")
    p.add_argument("--region", type=str, default="none", choices=["none", "mask"],
                   help="[additive] 'mask' (needs --use_mask): edit only a crop around each item's mask at the model's native size and return the "
                        "source-size image with the crop composited in (implies --output_size source)")
    p.add_argument("--region_padding", type=int, default=32, help="[additive] with --region mask: pixels of context around the mask's bounding box")
    return p


def region_kwargs(args, have_mask):
    """The --output_size / --region / --region_padding flags (absent on a parser without add_region_args) -> edit()'s keyword arguments."""
    region = getattr(args, "region", "none")
    if region == "mask" and not have_mask:
        raise ValueError("--region mask needs --use_mask")
    kw = {}
    if region == "mask":
        kw.update(region="mask", region_padding=getattr(args, "region_padding", 32))
    elif getattr(args, "output_size", "edit") == "source":
        kw.update(output_size="source")
    return kw


def add_metrics_args(p):
    """[additive] inline metrics.  Kept apart from build_parser() for the same reason as add_mask_args."""
    p.add_argument("--metrics", action="store_true",
                   help="[additive] score every edit where it is made (SSIM / PSNR / MSE against the source at 512x512, on the device, plus the "
                        "background scores bg_* with --use_mask): per-image values in --results_json, mean / std in the summary.  They are of the "
                        "result BEFORE JPEG encoding, so they differ slightly from evaluate.py's on the saved file")
    return p


def add_clip_args(p):
    """[additive] CLIP score of every edit.  Kept apart from build_parser() for the same reason as add_mask_args."""
    p.add_argument("--clip_score_dir", type=str, default=None,
                   help="[additive] with --metrics: a local transformers CLIPModel directory (config.json, model.safetensors, vocab.json, merges.txt; "
                        "openai/clip-vit-base-patch16 is the reference's); adds clip_score (and clip_score_edited with --use_mask) to every row.  "
                        "Default: FIE_CLIP_SCORE_DIR, else <weights_dir>/clip_score when it exists")
    return p


def add_dino_args(p):
    """[additive] DINO structure distance of every edit.  Kept apart from build_parser() for the same reason as add_mask_args."""
    p.add_argument("--dino_dir", type=str, default=None,
                   help="[additive] with --metrics: a local transformers ViTModel directory (config.json, model.safetensors; facebook/dino-vitb8 is the "
                        "reference's); adds dino_distance to every row (None for a source that is not square).  Default: FIE_DINO_DIR, else "
                        "<weights_dir>/dino when it exists")
    return p


def add_lpips_args(p):
    """[additive] LPIPS of every edit.  Kept apart from build_parser() for the same reason as add_mask_args."""
    p.add_argument("--lpips_dir", type=str, default=None,
                   help="[additive] with --metrics: a local directory with the LPIPS SqueezeNet weights (model.safetensors, or torchvision's "
                        "squeezenet1_1*.pth beside the lpips package's squeeze.pth); adds lpips (and bg_lpips with --use_mask) to every row.  "
                        "Default: FIE_LPIPS_DIR, else <weights_dir>/lpips when it exists")
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
    """[additive] strength sweeps.  Kept apart from build_parser() for the same reason as add_mask_args."""
    p.add_argument("--auto_strength", type=str, default=None, choices=["clip_score", "strongest"],
                   help="[additive] choose each image's strength on the device: every distinct step count of --strengths is edited in ONE device job "
                        "and scored there; 'strongest' keeps the strongest edit whose SSIM against the source (the background's with --use_mask) stays "
                        "at or above --min_ssim, 'clip_score' the edit with the best CLIP score (needs --clip_score_dir; among those that pass "
                        "--min_ssim when given).  Only the chosen image leaves the device; the chosen strength and step count go into --results_json.  "
                        "Not with --batch_size > 1, --tiles, --region mask; --strength is ignored")
    p.add_argument("--min_ssim", type=float, default=None, help="[additive] with --auto_strength: the SSIM every candidate must keep, -1..1")
    p.add_argument("--strengths", type=strengths_arg, default="all", metavar="{all,a,b,c}",
                   help="[additive] with --auto_strength: the strengths to try, 'all' (one per step count 1..--steps) or comma-separated numbers")
    return p


def sweep_kwargs(args):
    """The --auto_strength / --min_ssim / --strengths flags (absent on a parser without add_sweep_args) -> edit_sweep()'s keyword arguments, or {}."""
    select = getattr(args, "auto_strength", None)
    min_ssim = getattr(args, "min_ssim", None)
    if select is None:
        if min_ssim is not None:
            raise ValueError("--min_ssim needs --auto_strength")
        return {}
    if max(1, getattr(args, "batch_size", 1)) > 1:
        raise ValueError("--auto_strength with --batch_size > 1: a sweep is one device job per image")
    if getattr(args, "tiles", None) is not None:
        raise ValueError("--auto_strength with --tiles: a sweep runs as one device job")
    if getattr(args, "region", "none") == "mask":
        raise ValueError("--auto_strength with --region mask: a sweep runs on the whole image")
    if select == "strongest" and min_ssim is None:
        raise ValueError("--auto_strength strongest needs --min_ssim")
    if min_ssim is not None and not -1.0 <= min_ssim <= 1.0:
        raise ValueError(f"--min_ssim {min_ssim}: a number in -1..1")
    kw = dict(select=select, strengths=getattr(args, "strengths", "all"))
    if min_ssim is not None:
        kw["min_ssim"] = min_ssim
    return kw


def full_parser():
    """The parser main() reads: build_parser() and every additive group."""
    return add_sweep_args(add_tile_args(add_lpips_args(add_dino_args(add_clip_args(add_metrics_args(add_region_args(add_resolution_args(add_outpaint_args(
        add_levels_args(add_grow_args(add_blend_args(add_mask_args(build_parser())))))))))))))


METRIC_KEYS = ("ssim", "psnr", "mse", "bg_ssim", "bg_psnr", "bg_mse", "clip_score", "clip_score_edited", "dino_distance", "lpips", "bg_lpips")


def select_entries(mapping, args, say=print):
    """Reference :115-140: explicit ids win; else filter by type, then truncate to --num_images."""
    if args.image_ids:
        say("\n[2/3] Filtering by image IDs...")
        chosen = [(i, mapping[i]) for i in args.image_ids if i in mapping]
        say(f"      Selected {len(chosen)} images by ID")
        return chosen
    if args.editing_types:
        say(f"\n[2/3] Filtering by editing types: {args.editing_types}")
        chosen = [(i, e) for i, e in mapping.items() if e.get("editing_type_id") in args.editing_types]
        say(f"      Selected {len(chosen)} images by type")
    else:
        chosen = list(mapping.items())
        say(f"\n[2/3] Processing all images: {len(chosen)}")
    if args.num_images and args.num_images < len(chosen):
        chosen = chosen[: args.num_images]
        say(f"      Limited to first {args.num_images} images")
    return chosen


def save_comparison(path, source_img, edited_img, model, prompt):
    import matplotlib
    matplotlib.use("Agg")
    import matplotlib.pyplot as plt
    os.makedirs(os.path.dirname(path), exist_ok=True)
    fig, axes = plt.subplots(1, 2, figsize=(12, 6))
    axes[0].imshow(source_img)
    axes[0].set_title("Source Image")
    axes[1].imshow(edited_img)
    title = f'"{prompt[:60]}..."' if len(prompt) > 60 else f'"{prompt}"'
    axes[1].set_title(f"Edited ({model.upper()})\n{title}")
    for ax in axes:
        ax.axis("off")
    plt.tight_layout()
    plt.savefig(path, dpi=150, bbox_inches="tight")
    plt.close(fig)


def process_shard(editor, entries, args, edited_dir, comparisons_dir, progress=None):
    """The per-image loop (reference :176-261) over this rank's (index, image_id, entry) triples; with --in_flight > 1 the
    entries are dealt to worker threads (one graph slot each) and the per-worker results are merged."""
    n = max(1, getattr(args, "in_flight", 1))
    if n == 1:
        return _process_entries(editor, entries, args, edited_dir, comparisons_dir, progress)
    from concurrent.futures import ThreadPoolExecutor
    editor.set_in_flight(n)
    if hasattr(editor, "calibrate_in_flight"):        # untimed set-up: pick slot streams on which the n edits really overlap
        for _, _, entry in entries:
            try:
                probe = Image.open(safe_join(args.source_dir, entry["image_path"])).convert("RGB")
                extra = {} if args.strength is None else {"strength": args.strength}
                editor.calibrate_in_flight(probe, entry.get("editing_prompt") or "calibration", num_inference_steps=args.steps,
                                           guidance_scale=args.guidance, controlnet_conditioning_scale=args.control_scale,
                                           seed=args.seed, **extra)
                break
            except (OSError, ValueError, KeyError):
                continue

    def work(slot):
        editor.worker_slot(slot)
        return _process_entries(editor, entries[slot::n], args, edited_dir, comparisons_dir, progress if slot == 0 else None)

    with ThreadPoolExecutor(max_workers=n) as pool:
        parts = list(pool.map(work, range(n)))
    res = dict(processed=0, skipped=0, failed=0, total_time=0.0, rows=[])
    for part in parts:
        for k in ("processed", "skipped", "failed", "total_time"):
            res[k] += part[k]
        res["rows"] += part["rows"]
    res["rows"].sort(key=lambda r: r["index"])
    return res


def _process_entries(editor, entries, args, edited_dir, comparisons_dir, progress=None):
    import fie_amd  # noqa: F401
    from fie_amd import mask as hmask
    res = dict(processed=0, skipped=0, failed=0, total_time=0.0, rows=[])
    extra = {} if args.strength is None else {"strength": args.strength}
    bs = max(1, getattr(args, "batch_size", 1))
    use_mask = getattr(args, "use_mask", False)
    resolution = getattr(args, "resolution", "square")
    if resolution != "square":
        extra = dict(extra, resolution=resolution)
    with_metrics = getattr(args, "metrics", False)
    if with_metrics:
        extra = dict(extra, metrics=True)
    outpaint = getattr(args, "outpaint", None)
    masked = use_mask or outpaint is not None      # --outpaint: the new border is a mask
    if outpaint is not None:
        extra = dict(extra, outpaint=tuple(outpaint))
    extra = dict(extra, **region_kwargs(args, masked), **tile_kwargs(args), **hmask.cli_keywords(args, masked, "--use_mask"))
    picked = getattr(editor, "canny_density", None) is not None     # an edge-budget Canny: every row then says which thresholds its image got
    sweep = sweep_kwargs(args)                     # --auto_strength: one edit_sweep() per image in place of edit()
    pending = []                                   # (index, image_id, rel, output_path, source_img, prompt, mask) awaiting one device job

    def flush():
        if not pending:
            return
        kw = dict(num_inference_steps=args.steps, guidance_scale=args.guidance, controlnet_conditioning_scale=args.control_scale,
                  canny_low_threshold=args.canny_low, canny_high_threshold=args.canny_high, seed=args.seed, **extra)
        try:
            t0 = time.time()
            if sweep:
                mkw = dict(mask=pending[0][6]) if use_mask else {}
                out, info = editor.edit_sweep(image=pending[0][4], prompt=pending[0][5], negative_prompt=args.negative_prompt,
                                              **{k: v for k, v in kw.items() if k not in ("strength", "metrics")}, **mkw, **sweep)
                score = dict(chosen_strength=info["strength"][0], chosen_steps=info["steps"],
                             **({k: info[k] for k in METRIC_KEYS if k in info} if with_metrics else {}))
                edited = ([out], [score])
            elif bs == 1:
                mkw = dict(mask=pending[0][6]) if use_mask else {}
                edited = editor.edit(image=pending[0][4], prompt=pending[0][5], negative_prompt=args.negative_prompt, **kw, **mkw)
                edited = ([edited[0]], [edited[1]]) if with_metrics else [edited]
            else:
                mkw = dict(masks=[p[6] for p in pending]) if use_mask else {}
                edited = editor.edit_batch(images=[p[4] for p in pending], prompts=[p[5] for p in pending],
                                           negative_prompts=[args.negative_prompt] * len(pending), **kw, **mkw)
            dt = (time.time() - t0) / len(pending)
            edited, scores = edited if with_metrics or sweep else (edited, [{}] * len(pending))
            if picked:
                scores = [dict(s, canny_low=p[0], canny_high=p[1]) if p is not None else s for s, p in zip(scores, editor.last_canny_thresholds())]
            for (index, image_id, rel, output_path, source_img, prompt, _), out, score in zip(pending, edited, scores):
                res["total_time"] += dt
                out.save(output_path)
                res["processed"] += 1
                res["rows"].append(dict(index=index, image_id=image_id, image_path=rel, elapsed_s=dt, **score))
                if args.save_comparisons:
                    save_comparison(os.path.join(comparisons_dir, rel.replace(".jpg", ".png")), source_img, out, args.model, prompt)
                if res["processed"] % 10 == 0:
                    editor.clear_memory()
        except Exception as e:  # per-image isolation, as the reference does (a failing batch fails its images)
            ids = ", ".join(str(p[1]) for p in pending)
            print(f"\n      Error processing {ids} ({type(e).__name__}): {e}")
            res["failed"] += len(pending)
        pending.clear()

    for index, image_id, entry in (progress(entries) if progress else entries):
        try:
            rel = entry["image_path"]
            source_path = safe_join(args.source_dir, rel)
            output_path = os.path.join(edited_dir, rel)
            if args.skip_existing and os.path.exists(output_path):
                res["skipped"] += 1
                continue
            if not os.path.exists(source_path):
                res["failed"] += 1
                continue
            os.makedirs(os.path.dirname(output_path), exist_ok=True)
            source_img = Image.open(source_path).convert("RGB")
            prompt = entry.get("editing_prompt", "")
            if not prompt:
                res["failed"] += 1
                continue
            mask = None
            if use_mask:
                if not entry.get("mask"):
                    print(f"\n      Error processing {image_id}: --use_mask but the entry has no `mask`")
                    res["failed"] += 1
                    continue
                mask = hmask.rle_decode(entry["mask"], (source_img.height, source_img.width))
            pending.append((index, image_id, rel, output_path, source_img, prompt, mask))
            if len(pending) == bs:
                flush()
        except FileNotFoundError as e:
            print(f"\n      File not found for {image_id}: {e}")
            res["failed"] += 1
        except ValueError as e:
            print(f"\n      Invalid path for {image_id}: {e}")
            res["failed"] += 1
    flush()
    return res


def print_summary(tot, args, edited_dir, comparisons_dir, world, wall):
    bar = "=" * 60
    print(f"\n{bar}\nBATCH PROCESSING SUMMARY\n{bar}")
    print(f"\nProcessed:  {tot['processed']} images")
    print(f"Skipped:    {tot['skipped']} images")
    print(f"Failed:     {tot['failed']} images")
    if tot["processed"] > 0:
        print(f"\nAverage time per image: {tot['total_time'] / tot['processed']:.2f}s")
        print(f"Total time: {tot['total_time']:.2f}s ({tot['total_time'] / 60:.1f} minutes)")
        print(f"Throughput: {tot['processed'] / wall:.2f} images/sec wall-clock on {world} GPU(s)")
        if getattr(args, "auto_strength", None):
            chosen = [r["chosen_steps"] for r in tot.get("rows", []) if r.get("chosen_steps") is not None]
            print(f"\nChosen step counts (--auto_strength {args.auto_strength}, of {args.steps} steps):")
            for m in sorted(set(chosen), reverse=True):
                print(f"  {m} steps: {chosen.count(m)} images")
        if getattr(args, "metrics", False):
            import numpy as np
            print("\nMetrics of the edits (512x512, before JPEG encoding):")
            for k in METRIC_KEYS:
                vals = [r[k] for r in tot.get("rows", []) if r.get(k) is not None]
                finite = [v for v in vals if np.isfinite(v)]          # an unchanged image has PSNR inf
                if finite:
                    note = f"  ({len(vals) - len(finite)} infinite not counted)" if len(finite) < len(vals) else ""
                    print(f"  {k + ':':<9} {np.mean(finite):.6f} ± {np.std(finite):.6f}{note}")
    else:
        print("\n⚠ WARNING: No images were successfully processed!")
        print("  Check that:")
        print(f"    - Source images exist at: {args.source_dir}")
        print(f"    - Mapping file is correct: {args.mapping_file}")
        print("    - Selected filters match available images")
    print("\nOutputs saved to:")
    print(f"  - Edited images: {edited_dir}")
    if args.save_comparisons:
        print(f"  - Comparisons: {comparisons_dir}")
    print(bar)


def main(argv=None):
    parser = full_parser()
    args = parser.parse_args(argv)
    import fie_amd  # noqa: F401
    from fie_amd import buckets, mask as hmask
    masked = args.use_mask or args.outpaint is not None                # --outpaint: the new border is a mask
    try:
        tile_kwargs(args)
        sweep_kwargs(args)
        if args.region == "mask" and not masked:
            raise ValueError("--region mask needs --use_mask")
        hmask.cli_keywords(args, masked, "--use_mask")
    except ValueError as e:
        parser.error(str(e))
    if args.resolution != "square":
        args.resolution = buckets.parse(args.resolution)
    from fie_amd import dist as fdist
    rank, local, world = fdist.init()
    say = print if rank == 0 else (lambda *a, **k: None)
    if args.quality_mode:
        args.full_precision = args.full_controlnet = args.no_cpu_offload = True
        say("[Quality Mode] Enabled: fp32 + full ControlNet + no CPU offload")
    model_suffix = f"{args.model}_{'fp32' if args.full_precision else 'fp16'}"
    edited_dir = os.path.join(args.output_dir, "batch", "edited", model_suffix)
    comparisons_dir = os.path.join(args.output_dir, "batch", "comparisons", model_suffix)
    os.makedirs(edited_dir, exist_ok=True)
    if args.save_comparisons:
        os.makedirs(comparisons_dir, exist_ok=True)

    say(f"\n[1/3] Loading mapping file from {args.mapping_file}")
    mapping = load_mapping_file(args.mapping_file)
    say(f"      Total entries in mapping file: {len(mapping)}")
    selected = select_entries(mapping, args, say)
    if not selected:
        say("\n      No images selected. Exiting.")
        return
    mine = fdist.shard([(i, k, e) for i, (k, e) in enumerate(selected)], rank, world)

    say(f"\n[3/3] Initializing FastEditor ({model_suffix})...")
    clip_dir = dino_dir = lpips_dir = None
    if args.auto_strength == "clip_score" and not args.metrics:     # the selector reads the CLIP rows: the model is needed without --metrics too
        from fie_amd import clip_score as hclip
        clip_dir = hclip.resolve_dir(args.clip_score_dir)
        if clip_dir is None and args.weights_dir and os.path.isdir(os.path.join(args.weights_dir, "clip_score")):
            clip_dir = os.path.join(args.weights_dir, "clip_score")
    if args.metrics:
        from fie_amd import lpips as hlpips
        lpips_dir = hlpips.resolve_dir(args.lpips_dir)
        if lpips_dir is None and args.weights_dir and os.path.isdir(os.path.join(args.weights_dir, "lpips")):
            lpips_dir = os.path.join(args.weights_dir, "lpips")
        from fie_amd import dino as hdino
        dino_dir = hdino.resolve_dir(args.dino_dir)
        if dino_dir is None and args.weights_dir and os.path.isdir(os.path.join(args.weights_dir, "dino")):
            dino_dir = os.path.join(args.weights_dir, "dino")
        from fie_amd import clip_score as hclip
        clip_dir = hclip.resolve_dir(args.clip_score_dir)
        if clip_dir is None and args.weights_dir and os.path.isdir(os.path.join(args.weights_dir, "clip_score")):
            clip_dir = os.path.join(args.weights_dir, "clip_score")
    if args.auto_strength == "clip_score" and clip_dir is None:
        parser.error("--auto_strength clip_score needs a CLIP model: --clip_score_dir (or FIE_CLIP_SCORE_DIR, or <weights_dir>/clip_score)")
    from src.pipeline import FastEditor
    import contextlib
    import io
    with contextlib.redirect_stdout(sys.stdout if rank == 0 else io.StringIO()):
        import torch
        editor = FastEditor(model_name=args.model, device="cuda" if world == 1 else f"cuda:{local % max(torch.cuda.device_count(), 1)}",
                            enable_cpu_offload=not args.no_cpu_offload, use_full_precision=args.full_precision,
                            use_full_controlnet=args.full_controlnet, weights_dir=args.weights_dir,
                            clip_score_dir=clip_dir, dino_dir=dino_dir, lpips_dir=lpips_dir)
    if hasattr(editor, "pipe"):
        editor.pipe.set_progress_bar_config(disable=True)
    mem = editor.get_memory_usage()
    say(f"      GPU Memory: {mem['allocated_gb']:.2f}GB allocated, {mem['reserved_gb']:.2f}GB reserved")
    say(f"\n      Processing {len(selected)} images on {world} GPU(s)...")
    say(f"      Parameters: steps={args.steps}, guidance={args.guidance}, control_scale={args.control_scale}")
    if args.negative_prompt:
        say(f"      Negative prompt: {args.negative_prompt}")
    if getattr(editor, "canny_density", None) is None:
        say(f"      Canny thresholds: low={args.canny_low}, high={args.canny_high}")
    else:
        say(f"      Canny thresholds: picked per image at density {editor.canny_density:g} (FIE_CANNY_DENSITY), low / high = "
            f"{min(args.canny_low, args.canny_high)} / {max(args.canny_low, args.canny_high)} (each image's pair: --results_json)")
    if getattr(editor, "prompt_emphasis", None) is not None:
        say(f"      Prompt emphasis: the [...] marks of the prompts weigh {editor.prompt_emphasis:g} (FIE_PROMPT_EMPHASIS)")
    if getattr(editor, "control_weights", None) is not None:
        say(f"      Control weights: {editor.control_weights} (FIE_CONTROL_WEIGHTS)")

    progress = None
    if rank == 0:
        try:
            from tqdm import tqdm
            progress = lambda it: tqdm(it, desc="Editing")
        except ImportError:
            pass
    fdist.barrier()
    t0 = time.time()
    res = process_shard(editor, mine, args, edited_dir, comparisons_dir, progress)
    fdist.barrier()
    wall = time.time() - t0
    gathered = fdist.gather_results(res)
    if rank == 0:
        tot = fdist.merge_results(gathered)
        print_summary(tot, args, edited_dir, comparisons_dir, world, wall)
        if args.results_json:
            with open(args.results_json, "w") as fh:
                json.dump(dict(world_size=world, wall_s=wall, **tot), fh, indent=1)
        print("\nDone! Next steps:")
        print(f"  1. Review outputs: ls {edited_dir}")
        print(f"  2. Run evaluation: python evaluate.py --outputs_dir {edited_dir}")
    editor.clear_memory()


if __name__ == "__main__":
    main()
