#!/usr/bin/env python3
"""Evaluation harness -- drop-in for /root/reference/evaluate.py (same flags, same `metrics.csv` columns and
`summary.json` layout, reference :193-271), on the metrics this build restates (`src/metrics.py`: SSIM, PSNR, MSE).
LPIPS / CLIP score / DINO distance need checkpoints: without a local model directory (`--lpips_dir`, `--clip_score_dir`, `--dino_dir`) their cells
are empty in the CSV and `null` in the JSON.
Additive: `--use_mask` appends the background-preservation columns `bg_ssim, bg_psnr, bg_mse` (each item's PIE-Bench `mask`; both images
zeroed inside the edited region first) to the CSV and to `summary.json`, and `bg_lpips` behind them with an LPIPS directory.
Pairs are scored in chunks: on a GPU one launch per chunk.

Under `torch.distributed.run` the mapping entries are sharded image-parallel over the ranks (fie_amd.dist) and rank 0
writes the merged files -- the "gather of metrics" of SURVEY.md 8e.

    python evaluate.py --outputs_dir outputs/batch/edited/ssd-1b_fp16
"""
import argparse
import csv
import json
import os

os.environ.setdefault("GPU_MAX_HW_QUEUES", "16")    # before HIP initialises; see fie_amd.py
import sys

import numpy as np
from PIL import Image

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

METRICS = ("ssim", "lpips", "clip_score", "psnr", "mse", "dino_distance")
FIELDS = ["image_id", "image_path", "editing_type_id", "editing_prompt", *METRICS]
BG_METRICS = ("bg_ssim", "bg_psnr", "bg_mse")
BG_LPIPS_METRICS = ("bg_lpips",)                 # only with --use_mask AND an LPIPS weight directory (--lpips_dir)
EDITED_METRICS = ("clip_score_edited",)          # only with --use_mask AND a CLIP model directory (--clip_score_dir)
CHUNK = 16                      # pairs per calculate_pairs() call (one device launch and one synchronisation each)
KNOWN_SUFFIXES = ("sdxl_fp32", "sdxl_fp16", "ssd-1b_fp32", "ssd-1b_fp16")


def build_parser():
    p = argparse.ArgumentParser(description="Evaluate edited images")
    p.add_argument("--mapping_file", type=str, default="data/PIE-Bench_v1/mapping_file.json", help="Path to PIE-Bench mapping file")
    p.add_argument("--source_dir", type=str, default="data/PIE-Bench_v1/annotation_images", help="Directory containing source images")
    p.add_argument("--outputs_dir", type=str, required=True,
                   help="Directory containing edited images (e.g., outputs/batch/edited/sdxl_fp32)")
    p.add_argument("--results_file", type=str, default=None,
                   help="Output CSV file for metrics (auto-detected from outputs_dir if not specified)")
    p.add_argument("--summary_file", type=str, default=None,
                   help="Output JSON file for summary statistics (auto-detected from outputs_dir if not specified)")
    p.add_argument("--device", type=str, default="cuda", help="Device to use for metrics computation")
    return p


def add_mask_args(p):
    """[additive] background-preservation metrics.  Kept apart from build_parser(), whose flag set is the reference's."""
    p.add_argument("--use_mask", action="store_true",
                   help="[additive] also score the background (the region outside each item's PIE-Bench `mask`, a run-length code over the "
                        "512x512 image): columns bg_ssim, bg_psnr, bg_mse.  An item without a mask is skipped loudly")
    return p


def add_clip_args(p):
    """[additive] CLIP score.  Kept apart from build_parser() for the same reason as add_mask_args."""
    p.add_argument("--clip_score_dir", type=str, default=None,
                   help="[additive] a local transformers CLIPModel directory (openai/clip-vit-base-patch16 is the reference's): fills the clip_score "
                        "column (and, with --use_mask, adds clip_score_edited beside bg_*).  Default: FIE_CLIP_SCORE_DIR, else "
                        "<FIE_WEIGHTS_DIR>/clip_score when it exists; without one the column stays empty")
    return p


def add_dino_args(p):
    """[additive] DINO structure distance.  Kept apart from build_parser() for the same reason as add_mask_args."""
    p.add_argument("--dino_dir", type=str, default=None,
                   help="[additive] a local transformers ViTModel directory (facebook/dino-vitb8 is the reference's): fills the dino_distance "
                        "column for square pairs.  Default: FIE_DINO_DIR, else <FIE_WEIGHTS_DIR>/dino when it exists; without one the column stays empty")
    return p


def add_lpips_args(p):
    """[additive] LPIPS.  Kept apart from build_parser() for the same reason as add_mask_args."""
    p.add_argument("--lpips_dir", type=str, default=None,
                   help="[additive] a local directory with the LPIPS SqueezeNet weights (model.safetensors, or torchvision's squeezenet1_1*.pth beside "
                        "the lpips package's squeeze.pth): fills the lpips column (and, with --use_mask, adds bg_lpips behind bg_mse).  Default: "
                        "FIE_LPIPS_DIR, else <FIE_WEIGHTS_DIR>/lpips when it exists; without one the column stays empty")
    return p


def extra_columns(args, calc):
    """The columns behind the reference's: bg_* with --use_mask, bg_lpips / clip_score_edited when the calculator also has that model."""
    if not getattr(args, "use_mask", False):
        return ()
    return (BG_METRICS + (BG_LPIPS_METRICS if getattr(calc, "_lpips", None) is not None else ())
            + (EDITED_METRICS if getattr(calc, "_clip", None) is not None else ()))


def default_paths(args):
    tail = os.path.basename(args.outputs_dir.rstrip("/"))
    sub = f"{tail}/" if args.outputs_dir.rstrip("/").endswith(KNOWN_SUFFIXES) else ""
    args.results_file = args.results_file or f"results/{sub}metrics.csv"
    args.summary_file = args.summary_file or f"results/{sub}summary.json"
    for path in (args.results_file, args.summary_file):
        os.makedirs(os.path.dirname(path) or ".", exist_ok=True)


def _stats(values, with_median):
    vals = [v for v in values if v is not None]
    if not vals:
        return {"mean": None, "std": None, **({"median": None} if with_median else {})}
    out = {"mean": float(np.mean(vals)), "std": float(np.std(vals))}
    if with_median:
        out["median"] = float(np.median(vals))
    return out


def summarize(rows, metrics=METRICS):
    """reference :201-268: overall mean/std/median per metric + per-category mean/std and count."""
    summary = {"total_images": len(rows), "overall": {m: _stats([r[m] for r in rows], True) for m in metrics}, "by_category": {}}
    cats = {}
    for r in rows:
        cats.setdefault(r["editing_type_id"], []).append(r)
    for cat, rs in cats.items():
        summary["by_category"][cat] = {"count": len(rs), **{m: _stats([r[m] for r in rs], False) for m in metrics}}
    return summary


def evaluate_entries(entries, args, calc, progress=None):
    rows, skipped = [], 0
    use_mask = getattr(args, "use_mask", False)
    with_edited = use_mask and getattr(calc, "_clip", None) is not None
    with_bg_lpips = use_mask and getattr(calc, "_lpips", None) is not None
    names = METRICS + extra_columns(args, calc)
    if use_mask:
        from fie_amd import mask as hmask
    pending = []                                   # (index, image_id, rel, entry, source, edited, mask) awaiting one calculate_pairs() call

    def flush():
        nonlocal skipped
        if not pending:
            return
        try:
            ms = calc.calculate_pairs([p[4] for p in pending], [p[5] for p in pending], [p[6] for p in pending] if use_mask else None)
        except Exception:       # per-image isolation (reference :179-182): score the chunk's pairs one by one, only the failing ones are skipped
            ms = []
            for p in pending:
                try:
                    ms.append(calc.calculate_pairs([p[4]], [p[5]], [p[6]] if use_mask else None)[0])
                except Exception as e:
                    print(f"\n      Error processing {p[1]}: {e}")
                    skipped += 1
                    ms.append(None)
        clips = [None] * len(pending)
        if getattr(calc, "_clip", None) is not None:      # the chunk's CLIP scores in one batched pass; a failure leaves the column empty
            try:
                clips = calc.calculate_clip_scores([p[5] for p in pending], [p[3].get("editing_prompt", "") for p in pending],
                                                   [p[6] for p in pending] if use_mask else None)
            except Exception as e:
                print(f"\n      Error computing CLIP scores: {e}")
        dinos = [None] * len(pending)
        if getattr(calc, "_dino", None) is not None:      # the chunk's structure distances, one batched pass per size; square pairs only
            sq = [i for i, p in enumerate(pending) if p[4].size[0] == p[4].size[1] and p[5].size[0] == p[5].size[1]]
            try:
                for i, d in zip(sq, calc.calculate_dino_distances([pending[i][4] for i in sq], [pending[i][5] for i in sq])):
                    dinos[i] = d
            except Exception as e:
                print(f"\n      Error computing DINO distances: {e}")
        lps = [None] * len(pending)
        if getattr(calc, "_lpips", None) is not None:     # the chunk's LPIPS (and background LPIPS) in one batched pass
            try:
                lps = calc.calculate_lpipses([p[4] for p in pending], [p[5] for p in pending], [p[6] for p in pending] if use_mask else None)
            except Exception as e:
                print(f"\n      Error computing LPIPS: {e}")
        for (index, image_id, rel, entry, a, b, _), m, cs, dd, lp in zip(pending, ms, clips, dinos, lps):
            if m is None:
                continue
            m = calc.with_unavailable(m, None, None, entry.get("editing_prompt", ""))
            m["dino_distance"] = dd
            if lp:
                m.update(lp)
            if with_bg_lpips:
                m.setdefault("bg_lpips", None)
            if cs:
                m.update(cs)
            if with_edited:
                m.setdefault("clip_score_edited", None)
            rows.append(dict(index=index, image_id=image_id, image_path=rel, editing_type_id=entry.get("editing_type_id", "unknown"),
                             editing_prompt=entry.get("editing_prompt", ""), **{k: m[k] for k in names}))
        pending.clear()

    for index, image_id, entry in (progress(entries) if progress else entries):
        rel = entry["image_path"]
        src, out = os.path.join(args.source_dir, rel), os.path.join(args.outputs_dir, rel)
        if not (os.path.exists(out) and os.path.exists(src)):
            skipped += 1
            continue
        try:
            mask = None
            if use_mask:
                if not entry.get("mask"):
                    raise ValueError("--use_mask but the entry has no `mask`")
                mask = hmask.rle_decode(entry["mask"])
            pending.append((index, image_id, rel, entry, Image.open(src).convert("RGB"), Image.open(out).convert("RGB"), mask))
        except Exception as e:  # per-image isolation (reference :179-182)
            print(f"\n      Error processing {image_id}: {e}")
            skipped += 1
        if len(pending) == CHUNK:
            flush()
    flush()
    return rows, skipped


def main(argv=None):
    args = add_lpips_args(add_dino_args(add_clip_args(add_mask_args(build_parser())))).parse_args(argv)
    import fie_amd  # noqa: F401
    from fie_amd import dist as fdist
    from src.metrics import MetricsCalculator
    rank, local, world = fdist.init()
    say = print if rank == 0 else (lambda *a, **k: None)
    default_paths(args)
    say(f"\n[1/4] Loading mapping file from {args.mapping_file}")
    with open(args.mapping_file) as fh:
        mapping = json.load(fh)
    say(f"      Total entries: {len(mapping)}")
    say(f"\n[2/4] Scanning outputs in {args.outputs_dir}")
    say(f"\n[3/4] Initializing metrics on {args.device}...")
    device = args.device if world == 1 or not args.device.startswith("cuda") else f"cuda:{local}"
    calc = MetricsCalculator(device=device, clip_dir=args.clip_score_dir, dino_dir=args.dino_dir, lpips_dir=args.lpips_dir)
    mine = fdist.shard([(i, k, e) for i, (k, e) in enumerate(mapping.items())], rank, world)
    progress = None
    if rank == 0:
        try:
            from tqdm import tqdm
            progress = lambda it: tqdm(it, desc="Evaluating")
        except ImportError:
            pass
    rows, skipped = evaluate_entries(mine, args, calc, progress)
    gathered = fdist.gather_results(dict(rows=rows, skipped=skipped))
    if rank != 0:
        return
    rows = sorted((r for g in gathered for r in g["rows"]), key=lambda r: r["index"])
    skipped = sum(g["skipped"] for g in gathered)
    print(f"\n      Processed: {len(rows)} images\n      Skipped:   {skipped} images")
    if not rows:
        print("\n      No images were processed. Exiting.")
        return
    print("\n[4/4] Saving results...")
    with open(args.results_file, "w", newline="") as fh:
        extra = extra_columns(args, calc)
        w = csv.DictWriter(fh, fieldnames=FIELDS + list(extra), extrasaction="ignore")
        w.writeheader()
        w.writerows([{k: ("" if v is None else v) for k, v in r.items()} for r in rows])
    print(f"      Saved detailed metrics to: {args.results_file}")
    summary = summarize(rows, METRICS + extra)
    with open(args.summary_file, "w") as fh:
        json.dump(summary, fh, indent=2)
    print(f"      Saved summary statistics to: {args.summary_file}")
    fmt = lambda s, spec: "unavailable offline" if s["mean"] is None else f"{format(s['mean'], spec)} ± {format(s['std'], spec)}"
    bar = "=" * 60
    print(f"\n{bar}\nEVALUATION SUMMARY\n{bar}\n\nTotal Images Evaluated: {len(rows)}\n\nOverall Metrics:")
    labels = (("ssim", "SSIM:      ", ".4f"), ("lpips", "LPIPS:     ", ".4f"), ("psnr", "PSNR:      ", ".2f"), ("mse", "MSE:       ", ".6f"),
              ("clip_score", "CLIP Score:", ".2f"), ("dino_distance", "DINO Dist.:", ".4f"))
    if args.use_mask:
        labels += (("bg_ssim", "Bg SSIM:   ", ".4f"), ("bg_psnr", "Bg PSNR:   ", ".2f"), ("bg_mse", "Bg MSE:    ", ".6f"))
    if "bg_lpips" in extra:
        labels += (("bg_lpips", "Bg LPIPS:  ", ".4f"),)
    if "clip_score_edited" in extra:
        labels += (("clip_score_edited", "CLIP edited:", ".2f"),)
    for k, label, spec in labels:
        print(f"  {label} {fmt(summary['overall'][k], spec)}")
    print("\nMetrics by Category:")
    for cat in sorted(summary["by_category"]):
        c = summary["by_category"][cat]
        print(f"\n  Category {cat} ({c['count']} images):")
        for k, label, spec in labels:
            print(f"    {label} {fmt(c[k], spec)}")
    print(f"\n{bar}\n\nDone!")
    calc.clear_memory()


if __name__ == "__main__":
    main()
