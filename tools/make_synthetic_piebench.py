#!/usr/bin/env python3
"""Write a PIE-Bench-SHAPED synthetic dataset: `mapping_file.json` + one 512x512 JPEG per item under
the 700 real relative paths, with the real prompts / editing-type ids from tests/golden/pie_bench_items.csv and seeded synthetic
pictures (low-frequency colour fields + filled shapes, so Canny(100,200) finds real edges).

    python tools/make_synthetic_piebench.py --out data/PIE-Bench_v1 [--num 700] [--with_masks]
    python -m torch.distributed.run --nproc-per-node 8 --master-addr 127.0.0.1 run_batch.py --model ssd-1b --no_cpu_offload --seed 42
"""
import argparse
import csv
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from bench import synth_item_image  # noqa: E402


def item_mask_box(i, size=512):
    """(x0, y0, x1, y1): the pixel box around the first filled circle synth_item_image(i) draws (its seeded draws replayed: four per
    colour channel, then the circle's centre and radius)."""
    import numpy as np
    rng = np.random.default_rng(i)
    for _ in range(12):
        rng.uniform()
    cx, cy, r = rng.uniform(0.1, 0.9), rng.uniform(0.1, 0.9), rng.uniform(0.04, 0.2)
    lo = lambda v: max(int(np.floor((v - r) * size)), 0)
    hi = lambda v: min(int(np.ceil((v + r) * size)), size)
    return lo(cx), lo(cy), hi(cx), hi(cy)


def item_mask_rle(i, size=512):
    """PIE-Bench `mask` field of item i (--with_masks): the run-length code (fie_amd/mask.py: rle_encode) of item_mask_box."""
    import numpy as np
    import fie_amd  # noqa: F401
    from fie_amd import mask as hmask
    x0, y0, x1, y1 = item_mask_box(i, size)
    m = np.zeros((size, size), np.uint8)
    m[y0:y1, x0:x1] = 1
    return hmask.rle_encode(m)


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="data/PIE-Bench_v1")
    ap.add_argument("--num", type=int, default=700)
    ap.add_argument("--with_masks", action="store_true", help="add a PIE-Bench `mask` (a box around one drawn shape) to every item")
    args = ap.parse_args(argv)
    with open(os.path.join(ROOT, "tests", "golden", "pie_bench_items.csv")) as f:
        items = list(csv.DictReader(f))[: args.num]
    mapping = {}
    for i, it in enumerate(items):
        path = os.path.join(args.out, "annotation_images", it["image_path"])
        os.makedirs(os.path.dirname(path), exist_ok=True)
        synth_item_image(i).save(path, quality=95)
        mapping[it["image_id"]] = {"image_path": it["image_path"], "editing_prompt": it["editing_prompt"],
                                   "editing_type_id": it["editing_type_id"]}
        if args.with_masks:
            mapping[it["image_id"]]["mask"] = item_mask_rle(i)
    with open(os.path.join(args.out, "mapping_file.json"), "w") as f:
        json.dump(mapping, f, indent=1)
    print(f"wrote {len(mapping)} items under {args.out}")


if __name__ == "__main__":
    main()
