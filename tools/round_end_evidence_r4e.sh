#!/bin/bash
# Third session of round 4, second evidence call on ONE box: whole-edit A/B of the thin-conv kernel, the GPU suite on the LIVE tuner,
# BASELINE config 3 (SDXL, 8 images per job) and config 5 (SDXL W8A8, calibrated) beside fp16.  Outputs under OUTPUT_DIR.
OUT=${1:?usage: tools/round_end_evidence_r4e.sh OUTPUT_DIR}
cd "$(dirname "$0")/.." && mkdir -p "$OUT"
FIE_AUTOTUNE=0 timeout -k 10 200 python tools/thin_conv_edit_ab.py > "$OUT/r4e_thin_edit_ab.log" 2>&1; tail -n 8 "$OUT/r4e_thin_edit_ab.log"
FIE_TUNE_LIVE=1 timeout -k 10 480 python -m pytest tests -x -q -m gpu > "$OUT/r4e_gpu_suite_live.log" 2>&1; tail -n 2 "$OUT/r4e_gpu_suite_live.log"
grep -q " passed" "$OUT/r4e_gpu_suite_live.log" && ! grep -q " failed" "$OUT/r4e_gpu_suite_live.log" && \
timeout -k 10 300 python bench.py --full --model sdxl --batch 8 --no-cpu-baseline > "$OUT/r4e_bench_sdxl_b8.json" 2> "$OUT/r4e_bench_sdxl_b8.err" && \
timeout -k 10 300 python bench.py --full --model sdxl --weights f8e4m3 --no-cpu-baseline --no-extras > "$OUT/r4e_bench_sdxl_fp8.json" 2> "$OUT/r4e_bench_sdxl_fp8.err" && \
OUT="$OUT" python3 - <<'PY'
import json, os
for f in ("r4e_bench_sdxl_b8", "r4e_bench_sdxl_fp8"):
    d = json.loads(open(os.path.join(os.environ["OUT"], f + ".json")).read().strip().split("\n")[-1])
    print(f, d["value"], d["ms_per_step"], d["dtype"], d.get("batched_images_per_sec"), d["roofline"]["unet_forward"]["ms"])
PY
