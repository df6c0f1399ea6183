#!/bin/bash
# Round-end evidence on ONE box (run from the repo root): rocprofv3 --kernel-trace --stats of a short bench run, the per-shape in-situ table,
# and the fp8 configuration beside fp16.  Outputs under OUTPUT_DIR (copy what is to be judged into profiles/).
OUT=${1:?usage: tools/round_end_evidence.sh OUTPUT_DIR}
cd "$(dirname "$0")/.." && export TMPDIR=/tmp && rm -rf "$OUT/r3s_prof" "$OUT/r3s_shape" && mkdir -p "$OUT"
timeout -k 10 300 rocprofv3 --kernel-trace --stats --output-format csv -d "$OUT/r3s_prof" -o runc -- python3 bench.py --full --steps 5 --warmup 2 --no-cpu-baseline --no-extras > "$OUT/r3s_prof_bench.json" 2> "$OUT/r3s_prof_bench.err"
python3 tools/rocprof_summary.py "$OUT/r3s_prof" "$OUT/r03_final_bench" > /dev/null; head -12 "$OUT/r03_final_bench_summary.md" | cut -c1-160
mkdir -p "$OUT/r3s_shape" && timeout -k 10 250 rocprofv3 --kernel-trace --output-format csv -d "$OUT/r3s_shape/runc" -- python3 tools/shape_profile.py run "$OUT/r3s_shape/oplog.txt" > "$OUT/r3s_shape_run.log" 2>&1
python3 tools/shape_profile.py report "$OUT/r3s_shape" "$OUT/r3s_shape/report.md" > /dev/null 2> "$OUT/r3s_report.err"; head -16 "$OUT/r3s_shape/report.md" | tail -9
timeout -k 10 300 python bench.py --full --weights f8e4m3 --no-cpu-baseline > "$OUT/r3s_bench_fp8.json" 2> "$OUT/r3s_bench_fp8.err"
timeout -k 10 300 python bench.py --full --no-cpu-baseline --no-extras > "$OUT/r3s_bench_f16.json" 2> "$OUT/r3s_bench_f16.err"
OUT="$OUT" python3 - <<'PY'
import json, os
for f in ("r3s_bench_fp8", "r3s_bench_f16"):
    d = json.loads(open(os.path.join(os.environ["OUT"], f + ".json")).read().strip().split("\n")[-1])
    print(f, d["value"], d["ms_per_step"], d["dtype"], d["roofline"]["unet_forward"]["ms"])
PY
