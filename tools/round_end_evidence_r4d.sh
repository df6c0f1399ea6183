OUT=${1:?usage: tools/round_end_evidence_r4d.sh OUTPUT_DIR}
cd "$(dirname "$0")/.." && export TMPDIR=/tmp && rm -rf "$OUT/r4d_prof" "$OUT/r4d_shape" && mkdir -p "$OUT"
timeout -k 10 480 python -m pytest tests -x -q -m gpu > "$OUT/r4d_gpu_suite.log" 2>&1; tail -n 3 "$OUT/r4d_gpu_suite.log"
grep -q " passed" "$OUT/r4d_gpu_suite.log" && ! grep -q " failed" "$OUT/r4d_gpu_suite.log" && \
timeout -k 10 300 python bench.py --full > "$OUT/r4d_bench.json" 2> "$OUT/r4d_bench.err" && tail -c 600 "$OUT/r4d_bench.json" && \
timeout -k 10 300 rocprofv3 --kernel-trace --stats --output-format csv -d "$OUT/r4d_prof" -o runc -- python3 bench.py --full --steps 5 --warmup 2 --no-cpu-baseline --no-extras > "$OUT/r4d_prof_bench.json" 2> "$OUT/r4d_prof_bench.err" && \
python3 tools/rocprof_summary.py "$OUT/r4d_prof" "$OUT/r04_thin_bench" > /dev/null && head -12 "$OUT/r04_thin_bench_summary.md" | cut -c1-160 && \
mkdir -p "$OUT/r4d_shape" && timeout -k 10 250 rocprofv3 --kernel-trace --output-format csv -d "$OUT/r4d_shape/runc" -- python3 tools/shape_profile.py run "$OUT/r4d_shape/oplog.txt" > "$OUT/r4d_shape_run.log" 2>&1 && \
python3 tools/shape_profile.py report "$OUT/r4d_shape" "$OUT/r4d_shape/report.md" > /dev/null 2> "$OUT/r4d_report.err"; head -16 "$OUT/r4d_shape/report.md" | tail -9
