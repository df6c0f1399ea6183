#!/bin/bash
# Third session of round 4, LAST evidence call (final code): GPU suite on the frozen table (verbose, with durations), the bench line with --full, smoke().
OUT=${1:?usage: tools/round_end_evidence_r4h.sh OUTPUT_DIR}
cd "$(dirname "$0")/.." && export TMPDIR=/tmp && mkdir -p "$OUT"
timeout -k 10 600 python -m pytest tests -x -v -m gpu --durations=25 > "$OUT/r4h_gpu_suite.log" 2>&1; tail -n 32 "$OUT/r4h_gpu_suite.log" | cut -c1-150
grep -q " passed" "$OUT/r4h_gpu_suite.log" && ! grep -q " failed" "$OUT/r4h_gpu_suite.log" && \
timeout -k 10 300 python bench.py --full > "$OUT/r4h_bench.json" 2> "$OUT/r4h_bench.err" && tail -c 300 "$OUT/r4h_bench.json" && \
python -c "import __graft_entry__ as g; g.smoke(); print('smoke ok')" > "$OUT/r4h_smoke.log" 2>&1; tail -n 2 "$OUT/r4h_smoke.log"
