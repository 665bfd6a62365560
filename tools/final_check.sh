#!/bin/bash
# End-of-round check on one MI355X: the whole -m gpu suite (timed), smoke()
# and a 20-step default bench line with everything --full adds to it.
# Usage: tools/final_check.sh <tag>   -> $KH_OUT_DIR/<tag>/ (default bench_out/<tag>/)
set -o pipefail
tag=${1:?tag}
cd "$(dirname "$0")/.."
out=${KH_OUT_DIR:-bench_out}/$tag
mkdir -p "$out"
t0=$(date +%s)
timeout -k 10 900 python -u -m pytest tests -m gpu -x -q --timeout 170 --timeout-method thread \
    > "$out/gpu_tests.txt" 2>&1 || { echo "gpu suite failed"; tail -40 "$out/gpu_tests.txt"; exit 1; }
echo "suite $(( $(date +%s) - t0 )) s"; tail -2 "$out/gpu_tests.txt"
timeout -k 10 300 python -c "import __graft_entry__ as g; g.smoke(); print('smoke ok')" > "$out/smoke.txt" 2>&1 || { echo "smoke failed"; tail -20 "$out/smoke.txt"; exit 1; }
tail -1 "$out/smoke.txt"
timeout -k 10 400 python -u bench.py --full --steps 20 --warmup 2 > "$out/bench.json" 2> "$out/bench.err" || { echo "bench failed"; tail -20 "$out/bench.err"; exit 1; }
cat "$out/bench.json"
