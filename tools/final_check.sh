# End-of-session check: full GPU suite, smoke, default bench line with every leg (--full).
#   bash tools/final_check.sh [OUT_DIR]      (default: results/final)
set -o pipefail
out=${1:-results/final}
mkdir -p "$out"
timeout -k 10 900 python -u -m pytest tests -m gpu -x -q --timeout 120 --timeout-method thread > "$out/pytest_gpu.log" 2>&1 || { tail -30 "$out/pytest_gpu.log"; exit 1; }
tail -1 "$out/pytest_gpu.log"
timeout -k 10 300 python -u -c "import __graft_entry__ as g; g.smoke()" 2>&1 | grep smoke || exit 2
timeout -k 10 400 python -u bench.py --full > "$out/bench.json" 2> "$out/bench.err" || { tail -20 "$out/bench.err"; exit 3; }
cat "$out/bench.json"
