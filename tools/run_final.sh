# final verification on the GPU box: full GPU suite, smoke, then the benchmark with --full (CPU baseline and the other extras)
# under rocprofv3 --kernel-trace --stats
#   bash tools/run_final.sh OUTDIR      logs, the JSON line and the trace go to OUTDIR (relative to the repository root)
cd "$(dirname "$0")/.." || exit 1
R=$(pwd)
O=$(realpath -m "${1:?usage: tools/run_final.sh OUTDIR}")
mkdir -p "$O" || exit 1
timeout -k 10 900 python -m pytest tests -m gpu -q > "$O/final_tests.log" 2>&1; rc=$?; echo "pytest rc=$rc" >> "$O/final_tests.log"
tail -4 "$O/final_tests.log"
[ $rc -eq 0 ] || exit $rc
timeout -k 10 300 python -c "import __graft_entry__ as g; g.smoke(); print('smoke ok')" > "$O/final_smoke.log" 2>&1 || { tail -5 "$O/final_smoke.log"; exit 1; }
tail -2 "$O/final_smoke.log"
cd "${TMPDIR:-/tmp}" || exit 1
timeout -k 10 900 rocprofv3 --kernel-trace --stats -d "$O/prof_final" -o fin --output-format csv -- python3 "$R/bench.py" --full > "$O/final_bench.json" 2> "$O/final_bench.err"
rc=$?; tail -3 "$O/final_bench.err"; cat "$O/final_bench.json"; exit $rc
