# final verification without the profiler: full GPU suite, smoke, the benchmark with --full (CPU baseline and the other extras)
#   bash tools/run_final_light.sh OUTDIR      logs and the JSON line go to OUTDIR (relative to the repository root)
cd "$(dirname "$0")/.." || exit 1
O=${1:?usage: tools/run_final_light.sh OUTDIR}
mkdir -p "$O" || exit 1
timeout -k 10 900 python -m pytest tests -m gpu -q > "$O/final_tests.log" 2>&1; rc=$?; echo "pytest rc=$rc" >> "$O/final_tests.log"
tail -4 "$O/final_tests.log"
[ $rc -eq 0 ] || exit $rc
timeout -k 10 300 python -c "import __graft_entry__ as g; g.smoke(); print('smoke ok')" > "$O/final_smoke.log" 2>&1 || { tail -5 "$O/final_smoke.log"; exit 1; }
tail -2 "$O/final_smoke.log"
timeout -k 10 600 python bench.py --full > "$O/final_bench.json" 2> "$O/final_bench.err" || { tail -5 "$O/final_bench.err"; exit 1; }
tail -2 "$O/final_bench.err"; cat "$O/final_bench.json"
