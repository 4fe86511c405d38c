# two back-to-back driver-shape bench runs with every leg (--full, N = 1): run-to-run spread of a build;
# output under $1 (default bench_out)
out=${1:-bench_out}; mkdir -p "$out"
for i in 1 2; do
  timeout -k 10 600 python bench.py --full --steps 20 --warmup 5 > "$out/bench_final_$i.json" 2> "$out/bench_final_$i.err" || exit $?
  python3 tools/bench_brief.py "$out/bench_final_$i.json"
done
