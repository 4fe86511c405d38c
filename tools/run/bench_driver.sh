# the driver's bench shape with every leg (--full), N = 1; output under $1 (default bench_out)
out=${1:-bench_out}; mkdir -p "$out"
timeout -k 10 600 python bench.py --full --steps 20 --warmup 5 > "$out/bench_driver.json" 2> "$out/bench_driver.err"; rc=$?
tail -c 3000 "$out/bench_driver.err"; python3 tools/bench_brief.py "$out/bench_driver.json"; exit $rc
