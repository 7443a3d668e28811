# usage: bash tools/bench_all.sh <tag> [out dir, default bench_out]  -- one `bench.py --full` line per BASELINE config (with
# roofline and cpu_baseline), into <out dir>/<tag>_bench_cfg<N>.json
cd "$(dirname "$0")/.."
TAG=${1:-r03}
OUT=${2:-bench_out}
mkdir -p "$OUT"
for c in 2 1 3 5 4; do
  steps=30; [ $c = 4 ] && steps=10
  timeout -k 10 600 python bench.py --full --config $c --steps $steps --warmup 3 --cpu-seconds 8 > "$OUT/${TAG}_bench_cfg$c.log" 2>&1
  echo "cfg $c rc=$?"
  grep "^{" "$OUT/${TAG}_bench_cfg$c.log" > "$OUT/${TAG}_bench_cfg$c.json"
  python - "$OUT/${TAG}_bench_cfg$c.json" <<'PY'
import json, sys
d=json.load(open(sys.argv[1]))
r=d["roofline"]; cb=d["cpu_baseline"]
print("  %s: %.1f img/s, %.3f ms/step, dominant %s frac %.3f, step-level mfma frac %.3f, cpu %.1f img/s (%d cores), 1 thread %.1f" % (d["config"]["workload"][:40], d["value"], d["ms_per_step"], r["kernel"], r["frac"], d["config"]["decoder_mfma_frac_of_step"], cb["value"], cb["cores"], cb["one_thread"]["value"]))
PY
done
