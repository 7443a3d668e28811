# usage: bash tools/split_ab.sh [out dir, default bench_out]  -- parity subset + `bench.py --full` in fp16x3 mode
cd "$(dirname "$0")/.."
OUT=${1:-bench_out}
mkdir -p "$OUT"
export SVAE_GEMM=fp16x3
timeout -k 10 300 python -m pytest tests/test_gpu_parity.py tests/test_gpu_fullsize.py tests/test_gpu_geometry.py -x -q -m gpu > "$OUT/gpu_tests_split.log" 2>&1
tail -3 "$OUT/gpu_tests_split.log"
timeout -k 10 200 python bench.py --full --gemm fp16x3 --no-secondary --no-cpu-baseline > "$OUT/bench_split.json" 2> "$OUT/bench_split.err"
python - "$OUT/bench_split.json" <<'PY'
import json, sys
d = json.load(open(sys.argv[1]))
print(d["value"], d["ms_per_step"])
print(d["roofline"]["kernels_ms_per_step"])
PY
