# usage: bash tools/split_ablate.sh [out dir, default bench_out] -- time the fp16x3 forward kernel with the ablation builds
# under build/ (`bench.py --full`: the per-kernel breakdown)
cd "$(dirname "$0")/.."
OUT=${1:-bench_out}
mkdir -p "$OUT"
export SVAE_GEMM=fp16x3
for v in main ab1 ab2 ab3; do
  cp build/libsvae_$v.so spatial_vae_amd/libsvae_hip.so
  timeout -k 10 200 python bench.py --full --gemm fp16x3 --no-secondary --no-cpu-baseline --steps 20 > "$OUT/bench_$v.json" 2> "$OUT/bench_$v.err"
  python - "$OUT/bench_$v.json" "$v" <<'PY'
import json, sys
d = json.load(open(sys.argv[1]))
k = d["roofline"]["kernels_ms_per_step"]
print(sys.argv[2], d["ms_per_step"], "dense_fwd", k["dense_fwd"], "prepare", k["prepare"])
PY
done
