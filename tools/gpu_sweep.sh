# Pixel-count sweep of the room0 bench (headline + per-kernel spans).  usage: bash tools/gpu_sweep.sh OUTDIR
set -o pipefail
OUT=${1:?output directory}
mkdir -p $OUT
for px in 1000 2000 4000 8000 16000; do
  timeout -k 10 200 python bench.py --full --steps 20 --warmup 5 --no-cpu-baseline --pixels $px > $OUT/b$px.json 2> $OUT/b$px.err || { tail -5 $OUT/b$px.err; exit 1; }
  python -c "import json; d=json.load(open('$OUT/b$px.json')); print($px, round(d['value']/1e6,1), round(d['ms_per_step'],3), d['kernels_ms'])"
done
