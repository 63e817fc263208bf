cd "${GRAFT_REPO_ROOT}"
OUT=${OUT_DIR:-bench_out}
mkdir -p "$OUT"
for i in 1 2 3 4 5 6; do
  DIETGPU_BENCH_ADDRS=1 timeout -k 10 120 python3 bench.py --full --no-cpu-baseline --no-extras --steps 100 --warmup 5 > "$OUT/rep_$i.log" 2> "$OUT/rep_$i.err" || exit 1
  python3 -c "
import json
for l in open('$OUT/rep_$i.log'):
    if l.startswith('{'):
        d=json.loads(l); print($i, d['ms_per_step'], d['kernels'])
for l in open('$OUT/rep_$i.err'):
    if l.startswith('addrs'): print(l.strip())"
done
