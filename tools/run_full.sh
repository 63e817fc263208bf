#!/bin/bash
# GPU box: the GPU test suite, then the full bench (headline + per-kernel
# figures + CPU baseline + extras: `bench.py --full`).  Logs go to
# $OUT_DIR (default bench_out/).
cd "${GRAFT_REPO_ROOT:-$(dirname "$0")/..}"
export OUT=${OUT_DIR:-bench_out}
mkdir -p "$OUT"
if [ -z "$SKIP_TESTS" ]; then
  timeout -k 10 300 python -u -m pytest tests -m gpu -x -q --timeout 120 --timeout-method thread > "$OUT/t1.log" 2>&1; rc=$?
  tail -2 "$OUT/t1.log"
  [ $rc -eq 0 ] || exit $rc
fi
timeout -k 10 600 python3 bench.py --full ${BENCH_ARGS:---steps 100 --warmup 10} > "$OUT/bench_full.log" 2>&1 || exit $?
python3 - <<'PY'
import json, os
s = open(os.path.join(os.environ["OUT"], "bench_full.log")).read()
d = json.JSONDecoder().raw_decode(s[s.rindex('{"metric"'):])[0]
print({k: d[k] for k in ("value", "ms_per_step", "kernels")}, d["roofline"]["frac"])
for e in d.get("extras", []):
    print(e.get("config")[:64], e.get("compress_ms"), e.get("decompress_ms"), e.get("algorithmic_GBps"))
PY
