#!/bin/bash
# GPU box: the out-of-order-start tests against the test-only variant library
# set tools/ablibs/pskew/ (python tools/variants.py pskew), which delays every
# k_pcompress workgroup by (63 - g % 64) us at its start.  tools/ab.py swaps
# the set in and restores the in-tree one on exit, whatever happens.  The log
# goes to $OUT_DIR (default bench_out/).
set -e
cd "${GRAFT_REPO_ROOT:-$(dirname "$0")/..}"
OUT=${OUT_DIR:-bench_out}
mkdir -p "$OUT"
python3 tools/ab.py with tools/ablibs/pskew --limit 200 -- python -u -m pytest tests/test_gpu_progress.py \
  tests/test_gpu_teams.py -x -v --timeout 120 --timeout-method thread -k "out_of_order or team_layouts" \
  > "$OUT/${TAG:-skew}_skew_tests.log" 2>&1
tail -3 "$OUT/${TAG:-skew}_skew_tests.log"
