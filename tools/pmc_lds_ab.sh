#!/bin/bash
# GPU box: per variant library set, the c2 bench's LDS PMC (bank conflicts /
# active cycles, one rocprofv3 pass), each under the set swapped in by
# tools/ab.py.  Time the sets against the in-tree build with `tools/ab.py run`.
# Output goes to $OUT_DIR (default bench_out/).
#   usage: bash tools/pmc_lds_ab.sh tools/ablibs/<variant>...
cd "${GRAFT_REPO_ROOT:-$(dirname "$0")/..}"
export TMPDIR=/tmp
OUT=${OUT_DIR:-bench_out}
mkdir -p "$OUT"
for L in "$@"; do
  T=$(basename "$L")
  python3 tools/ab.py with "$L" --limit 120 -- rocprofv3 --pmc SQ_LDS_BANK_CONFLICT SQ_LDS_IDX_ACTIVE SQ_INSTS_LDS SQ_INSTS_VALU GRBM_GUI_ACTIVE \
    -d "$OUT/pl_$T" -o run --output-format csv -- python3 bench.py --steps 2 --warmup 1 --no-cpu-baseline --no-extras --no-verify > "$OUT/pl_$T.log" 2>&1 || exit 1
done
