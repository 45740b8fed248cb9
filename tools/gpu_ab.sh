#!/bin/bash
# Same-box A/B of env knobs on the full bench line (no CPU leg): one line per run.  A run whose
# result check fails still prints its times, marked CHECK-FAILED.
#   AB="CE_V3=2 CE_V3=3" BENCH_ARGS="--no-variant-b" tools/gpu_ab.sh
cd "$(dirname "$0")/.."
OUT=${OUT:-bench_out}
mkdir -p $OUT
run() {
  echo -n "$1 "
  env ${1//,/ } timeout -k 10 200 python bench.py --full --configs '' --no-cpu ${BENCH_ARGS:-} > $OUT/ab.json 2> $OUT/ab.err
  local rc=$?
  [ $rc -eq 124 ] || [ $rc -eq 137 ] || [ $rc -ge 128 ] && { echo "bench died rc=$rc"; tail -3 $OUT/ab.err; return 1; }
  python3 -c "
import json,sys;d=json.loads(open('$OUT/ab.json').read());b=d.get('variant_b') or {}
print(d['ms_per_step'],d['roofline']['avg_launch_ms'],d['kernels_ms_per_step'].get('open_setup'),'B',b.get('avg_launch_ms'),'' if $rc == 0 else 'CHECK-FAILED')" || { tail -3 $OUT/ab.err; return 1; }
}
for v in ${AB:-"X=0" "CE_SPIN=1"}; do run $v || exit 1; done
