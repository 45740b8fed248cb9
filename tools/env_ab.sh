#!/bin/bash
# Same-box A/B of one env knob on the full C2 bench line (no CPU leg), twice each:
#   KNOB=CE_V3 VALS="0 1 2 3" tools/env_ab.sh
cd "$(dirname "$0")/.."
OUT=${OUT:-bench_out}
mkdir -p $OUT
for r in 1 2; do
  for V in ${VALS}; do
    echo -n "$KNOB=$V "
    env $KNOB=$V timeout -k 10 200 python bench.py --full --configs '' --no-cpu --no-host-buffers ${BENCH_ARGS:-} 2> $OUT/envab.err | python3 -c "
import json,sys;d=json.loads(sys.stdin.read().strip().splitlines()[-1]);b=d.get('variant_b') or {}
print(d['ms_per_step'],d['roofline']['avg_launch_ms'],'B',b.get('ms_per_step'),b.get('avg_launch_ms'))" || { tail -3 $OUT/envab.err; exit 1; }
  done
done
