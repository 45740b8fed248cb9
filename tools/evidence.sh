#!/bin/bash
# Round evidence on one box: the full bench line, rocprofv3 kernel stats of the C2 step, the C3
# line with its CPU baseline, and the C3 step traces (GPU timeline, host calls, traffic).
set -o pipefail
cd "$(dirname "$0")/.."
R=$PWD
EV=$R/${OUT:-bench_out}/ev
mkdir -p $EV
timeout -k 10 900 python -u bench.py --full > $EV/bench.json 2> $EV/bench.err || { echo "bench rc=$?"; tail -5 $EV/bench.err; exit 1; }
tail -1 $EV/bench.json | head -c 300; echo
(T=$(mktemp -d) && cd $T && export TMPDIR=$T && timeout -k 10 300 rocprofv3 --kernel-trace --stats --output-format csv -d $EV/prof -o b -- python3 $R/bench.py --full --steps 10 --no-cpu --configs '' --no-variant-b --no-host-buffers >$EV/bench_prof.json 2> $EV/bench_prof.err) || { echo "prof failed"; exit 1; }
timeout -k 10 300 python -u bench_configs.py --config c3 > $EV/c3.json 2> $EV/c3.err || { echo "c3 failed"; exit 1; }
CE_C3_NO_NAMES=1 timeout -k 10 300 python -u bench_configs.py --config c3 --no-cpu > $EV/c3_no_names.json 2> $EV/c3nn.err || { echo "c3nn failed"; exit 1; }
CE_C3_NO_NAMES=1 bash tools/c3_step.sh > /dev/null && CE_C3_NO_NAMES=1 bash tools/c3_host.sh > /dev/null && CE_C3_NO_NAMES=1 bash tools/c3_traffic.sh > /dev/null && echo evidence done
