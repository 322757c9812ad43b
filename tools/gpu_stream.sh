#!/bin/bash
# config-4 frontend lines (both windows) with the per-phase breakdown
set -o pipefail
export TMPDIR=/tmp
OUT=${OUT:-bench_out}
mkdir -p $OUT
T=${TAG:-s}
timeout -k 10 400 python -u bench.py --full --workload stream --steps ${STEPS:-500} --cpu-seconds 5 > $OUT/${T}_stream_json.json 2> $OUT/${T}_stream_json.err &&
timeout -k 10 400 python -u bench.py --full --workload stream --window config2 --steps ${STEPS:-500} --cpu-seconds 5 > $OUT/${T}_stream_c2.json 2> $OUT/${T}_stream_c2.err
