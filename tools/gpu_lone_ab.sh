#!/bin/bash
# Lone-scan (batch 1) latency A/B: default build vs ablib variants; per-kernel
# one-stream event times of the lone path.  Usage: tools/gpu_lone_ab.sh <variant> ...
export TMPDIR=/tmp
OUT=${OUT:-bench_out}
mkdir -p $OUT
for v in default "$@"; do
  if [ $v = default ]; then L=""; else L="LGS_LIB=ablib/$v.so"; fi
  env $L timeout -k 10 300 python -u bench.py --full --batch 1 --streams 1 --steps 400 --no-cpu --loop-line 0 --dropin-line 0 > $OUT/lone_$v.json 2> $OUT/lone_$v.err || exit $?
  python3 -c "
import json; d=json.loads(open('$OUT/lone_$v.json').read().strip().splitlines()[-1])
print('$v', d['value'], 'p50', d['p50_scan_match_ms'], 'p90', d['p90_scan_match_ms'], {k: v['avg_ms'] for k, v in d['kernels'].items()})"
done
