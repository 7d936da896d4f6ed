#!/bin/bash
# GPU tests named by TESTS (optional), then an interleaved new/old A/B of the default bench line
# (tools/_ab/libmmfd_old.so = the previous build, swapped in place)
set -e
cd "$GRAFT_REPO_ROOT"
OUT=${OUT:-out}  # where the logs go
mkdir -p $OUT
if [ -n "$TESTS" ]; then
  timeout -k 10 600 python -u -m pytest $TESTS -m gpu -x -q --timeout 300 --timeout-method thread > $OUT/ab_t.log 2>&1 \
    || { echo TESTS_FAILED; tail -30 $OUT/ab_t.log; exit 1; }
  echo TESTS_OK; tail -1 $OUT/ab_t.log
fi
LIB=multimodal-misinformation-detection_amd/libmmfd_hip.so
cp $LIB $OUT/_new.so
for r in 1 2; do
  for v in new old; do
    if [ $v = old ]; then cp tools/_ab/libmmfd_old.so $LIB; else cp $OUT/_new.so $LIB; fi
    timeout -k 10 300 python bench.py --steps 8 --warmup 2 --full --no-cpu-baseline $BENCH_ARGS > $OUT/bab_$v$r.log 2>&1
    python3 -c "
import json
for l in open('$OUT/bab_$v$r.log'):
    if l.startswith('{'):
        d = json.loads(l); b = d.get('bf16') or {}
        print('$v$r', d['value'], d['ms_per_step'], d['roofline']['frac'], b.get('value'), b.get('ms_per_step'))"
  done
done
cp $OUT/_new.so $LIB
rm -f $OUT/_new.so
