#!/bin/bash
# One GPU session: tests, smoke, bench (with CPU baseline and the N=1 extras).  Stops at the
# first failure; every step has its own time limit.
set -o pipefail
export PYTHONDONTWRITEBYTECODE=1
OUT=${OUT:-results}
mkdir -p $OUT
echo "== pytest -m gpu"; timeout -k 10 900 python -u -m pytest tests -x -q -m gpu --timeout 300 --timeout-method thread > $OUT/gpu_tests.log 2>&1; rc=$?; tail -5 $OUT/gpu_tests.log; [ $rc -eq 0 ] || exit $rc
echo "== smoke"; timeout -k 10 300 python -c "import __graft_entry__ as g; g.smoke()" > $OUT/smoke.log 2>&1; rc=$?; tail -3 $OUT/smoke.log; [ $rc -eq 0 ] || exit $rc
echo "== bench"; timeout -k 10 600 python bench.py --full > $OUT/bench.json 2> $OUT/bench.err; rc=$?; cat $OUT/bench.json; tail -3 $OUT/bench.err; [ $rc -eq 0 ] || exit $rc
if [ -n "$PROFILE" ]; then echo "== profile"; bash tools/profile.sh; fi
