#!/bin/bash
# GPU box check: the -m gpu suite, then (only if pytest ended normally: all passed or some tests
# failed) one full bench run (bench.py --full: CPU baseline, parity checks, roofline).
# Usage: tools/gpu_check.sh [pytest selection args...]; logs go to $CHECK_OUT (default check_out/)
cd "$(dirname "$0")/.." || exit 2
OUT=${CHECK_OUT:-check_out}
mkdir -p "$OUT"
timeout -k 10 1000 python -u -m pytest tests -m gpu -v --timeout 300 --timeout-method thread "$@" > "$OUT/gpu_tests.log" 2>&1
rc=$?
echo "pytest exit $rc" >> "$OUT/gpu_tests.log"
tail -5 "$OUT/gpu_tests.log"
if [ $rc -ne 0 ] && [ $rc -ne 1 ]; then exit $rc; fi
timeout -k 10 300 python -u bench.py --full > "$OUT/bench.log" 2>&1
rc2=$?
tail -3 "$OUT/bench.log"
exit $rc2
