OUT=${OUT:-out}  # results directory
mkdir -p $OUT
timeout -k 10 300 python -u -m pytest tests -m gpu -x -q --timeout 120 --timeout-method thread > $OUT/gputests.log 2>&1; rc=$?; tail -4 $OUT/gputests.log; [ $rc -eq 0 ] || exit $rc
timeout -k 10 200 python bench.py --full --config 2 --steps 10 --warmup 2 --cpu-sample 0 --cpu-workers 0 > $OUT/bc2.log 2>&1 || exit 1
timeout -k 10 200 python bench.py --full --config 3 --steps 5 --warmup 1 --cpu-sample 0 --cpu-workers 0 > $OUT/bc3.log 2>&1 || exit 1
grep -ho "\"value\": [0-9.]*\|\"kernel_ms_per_step\": {[^}]*}" $OUT/bc2.log $OUT/bc3.log
