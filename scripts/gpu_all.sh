#!/bin/bash
# full GPU regression: every gpu-marked test + the three bench workloads
export RES=$(realpath -m "${RES:-out}"); mkdir -p "$RES"   # where this script writes its results
export PYTHONDONTWRITEBYTECODE=1
timeout 1200 python -m pytest tests -m gpu -q --tb=short -p no:cacheprovider > $RES/t_all.log 2>&1
echo "tests rc=$?" > $RES/rc.log
timeout 900 python bench.py --full --steps 8 --warmup 3 --no-cpu-baseline > $RES/bench_full.log 2>&1
echo "bench full rc=$?" >> $RES/rc.log
timeout 600 python bench.py --full --steps 10 --warmup 3 --no-cpu-baseline --workload vtp_base_rec > $RES/bench_rec.log 2>&1
echo "bench rec rc=$?" >> $RES/rc.log
cat $RES/rc.log
grep -E "passed|failed|FAILED|rror" $RES/t_all.log | tail -8
tail -1 $RES/bench_full.log | cut -c1-200
tail -1 $RES/bench_rec.log | cut -c1-200
