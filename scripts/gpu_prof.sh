#!/bin/bash
# rocprofv3 kernel-trace summary of the default bench command (eager so every kernel is attributed) -> $RES/prof_full
export RES=$(realpath -m "${RES:-out}"); mkdir -p "$RES"   # where this script writes its results
export PYTHONDONTWRITEBYTECODE=1
R=$PWD
mkdir -p $RES/prof_full
cd /tmp && export TMPDIR=/tmp
VTP_OVERLAP=${VTP_OVERLAP:-1} timeout 900 rocprofv3 --kernel-trace --stats --output-format csv -d $RES/prof_full -o full -- python $R/bench.py --full --steps 4 --warmup 2 --no-cpu-baseline --no-lpips-run --no-separate-run --no-graphs > $RES/prof_full.log 2>&1
echo "prof rc=$?"
cd $R
ls $RES/prof_full | head
f=$(find $RES/prof_full -name "*kernel_stats.csv" | head -1)
head -40 "$f" | cut -c1-200
# keep only the summary (the trace is large)
find $RES/prof_full -name "*kernel_trace.csv" -delete
find $RES/prof_full -name "*.db" -delete
tail -1 $RES/prof_full.log | cut -c1-300
