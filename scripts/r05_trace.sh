#!/bin/bash
# kernel trace of the default bench (hipGraph segments + side streams) for tools/trace_gaps.py
export RES=$(realpath -m "${RES:-out}"); mkdir -p "$RES"   # where this script writes its results
cd "$(dirname "$0")/.." && export TMPDIR=/tmp
rm -rf $RES/trace
export PYTHONDONTWRITEBYTECODE=1
timeout 300 rocprofv3 --kernel-trace --output-format csv -d $RES/trace -- python bench.py --full --steps 6 --warmup 3 --no-cpu-baseline --no-lpips-run --no-separate-run > $RES/trace_bench.log 2>&1
tail -1 $RES/trace_bench.log | cut -c1-300
f=$(ls $RES/trace/*/*_kernel_trace.csv | head -1)
ls -la $f
python tools/trace_gaps.py $f > $RES/trace_gaps.txt 2>&1
cat $RES/trace_gaps.txt
cp $f $RES/trace_kernels.csv
rm -rf $RES/trace
