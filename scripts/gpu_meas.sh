#!/bin/bash
# measurement bundle for profiles/: default bench line (with cpu_baseline), rocprofv3 kernel stats of the same command in eager
# / no-overlap mode (per-kernel durations comparable with bench's HIP-event roofline), PMC traffic passes
export RES=$(realpath -m "${RES:-out}"); mkdir -p "$RES"   # where this script writes its results
export PYTHONDONTWRITEBYTECODE=1
python bench.py --full > $RES/bench_default.json 2> $RES/bench_default.err; echo "bench rc=$?"; cut -c1-400 $RES/bench_default.json
VTP_OVERLAP=0 bash scripts/gpu_prof.sh > $RES/prof_run.log 2>&1; tail -3 $RES/prof_run.log | cut -c1-300
bash scripts/gpu_pmc.sh
