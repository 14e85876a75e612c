#!/bin/bash
# round 5, final build: serial-mode kernel stats, the three PMC passes, then the default bench line quoting THESE counters
export RES=$(realpath -m "${RES:-out}"); mkdir -p "$RES"   # where this script writes its results
export PYTHONDONTWRITEBYTECODE=1
VTP_OVERLAP=0 bash scripts/gpu_prof.sh > $RES/prof_serial.log 2>&1
cp $(find $RES/prof_full -name "*kernel_stats.csv" | head -1) $RES/r05_kernel_stats_full_eager_b32.csv
head -8 $RES/r05_kernel_stats_full_eager_b32.csv | cut -c1-160
bash scripts/gpu_pmc.sh 2>&1 | tail -6
cp $RES/pmc_summary.json $RES/r05_pmc_summary.json
cp $RES/r05_pmc_summary.json profiles/r05_pmc_summary.json
VTP_BENCH_GEMM_TABLE=$RES/r05_gemm_table.txt timeout 900 python bench.py --full > $RES/r05_bench_default_n1.json 2> $RES/r05_bench_default_n1.err
echo "bench rc=$?"; cut -c1-300 $RES/r05_bench_default_n1.json
