#!/bin/bash
# the round's evidence in one call: every GPU test with the parity lines kept, serial-mode kernel stats, the PMC passes, then the
# default bench line (driver contract, CPU baseline included) with the per-shape GEMM table.  TAG=r04 by default.
export RES=$(realpath -m "${RES:-out}"); mkdir -p "$RES"   # where this script writes its results
export PYTHONDONTWRITEBYTECODE=1
R=$PWD; T=${TAG:-r04}
timeout 1800 python -m pytest tests -m gpu -q -s -p no:cacheprovider > $RES/${T}_gputests.log 2>&1
echo "gpu tests rc=$?"; grep -E "passed|failed" $RES/${T}_gputests.log | tail -2
grep -E "^\.*F*(PARITY|TOOLS)|\[attn_bwd|split-K combine|fp8 vs bf16|resume shard|grouped wgrad" $RES/${T}_gputests.log | sed 's/^[.F]*//' > $RES/${T}_parity.log
wc -l $RES/${T}_parity.log
VTP_OVERLAP=0 bash scripts/gpu_prof.sh > $RES/prof_serial.log 2>&1
cp $RES/prof_full/full_kernel_stats.csv $RES/${T}_kernel_stats_full_eager_b32.csv
head -12 $RES/${T}_kernel_stats_full_eager_b32.csv | cut -c1-160
bash scripts/gpu_pmc.sh 2>&1 | tail -16
cp $RES/pmc_summary.json $RES/${T}_pmc_summary.json
# the bench line last: its roofline block quotes the SQ counters of THIS build (the summary just written), not of an earlier one
cp $RES/${T}_pmc_summary.json profiles/${T}_pmc_summary.json
VTP_BENCH_GEMM_TABLE=$RES/${T}_gemm_table.txt timeout 1200 python bench.py --full > $RES/${T}_bench_default_n1.json 2> $RES/${T}_bench_default_n1.err
echo "bench rc=$?"; cut -c1-400 $RES/${T}_bench_default_n1.json
