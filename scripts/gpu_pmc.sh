#!/bin/bash
# HBM traffic and SQ counters of the default bench command (eager launches, no stream overlap), separate PMC passes
export RES=$(realpath -m "${RES:-out}"); mkdir -p "$RES"   # where this script writes its results
export PYTHONDONTWRITEBYTECODE=1 VTP_OVERLAP=0
R=$PWD
rm -rf $RES/pmc; mkdir -p $RES/pmc
cd /tmp && export TMPDIR=/tmp
# three separate passes (MI355X_MICROARCH.md: FETCH_SIZE and WRITE_SIZE do not fit one pass; SQ set = 8 SQ slots + GRBM): HBM bytes, and
# matrix-pipe / VALU / LDS occupancy (MfmaUtil of north_star -- tools/pmc_summarize.py `derived`)
i=0
for c in "FETCH_SIZE" "WRITE_SIZE" "SQ_VALU_MFMA_BUSY_CYCLES SQ_BUSY_CYCLES SQ_ACTIVE_INST_VALU SQ_LDS_BANK_CONFLICT SQ_LDS_IDX_ACTIVE SQ_WAVE_CYCLES SQ_INSTS_VALU GRBM_GUI_ACTIVE"; do
  i=$((i+1))
  timeout 600 rocprofv3 --pmc $c --kernel-trace --output-format csv -d $RES/pmc/p$i -o pmc -- python $R/bench.py --full --steps 1 --warmup 1 --no-cpu-baseline --no-lpips-run --no-separate-run --no-graphs > $RES/pmc_p$i.log 2>&1
  echo "pmc pass $i rc=$?"
done
cd $R
python tools/pmc_summarize.py $RES/pmc $RES/pmc_summary.json
find $RES/pmc -name "*.csv" -size +1M -delete
