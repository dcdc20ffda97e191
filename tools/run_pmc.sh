#!/bin/bash
# usage (on the GPU machine): [OUT=<dir>] tools/run_pmc.sh <outdir-name> [bench args...]
# one rocprofv3 PMC pass over bench.py --full (counters only with --kernel-trace)
set -e
name=$1; shift
R=$(cd "$(dirname "$0")/.." && pwd)
mkdir -p ${OUT:-$R/prof_out}
out=$(cd ${OUT:-$R/prof_out} && pwd)/$name
cd /tmp && export TMPDIR=/tmp
rocprofv3 --kernel-trace --pmc SQ_WAVES SQ_INSTS_VALU SQ_INSTS_SALU SQ_INSTS_LDS SQ_WAVE_CYCLES SQ_ACTIVE_INST_VALU SQ_WAIT_INST_ANY SQ_BUSY_CYCLES \
  --output-format csv -d $out -- python3 $R/bench.py --full --steps 2 --warmup 1 --no-cpu --no-latency "$@" > $out.log 2>&1
python3 $R/tools/pmc_summary.py $out
