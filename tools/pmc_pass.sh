#!/bin/bash
# SQ counters of the curvature pass kernels (three sets, separate runs): OUT=<dir> tools/pmc_pass.sh <tag> [kernel-name filter]
# (run on the GPU box; writes <dir>/<tag>_pmc_sq_{insts,waits}.txt and <dir>/<tag>_pmc_lds.txt, with the runs' logs)
ROOT=$(cd "$(dirname "$0")/.." && pwd)
OUT=$(mkdir -p "${OUT:?OUT=<directory for the results> bash tools/pmc_pass.sh <tag> [filter]}" && cd "$OUT" && pwd) || exit 1
F=${2:-k_h2}
cd /tmp && export TMPDIR=/tmp
run() {  # set name, output name, counters...
  s=$1; o=$2; shift 2
  REPS=5 timeout -k 10 400 rocprofv3 --pmc "$@" --output-format csv -d /tmp/pmc${s}_$tag -o p -- python3 $ROOT/tools/probe_pass.py > $OUT/${tag}_pmc_$s.log 2>&1 || exit 1
  python3 $ROOT/tools/pmc_summary.py /tmp/pmc${s}_$tag/p_counter_collection.csv $F > $OUT/${tag}_pmc_$o.txt
}
tag=$1
run a sq_insts SQ_WAVE_CYCLES SQ_INSTS_VALU SQ_INSTS_SALU SQ_INSTS_LDS SQ_ACTIVE_INST_VALU SQ_WAIT_ANY SQ_WAIT_INST_ANY SQ_INSTS_VMEM_RD
run b sq_waits SQ_WAVE_CYCLES SQ_BUSY_CYCLES SQ_WAIT_ANY SQ_WAIT_INST_ANY SQ_ACTIVE_INST_ANY SQ_ACTIVE_INST_VALU SQ_ACTIVE_INST_LDS SQ_WAIT_INST_LDS
run c lds SQ_LDS_BANK_CONFLICT SQ_LDS_IDX_ACTIVE SQ_LDS_ADDR_CONFLICT SQ_WAVES SQ_INSTS_LDS
