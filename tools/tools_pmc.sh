#!/bin/bash
# HBM traffic per kernel from rocprofv3 PMC counters: one pass per counter (FETCH_SIZE and
# WRITE_SIZE do not fit one TCC pass on gfx950), kernel dispatch data only, eager steps.
# Output: $MRG_OUT/pmc (default prof_out/pmc in the repository, ignored by git).
set -o pipefail
export TMPDIR=/tmp
R=$GRAFT_REPO_ROOT
O=${MRG_OUT:-$R/prof_out}/pmc
mkdir -p $O
cd /tmp
for c in FETCH_SIZE WRITE_SIZE; do
  timeout -k 10 400 rocprofv3 --pmc $c -d $O/$c -o pmc --output-format csv -- python3 $R/bench.py --full --graph 0 --wgrad-stream 0 --cpu-baseline 0 --steps 1 --warmup 1 > $O/$c.log 2>&1 || { echo "pmc $c failed"; tail -20 $O/$c.log; exit 1; }
  echo "pmc $c ok"
done
