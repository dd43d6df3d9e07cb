#!/bin/bash
# The profile recipe behind profiles/r01_*: run on the GPU box from the repo root
#   (bash tools/lab/prof.sh OUTDIR, OUTDIR an absolute path); outputs land under OUTDIR.
# 1. kernel trace + stats of the bench command   2./3. FETCH_SIZE / WRITE_SIZE of the relax kernels
# (counters in their own passes, with --kernel-trace only)   4. the bench line itself
cd /tmp && export TMPDIR=/tmp
R=${GRAFT_REPO_ROOT:-/root/repo}
O=${1:?usage: prof.sh OUTDIR}
mkdir -p $O
rocprofv3 --kernel-trace --stats --output-format csv -d $O/prof -o b -- python3 $R/bench.py --full --steps 5 --warmup 1 --no-cpu-baseline --particles 0 > $O/prof.log 2>&1 && \
rocprofv3 --pmc FETCH_SIZE --kernel-trace --output-format csv -d $O/pmc_fetch -o f -- python3 $R/tools/relax_only.py 8 > $O/pmc_fetch.log 2>&1 && \
rocprofv3 --pmc WRITE_SIZE --kernel-trace --output-format csv -d $O/pmc_write -o w -- python3 $R/tools/relax_only.py 8 > $O/pmc_write.log 2>&1
cd $R && timeout -k 10 300 python bench.py --full > $O/bench.json 2> $O/bench.err
tail -c 400 $O/bench.json
