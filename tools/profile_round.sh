#!/bin/bash
# usage (on the GPU box, from the repo root): tools/profile_round.sh <tag>      e.g. r01_v6
# Produces <out>/<tag>_bench_kernel_stats.csv, <out>/<tag>_pmc_fetch_write.json, <out>/<tag>_bench.json with
# <out> = $PROFILE_OUT (default: profile_out/ in the repo root); copy them into profiles/.  Counters are collected in their
# own passes (no tracing flags next to --pmc).  Every bench.py run here is a --full one: the roofline probes are part of what
# is profiled, and the committed PMC summary is what --full's roofline.traffic reads.
TAG=${1:-rXX}
R=${GRAFT_REPO_ROOT:-$PWD}
O=${PROFILE_OUT:-$R/profile_out}
mkdir -p $O
cd /tmp && export TMPDIR=/tmp
rocprofv3 --kernel-trace --stats --output-format csv -d $O/prof_$TAG -o bench -- \
  python $R/bench.py --full --no-cpu-baseline --no-secondary > $O/prof_$TAG.log 2>&1
for c in FETCH_SIZE WRITE_SIZE; do
  rocprofv3 --pmc $c --output-format csv -d $O/pmc_${TAG}_$c -o b -- \
    python $R/bench.py --full --steps 1 --warmup 0 --no-cpu-baseline --no-secondary --spmm-reps 5 > $O/pmc_${TAG}_$c.log 2>&1
done
cd $R
python tools/summarize_prof.py stats $O/prof_$TAG $O/${TAG}_bench_kernel_stats.csv
python tools/summarize_prof.py pmc $O/${TAG}_pmc_fetch_write.json \
  FETCH_SIZE=$O/pmc_${TAG}_FETCH_SIZE WRITE_SIZE=$O/pmc_${TAG}_WRITE_SIZE
cp $O/${TAG}_pmc_fetch_write.json profiles/  # bench.py --full reads roofline.traffic from the newest committed summary
python bench.py --full 2>/dev/null | tail -1 > $O/${TAG}_bench.json   # the driver's line (<= 6 KB)
cp bench_detail.json $O/${TAG}_bench_detail.json                      # everything measured (the DETAIL line)
rm -rf $O/prof_$TAG $O/pmc_${TAG}_FETCH_SIZE $O/pmc_${TAG}_WRITE_SIZE
head -12 $O/${TAG}_bench_kernel_stats.csv | cut -c1-150
python -c "
import json; j=json.load(open('$O/${TAG}_pmc_fetch_write.json'))
for k in j:
    for kk,v in j[k].items():
        if 'tcg' in kk or 'spmm' in kk: print(k, kk, v)
print(open('$O/${TAG}_bench.json').read()[:300])"
