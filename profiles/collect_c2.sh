#!/bin/bash
# BASELINE configs[1] (64 rows x 10 Mb): the bench line (--full: with the oracle check, aligned rows and CPU baseline) and
# rocprofv3 --kernel-trace --stats of the same steps.
# usage (on the GPU box): profiles/collect_c2.sh <tag> [<out dir>, default profiles/_out]
#   -> <out dir>/bench_<tag>_c2.json, <out dir>/prof_<tag>_c2/
set -e
TAG=${1:-r03}
R=$GRAFT_REPO_ROOT
OUT=$(realpath -m "${2:-$R/profiles/_out}")
mkdir -p "$OUT"
cd /tmp && export TMPDIR=/tmp
python3 $R/bench.py --workload c2 --steps 20 --warmup 3 --full > $OUT/bench_${TAG}_c2.json 2> $OUT/bench_${TAG}_c2.err
rocprofv3 --kernel-trace --stats -d $OUT/prof_${TAG}_c2 -o c2 --output-format csv -- python3 $R/bench.py --workload c2 --steps 20 --warmup 3 --full --cpu-baseline-mb 0 --verify 0 > $OUT/prof_${TAG}_c2.log 2>&1
echo "c2 stats rc=$?"
cut -c1-200 $OUT/bench_${TAG}_c2.json
