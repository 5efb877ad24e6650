#!/bin/bash
# Collect PMC counters for the bench in separate passes (rocprofv3 --pmc with --kernel-trace only).
# usage: bash tools/pmc.sh TAG "CTR1 CTR2 ..." "CTR..." ...   (on an MI355X, from the repo root)
# Output under $PROFILE_OUT (default profile_out/ in the repo root).
tag=$1; shift
root=$(cd "$(dirname "$0")/.." && pwd)
out=${PROFILE_OUT:-$root/profile_out}
mkdir -p $out
cd /tmp && export TMPDIR=/tmp
i=0
for set in "$@"; do
  i=$((i+1))
  timeout -k 5 150 rocprofv3 --kernel-trace --pmc $set -d $out/${tag}_$i -o run --output-format csv -- \
      python3 $root/bench.py --full --steps 1 --warmup 1 --check 0 --cpu-reads 0 > $out/${tag}_$i.log 2>&1 || exit 1
done
python3 $root/tools/pmc_sum.py $out/${tag}_*/ > $out/${tag}_summary.txt
cat $out/${tag}_summary.txt
