#!/bin/bash
# Round profile artifacts (run on the GPU box from the repo root):
#   1) rocprofv3 --kernel-trace --stats of the bench command itself  -> $OUT/stats_<tag>/
#   2) separate --pmc passes (FETCH_SIZE, WRITE_SIZE; MI355X_MICROARCH.md §HBM: never combined
#      with other traces) over tools/kprof.py --lookup                   -> $OUT/hbm_<tag>_*/
#   3) per-kernel HBM bytes per launch                                  -> $OUT/pmc_<tag>/pmc_<kernel>.json
# usage: bash tools/gpu_profile.sh <tag> [bench args]
TAG=$1; shift
R=$PWD; OUT=${HGA_OUT:-bench_out}; mkdir -p $OUT   # HGA_OUT: output folder, relative to the repo root
cd /tmp && export TMPDIR=/tmp
timeout -k 10 400 rocprofv3 --kernel-trace --stats --output-format csv -d $R/$OUT/stats_$TAG -o run -- \
    python3 $R/bench.py --full --steps 10 --warmup 2 --no-cpu --no-scale "$@" > $R/$OUT/stats_$TAG.json 2> $R/$OUT/stats_$TAG.err \
    || { echo "stats run failed"; tail -5 $R/$OUT/stats_$TAG.err; exit 1; }
for p in FETCH_SIZE WRITE_SIZE; do
  timeout -k 10 300 rocprofv3 --kernel-trace --pmc $p --output-format csv -d $R/$OUT/hbm_${TAG}_$p -o run -- \
      python3 $R/tools/kprof.py --reps 2 --lookup --connections --hll > $R/$OUT/hbm_${TAG}_$p.log 2>&1 \
      || { echo "pmc $p failed"; tail -3 $R/$OUT/hbm_${TAG}_$p.log; exit 1; }
done
cd $R && python3 tools/pmc_summary.py $OUT/hbm_${TAG}_* --json $OUT/hbm_$TAG.json > $OUT/hbm_$TAG.txt \
  && python3 tools/make_pmc_json.py $OUT/hbm_$TAG.json $OUT/pmc_$TAG && cat $OUT/hbm_$TAG.txt
