#!/bin/bash
# eager train-step census: kernels of one step (between two adam launches) -> $OUT/census.txt (OUT default: records)
O=$(realpath -m "${OUT:-records}"); mkdir -p $O; R=$PWD; cd /tmp && export TMPDIR=/tmp
rocprofv3 --kernel-trace -d $O/census -o r -- python $R/bench.py --steps 4 --warmup 2 --no-graph --skip-cpu-baseline --no-alt "$@" > $O/census.log 2>&1
cd $R; python scripts/step_census.py $O/census/r_results.db --seq > $O/census.txt 2>&1; rm -rf $O/census; cat $O/census.txt
