#!/bin/bash
# rocprofv3 kernel trace of a short eager bench; summary -> $OUT/<name>.stats.txt (OUT default: records)
NAME=${1:-prof}
shift
O=$(realpath -m "${OUT:-records}")
mkdir -p $O
R=$PWD
cd /tmp && export TMPDIR=/tmp
rocprofv3 --kernel-trace --stats -d $O/$NAME -o r -- python $R/bench.py --steps 5 --warmup 2 --no-graph --skip-cpu-baseline "$@" > $O/$NAME.log 2>&1
cd $R
python scripts/rocpd_stats.py $O/$NAME/r_results.db 60 > $O/$NAME.stats.txt 2>&1
python scripts/rocpd_seq.py $O/$NAME/r_results.db 300 60 > $O/$NAME.seq.txt 2>&1; rm -rf $O/$NAME
grep '"metric"' $O/$NAME.log | head -1
