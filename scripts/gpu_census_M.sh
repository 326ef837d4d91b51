O=$(realpath -m "${OUT:-records}"); mkdir -p $O; R=$PWD; cd /tmp && export TMPDIR=/tmp
rocprofv3 --kernel-trace -d $O/census${1:-M} -o r -- python $R/scripts/census_config.py ${1:-M} ${2:-bf16} $CENSUS_GEMM > $O/census${1:-M}.log 2>&1
cd $R; python scripts/step_census.py $O/census${1:-M}/r_results.db $3 > $O/census${1:-M}.txt 2>&1; rm -rf $O/census${1:-M}; head -40 $O/census${1:-M}.txt
