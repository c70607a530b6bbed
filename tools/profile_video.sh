#!/bin/bash
# On the GPU box: the three rocprofv3 passes of bench.py (kernel trace + stats, FETCH_SIZE, WRITE_SIZE; separate passes)
# and their summary -> $OUT/<tag>_summary.txt, profiles/<tag>_kernel_stats.txt, <tag>_pmc.txt, pmc_traffic.json
# (tools/profile_round.sh without the test and bench runs).     tools/profile_video.sh r01o
tag="${1:-rXX}"
ROOT=$(pwd)
OUT="${OUT:-$(pwd)/profile_out}"
mkdir -p "$OUT"
cd /tmp; export TMPDIR=/tmp
rm -rf $OUT/prof_trace $OUT/prof_fetch $OUT/prof_write
rocprofv3 --kernel-trace --stats -d $OUT/prof_trace -- python $ROOT/bench.py --full --steps 5 --warmup 1 --no-cpu-baseline --no-audio > $OUT/${tag}_bench_under_rocprof.json 2> $OUT/${tag}_rocprof_trace.err
rocprofv3 --kernel-trace --pmc FETCH_SIZE -d $OUT/prof_fetch -- python $ROOT/bench.py --full --steps 2 --warmup 1 --no-cpu-baseline --no-audio > /dev/null 2> $OUT/${tag}_rocprof_fetch.err
rocprofv3 --kernel-trace --pmc WRITE_SIZE -d $OUT/prof_write -- python $ROOT/bench.py --full --steps 2 --warmup 1 --no-cpu-baseline --no-audio > /dev/null 2> $OUT/${tag}_rocprof_write.err
cd $ROOT
python tools/rocprof_summary.py $tag $OUT/prof_trace $OUT/prof_fetch $OUT/prof_write > $OUT/${tag}_summary.txt 2>&1; tail -30 $OUT/${tag}_summary.txt
mkdir -p $OUT/profiles_out; cp profiles/${tag}_* profiles/pmc_traffic.json $OUT/profiles_out/ 2>/dev/null
