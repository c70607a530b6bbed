#!/bin/bash
# On the GPU box: MP2 stage GPU tests, smoke, its bench figure, a rocprofv3 kernel trace of it, then the default
# bench.py line (with audio_stage) and the whole GPU suite, in that order of priority (each under its own timeout);
# everything lands in $OUT/<tag>_*.
#   tools/mp2_profile.sh r01f
tag="${1:-rXX}"
ROOT=$(pwd)
OUT="${OUT:-$(pwd)/profile_out}"
mkdir -p "$OUT"
(time timeout 240 python -m pytest tests/test_mp2_gpu.py tests/test_mp2_node_host.py -m gpu -q) > $OUT/${tag}_mp2_pytest.log 2>&1; tail -6 $OUT/${tag}_mp2_pytest.log
(time timeout 200 python -c "import __graft_entry__ as g; g.smoke()") > $OUT/${tag}_smoke.log 2>&1; tail -3 $OUT/${tag}_smoke.log
timeout 120 python tools/mp2_bench.py > $OUT/${tag}_mp2_bench.json 2> $OUT/${tag}_mp2_bench.err || tail -5 $OUT/${tag}_mp2_bench.err
cat $OUT/${tag}_mp2_bench.json
cd /tmp; export TMPDIR=/tmp
rm -rf $OUT/prof_mp2
timeout 200 rocprofv3 --kernel-trace --stats -d $OUT/prof_mp2 -- python $ROOT/tools/mp2_bench.py --reps 20 > $OUT/${tag}_mp2_bench_under_rocprof.json 2> $OUT/${tag}_mp2_rocprof.err
cd $ROOT
find $OUT/prof_mp2 -name "*kernel_stats.csv" -exec cp {} $OUT/${tag}_mp2_kernel_stats.csv \;
head -12 $OUT/${tag}_mp2_kernel_stats.csv
find $OUT/prof_mp2 -name "*kernel_trace.csv" -size +8M -delete
(time timeout 420 python bench.py --full) > $OUT/${tag}_bench.json 2> $OUT/${tag}_bench.err || tail -5 $OUT/${tag}_bench.err
cat $OUT/${tag}_bench.json
(time timeout 900 python -m pytest tests -m gpu -x -q) > $OUT/${tag}_pytest_all.log 2>&1; tail -4 $OUT/${tag}_pytest_all.log
