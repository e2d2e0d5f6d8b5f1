#!/bin/bash
# Round-3 measurement set (run on the GPU box through gpurun): bench line, rocprofv3 kernel stats, HBM traffic (two PMC passes)
# and an SQ counter pass on the same resident-prove workload. usage: scripts/measure_r03.sh <tag> [pmc]
tag=${1:-r03_a}
set -x
cd $GRAFT_REPO_ROOT
R=$PWD
O=$GRAFT_REPO_ROOT/gpurun_out
python bench.py --full > $O/bench_$tag.json 2> $O/bench_$tag.err
cd /tmp && export TMPDIR=/tmp
rocprofv3 --kernel-trace --stats -d $O/prof_$tag -o runc --output-format csv -- python3 $GRAFT_REPO_ROOT/scripts/prove_once.py 32768 16 6 > $O/prove_once_$tag.txt 2>/dev/null
# the same for the bench command itself (its proves mix the overlapped timed region with one-stream profiling passes) and for
# one-stream proves only (isolated kernel durations)
rocprofv3 --kernel-trace --stats -d $O/profb_$tag -o runc --output-format csv -- python3 $R/bench.py --full --steps 10 --warmup 3 --no-cpu-baseline > $O/bench_${tag}_under_rocprof.json 2>/dev/null
HG_ONE_STREAM=1 rocprofv3 --kernel-trace --stats -d $O/profi_$tag -o runc --output-format csv -- python3 $GRAFT_REPO_ROOT/scripts/prove_once.py 32768 16 6 > /dev/null 2>&1
python3 $GRAFT_REPO_ROOT/scripts/summarize_trace.py $(ls $O/profb_$tag/*kernel_trace.csv | head -1) 60 > $O/${tag}_bench_kernel_trace_summary.txt
python3 $GRAFT_REPO_ROOT/scripts/summarize_trace.py $(ls $O/profi_$tag/*kernel_trace.csv | head -1) 60 > $O/${tag}_one_stream_kernel_trace_summary.txt
rm -rf $O/profb_$tag $O/profi_$tag
if [ "$2" = "pmc" ]; then
rocprofv3 --pmc FETCH_SIZE -d $O/pmc_${tag}_FETCH -o run --output-format csv -- python3 $GRAFT_REPO_ROOT/scripts/prove_once.py 32768 16 2 > /dev/null 2>&1
rocprofv3 --pmc WRITE_SIZE -d $O/pmc_${tag}_WRITE -o run --output-format csv -- python3 $GRAFT_REPO_ROOT/scripts/prove_once.py 32768 16 2 > /dev/null 2>&1
rocprofv3 --pmc SQ_INSTS_VALU SQ_ACTIVE_INST_VALU SQ_WAVE_CYCLES SQ_BUSY_CYCLES SQ_WAIT_ANY SQ_WAIT_INST_ANY SQ_ACTIVE_INST_ANY SQ_WAVES -d $O/pmc_${tag}_SQ -o run --output-format csv -- python3 $GRAFT_REPO_ROOT/scripts/prove_once.py 32768 16 2 > /dev/null 2>&1
fi
cd $GRAFT_REPO_ROOT
python scripts/summarize_trace.py $(ls $O/prof_$tag/*kernel_trace.csv | head -1) 60 > $O/${tag}_kernel_trace_summary.txt
cp $(ls $O/prof_$tag/*kernel_stats.csv | head -1) $O/${tag}_rocprofv3_kernel_stats.csv
if [ "$2" = "pmc" ]; then
python scripts/pmc_summary.py $(ls $O/pmc_${tag}_FETCH/*counter_collection.csv | head -1) $(ls $O/pmc_${tag}_WRITE/*counter_collection.csv | head -1) $O/${tag}_pmc_hbm_traffic.json > $O/${tag}_pmc_hbm_traffic.txt
python scripts/pmc_sq.py $(ls $O/pmc_${tag}_SQ/*counter_collection.csv | head -1) 30 > $O/${tag}_pmc_sq.txt
fi
rm -rf $O/prof_$tag $O/pmc_${tag}_FETCH $O/pmc_${tag}_WRITE $O/pmc_${tag}_SQ
cat $O/bench_$tag.json; head -40 $O/${tag}_kernel_trace_summary.txt
