#!/bin/bash
# Round-1 measurement set: bench line, rocprofv3 kernel stats of the bench command, HBM traffic (two PMC passes).
# usage: scripts/measure_set.sh <output directory>
set -x
R=$(cd "$(dirname "$0")/.." && pwd)
mkdir -p "$1" && O=$(cd "$1" && pwd) || exit 1
cd "$R"
python bench.py --full > $O/bench_r01j.json 2> $O/bench_r01j.err
cd /tmp && export TMPDIR=/tmp
rocprofv3 --kernel-trace --stats -d $O/prof_r1j -o runc --output-format csv -- python3 $R/bench.py --full --steps 10 --warmup 3 --no-cpu-baseline > $O/bench_r01j_prof.json 2>/dev/null
rocprofv3 --pmc FETCH_SIZE -d $O/pmc_j_FETCH -o run --output-format csv -- python3 $R/scripts/prove_once.py 32768 16 2 > /dev/null 2>&1
rocprofv3 --pmc WRITE_SIZE -d $O/pmc_j_WRITE -o run --output-format csv -- python3 $R/scripts/prove_once.py 32768 16 2 > /dev/null 2>&1
cd "$R"
python scripts/summarize_trace.py $(ls $O/prof_r1j/*kernel_trace.csv | head -1) 50 > $O/prof_r1j_summary.txt
python scripts/pmc_summary.py $(ls $O/pmc_j_FETCH/*counter_collection.csv | head -1) $(ls $O/pmc_j_WRITE/*counter_collection.csv | head -1) $O/pmc_r01j.json > $O/pmc_r01j.txt
cp $(ls $O/prof_r1j/*kernel_stats.csv | head -1) $O/prof_r1j_kernel_stats.csv
rm -rf $O/prof_r1j $O/pmc_j_FETCH $O/pmc_j_WRITE
cat $O/bench_r01j.json; head -12 $O/pmc_r01j.txt
