#!/bin/bash
# Regenerates the evidence under profiles/ on a GPU box (run from the repo root; outputs under $OUT, default prof_out/):
#   1. the default bench line                       -> $OUT/fp_line.json
#   2. rocprofv3 --kernel-trace --stats of bench.py -> $OUT/fp_trace/ (+ per-step summary)
#   3. two PMC passes (FETCH_SIZE, WRITE_SIZE), each in its own run, no tracing flags besides the counters
# Copy afterwards (on the build machine): see the cp lines at the end of this script's output.
set -e
cd /tmp && export TMPDIR=/tmp && cd - > /dev/null
OUT=${OUT:-prof_out}
mkdir -p $OUT
R=${1:-r01}
python3 bench.py --full --extras > $OUT/fp_line.json 2> $OUT/fp_line.err
echo "bench line done"
rm -rf $OUT/fp_trace $OUT/pmc_fetch $OUT/pmc_write
rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/fp_trace -- python3 bench.py --full --steps 5 --warmup 2 --no-cpu-baseline --no-logpdf --no-cfg3 --no-host-io > $OUT/fp_trace.json 2> $OUT/fp_trace.err
python3 tools/prof_summary.py $OUT/fp_trace 12 > $OUT/fp_summary.txt      # 2 warm-up + 5 pipelined + 5 separate-call steps
cp $(ls -t $OUT/fp_trace/*/*kernel_stats.csv | head -1) $OUT/fp_kernel_stats.csv
echo "kernel trace done"
rocprofv3 --pmc FETCH_SIZE -d $OUT/pmc_fetch --output-format csv -- python3 bench.py --full --steps 1 --warmup 1 --no-cpu-baseline --no-logpdf --no-cfg3 --no-host-io > /dev/null 2> $OUT/pmc_fetch.err
echo "pmc fetch done"
rocprofv3 --pmc WRITE_SIZE -d $OUT/pmc_write --output-format csv -- python3 bench.py --full --steps 1 --warmup 1 --no-cpu-baseline --no-logpdf --no-cfg3 --no-host-io > /dev/null 2> $OUT/pmc_write.err
echo "pmc write done"
python3 tools/pmc_traffic.py $OUT/pmc_fetch $OUT/pmc_write $OUT/fp_pmc_traffic.json 1000 64
cp $(ls -t $OUT/pmc_fetch/*/*counter_collection.csv | head -1) $OUT/fp_pmc_fetch_size.csv
cp $(ls -t $OUT/pmc_write/*/*counter_collection.csv | head -1) $OUT/fp_pmc_write_size.csv
rm -rf $OUT/fp_trace/*/*kernel_trace.csv.bak
head -12 $OUT/fp_summary.txt
tail -c 700 $OUT/fp_line.json
