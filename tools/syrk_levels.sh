#!/bin/bash
# per-launch durations of the contribution-block SYRK for two settings of an environment variable
cd /tmp && export TMPDIR=/tmp && cd - > /dev/null
var=$1; shift
OUT=${OUT:-prof_out}      # traces and per-launch tables
mkdir -p $OUT
for v in "$@"; do
  export $var=$v
  rocprofv3 --kernel-trace --output-format csv -d $OUT/sl_$v -- python3 bench.py --full --no-cpu-baseline --steps 3 --warmup 2 --no-logpdf --no-cfg3 > $OUT/sl_$v.json 2> $OUT/sl_$v.err || { tail -5 $OUT/sl_$v.err; exit 1; }
  python3 tools/timeline.py $OUT/sl_$v 0 | grep syrk > $OUT/sl_$v.txt
  echo "== $var=$v"; cat $OUT/sl_$v.txt
done
