#!/bin/bash
# kernel traces of the separate-calls step and of the pipelined step (program directly behind `--`), then tools/pipeline_gaps.py
cd /tmp && export TMPDIR=/tmp && cd - > /dev/null
OUT=${OUT:-prof_out}
mkdir -p $OUT
rm -rf $OUT/pg_sep $OUT/pg_pip
rocprofv3 --kernel-trace --output-format csv -d $OUT/pg_sep -- python3 bench.py --full --steps 4 --warmup 2 --separate-calls --no-cpu-baseline --no-logpdf --no-cfg3 --no-host-io > $OUT/pg_sep.json 2> $OUT/pg_sep.err || { tail -3 $OUT/pg_sep.err; exit 1; }
rocprofv3 --kernel-trace --output-format csv -d $OUT/pg_pip -- python3 bench.py --full --steps 4 --warmup 2 --no-cpu-baseline --no-logpdf --no-cfg3 --no-host-io > $OUT/pg_pip.json 2> $OUT/pg_pip.err || { tail -3 $OUT/pg_pip.err; exit 1; }
python3 tools/pipeline_gaps.py $OUT/pg_sep $OUT/pg_pip > $OUT/r06_pipeline_gaps.txt
cat $OUT/r06_pipeline_gaps.txt
