#!/bin/bash
# Round 6, GPU job 8 (final HEAD): race hunts (four lanes vs one stream; pipelined vs plain loop), the bench line, small-batch lines.
tag=${1:-r06h}
out=${2:?usage: tools/round6_job8.sh <tag> <output dir>}
mkdir -p $out
python3 tools/stress_bits.py > $out/${tag}_stress_bits.txt 2>&1; tail -2 $out/${tag}_stress_bits.txt
python3 tools/stress_pipeline.py 200 4 > $out/${tag}_stress_pipeline.txt 2>&1; tail -2 $out/${tag}_stress_pipeline.txt
python3 bench.py --full > $out/${tag}_bench_line.json 2> $out/${tag}_bench_line.err
for g in 64 32 16 8; do python3 bench.py --graphs $g --no-cpu-baseline > $out/${tag}_graphs$g.json 2>> $out/${tag}_bench_line.err; done
grep -h -o '"ms_per_step": [0-9.]*' $out/${tag}_bench_line.json $out/${tag}_graphs*.json
python3 tools/check_schedule.py > $out/${tag}_check_schedule.txt 2>&1; tail -1 $out/${tag}_check_schedule.txt
