#!/bin/bash
# The round's measurement set (on the GPU box): the full bench line, the sustained 1000-step line, the small-batch lines (one GPU's
# share of the headline batch on 2 / 4 / 8 GPUs), config 2, the training step; everything lands in <output dir>/<tag>_*.
#   usage: tools/measure_round.sh <tag> <output dir>
tag=${1:-r04}
out=${2:?usage: tools/measure_round.sh <tag> <output dir>}
mkdir -p $out
python3 bench.py --full > $out/${tag}_bench_line.json 2> $out/${tag}_bench_line.err
python3 bench.py --steps 1000 --warmup 0 --repeats 1 --no-cpu-baseline > $out/${tag}_bench_1000steps.json 2>> $out/${tag}_bench_line.err
for g in 64 32 16 8; do
  python3 bench.py --graphs $g --no-cpu-baseline > $out/${tag}_graphs$g.json 2>> $out/${tag}_bench_line.err
done
python3 tools/bench_config2.py > $out/${tag}_config2_sample100.json 2>> $out/${tag}_bench_line.err
python3 tools/bench_train.py --steps 10 --warmup 2 > $out/${tag}_train_bench_line.json 2>> $out/${tag}_bench_line.err
grep -h -o '"ms_per_step": [0-9.]*' $out/${tag}_bench_line.json $out/${tag}_bench_1000steps.json $out/${tag}_graphs*.json
tail -c 400 $out/${tag}_config2_sample100.json; tail -c 300 $out/${tag}_train_bench_line.json
