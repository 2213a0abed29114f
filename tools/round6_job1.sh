#!/bin/bash
# Round 6, first GPU job: the suite at HEAD (order-point fix of the pipelined v2 schedule), the bench line, the pipelined-loop race hunt,
# the scaling prediction from real shares and the HIP half of the 32-graph x 1000-step match-rate record.
tag=${1:-r06a}
out=${2:?usage: tools/round6_job1.sh <tag> <output dir>}
mkdir -p $out
python3 -m pytest tests -m gpu -x -q 2>&1 | tail -8 > $out/${tag}_pytest.txt
python3 bench.py --full > $out/${tag}_bench_line.json 2> $out/${tag}_bench_line.err
python3 tools/stress_pipeline.py > $out/${tag}_stress_pipeline.txt 2>&1
python3 tools/predict_scaling.py > $out/${tag}_predicted_scaling.txt 2>&1
python3 tools/match_rate.py hip 1000 32 > $out/${tag}_match_rate_hip.json 2> $out/${tag}_match_rate_hip.err
tail -3 $out/${tag}_pytest.txt; cat $out/${tag}_bench_line.json | cut -c1-400; tail -2 $out/${tag}_stress_pipeline.txt
grep predicted $out/${tag}_predicted_scaling.txt; cut -c1-600 $out/${tag}_match_rate_hip.json; tail -3 $out/${tag}_match_rate_hip.err
