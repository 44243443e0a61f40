#!/bin/bash
# Sample power / clocks while the bench runs (evidence for the power-limited regime):  bash tools/clock_probe.sh <out dir>
O=${1:?usage: tools/clock_probe.sh <out dir>}; mkdir -p "$O"
python bench.py --full --steps 150 --warmup 15 --no-cpu-baseline > "$O/bench_clk.json" 2>/dev/null &
BP=$!
sleep 6
for i in $(seq 1 8); do amd-smi metric -g 0 --power --clock 2>/dev/null | grep -E "SOCKET_POWER|GFX_0|CLK:|MIN_CLK|MAX_CLK|CLK_LOCKED|DEEP_SLEEP|THROTTLE" | head -12 | tr '\n' ' ' | sed 's/  */ /g'; echo; sleep 0.5; done > "$O/clocks.txt"
wait $BP
cat "$O/clocks.txt"
amd-smi static -g 0 --limit 2>/dev/null | grep -iE "power|cap" | head -8
python -c "import json, sys; d=json.load(open(sys.argv[1])); print(d['value'], d['ms_per_step'], d['roofline']['achieved'])" "$O/bench_clk.json"
