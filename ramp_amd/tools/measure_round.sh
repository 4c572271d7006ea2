#!/bin/bash
# The round's evidence in one GPU call: the bench line (with roofline + CPU baseline), the rocprofv3 kernel summary of
# the same command, PMC traffic of one evaluation inside a sampling job, and the other configs' bench lines.
# Usage: OUT=<dir> bash ramp_amd/tools/measure_round.sh [tag]   -> <dir>/<tag>_*
set -e
OUT=${OUT:?set OUT to the directory that receives the results}
mkdir -p "$OUT" && OUT=$(cd "$OUT" && pwd)
cd "$(dirname "$0")/../.."
export TMPDIR=/tmp
T=${1:-round}
python3 bench.py --full > "$OUT/${T}_bench.json" 2> "$OUT/${T}_bench.err"
echo "bench done"
rm -rf "$OUT/${T}_prof"
rocprofv3 --kernel-trace --stats --output-format csv -d "$OUT/${T}_prof" -- python3 bench.py --steps 3 --warmup 1 --no-cpu-baseline --no-roofline > "$OUT/${T}_prof_bench.json" 2> "$OUT/${T}_prof.err"
cp $(find "$OUT/${T}_prof" -name "*kernel_stats.csv" | head -1) "$OUT/${T}_kernel_stats.csv"
rm -rf "$OUT/${T}_prof"
echo "kernel stats done"
rm -rf "$OUT/pmc_sample_fetch" "$OUT/pmc_sample_write"
rocprofv3 --pmc FETCH_SIZE --output-format csv -d "$OUT/pmc_sample_fetch" -- python3 ramp_amd/tools/sample_pmc.py > "$OUT/${T}_pmc_f.log" 2>&1
rocprofv3 --pmc WRITE_SIZE --output-format csv -d "$OUT/pmc_sample_write" -- python3 ramp_amd/tools/sample_pmc.py > "$OUT/${T}_pmc_w.log" 2>&1
python3 ramp_amd/tools/pmc_summary.py "$OUT/pmc_sample_fetch" "$OUT/pmc_sample_write" "$OUT/${T}_pmc_traffic.json" > "$OUT/${T}_pmc_summary.log" 2>&1
rm -rf "$OUT/pmc_sample_fetch" "$OUT/pmc_sample_write"
echo "pmc done"
for c in 3 4 5; do python3 bench.py --config $c --no-cpu-baseline --no-roofline > "$OUT/${T}_bench_c$c.json" 2> "$OUT/${T}_bench_c$c.err"; done
echo "configs done"
