# Round evidence on one GPU box: rocprofv3 kernel statistics of the bench command (config 2) and of config 5's shard, the per-kernel counter
# passes (pmc_round.sh), the --full bench line.   usage: OUT=<dir> bash ramp_amd/tools/round_evidence.sh r05  -> <dir>/r05_*
OUT=${OUT:?set OUT to the directory that receives the results}
mkdir -p "$OUT" && OUT=$(cd "$OUT" && pwd)
cd "$(dirname "$0")/../.."
export TMPDIR=/tmp
T=${1:-r05}
timeout -k 10 300 rocprofv3 --kernel-trace --stats --output-format csv -d "$OUT/${T}_stats" -- python3 bench.py --steps 3 --warmup 1 --no-cpu-baseline --no-other-configs --no-roofline > "$OUT/${T}_stats_bench.log" 2>&1
find "$OUT/${T}_stats" -name '*kernel_stats.csv' -exec cp {} "$OUT/${T}_kernel_stats.csv" \;
rm -rf "$OUT/${T}_stats"
echo stats-done
timeout -k 10 300 rocprofv3 --kernel-trace --stats --output-format csv -d "$OUT/${T}_stats5" -- python3 bench.py --config 5 --steps 2 --warmup 1 --no-cpu-baseline --no-roofline > "$OUT/${T}_stats5_bench.log" 2>&1
find "$OUT/${T}_stats5" -name '*kernel_stats.csv' -exec cp {} "$OUT/${T}_config5_kernel_stats.csv" \;
rm -rf "$OUT/${T}_stats5"
echo stats5-done
OUT="$OUT" bash ramp_amd/tools/pmc_round.sh ${T} > "$OUT/${T}_pmc_tail.txt" 2>&1
echo pmc-done
timeout -k 10 400 python bench.py --full > "$OUT/${T}_bench.json" 2> "$OUT/${T}_bench.err"
echo bench-done
tail -c 400 "$OUT/${T}_bench.json"
