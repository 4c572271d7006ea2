# Config 5's kernel statistics and the --full bench line.   usage: OUT=<dir> bash ramp_amd/tools/config5_evidence.sh  -> <dir>/r06b_*
OUT=${OUT:?set OUT to the directory that receives the results}
mkdir -p "$OUT" && OUT=$(cd "$OUT" && pwd)
cd "$(dirname "$0")/../.."
export TMPDIR=/tmp
timeout -k 10 400 rocprofv3 --kernel-trace --stats --output-format csv -d "$OUT/r06b_stats5" -- python3 bench.py --config 5 --steps 2 --warmup 1 --no-cpu-baseline --no-roofline > "$OUT/r06b_stats5_bench.log" 2>&1
find "$OUT/r06b_stats5" -name '*kernel_stats.csv' -exec cp {} "$OUT/r06b_config5_kernel_stats.csv" \;
rm -rf "$OUT/r06b_stats5"
echo stats5-done
timeout -k 10 500 python bench.py --full > "$OUT/r06b_bench.json" 2> "$OUT/r06b_bench.err"
echo bench-done
tail -c 300 "$OUT/r06b_bench.json"
