# Round-end evidence on one GPU box: the GPU suite, rocprofv3 kernel statistics, the two HBM-traffic counter passes, the --full bench line.
# (run as: OUT=<dir> bash ramp_amd/tools/final_evidence.sh; results under <dir>/fe_*)
set -e
OUT=${OUT:?set OUT to the directory that receives the results}
mkdir -p "$OUT" && OUT=$(cd "$OUT" && pwd)
cd "$(dirname "$0")/../.."
export TMPDIR=/tmp
timeout -k 10 900 python -m pytest tests -m gpu -q -x > "$OUT/fe_gpu_tests.log" 2>&1
echo tests-done
timeout -k 10 300 rocprofv3 --kernel-trace --stats --output-format csv -d "$OUT/fe_stats" -- python3 bench.py --steps 3 --warmup 1 --no-cpu-baseline --no-other-configs --no-roofline > "$OUT/fe_stats_bench.log" 2>&1
echo stats-done
timeout -k 10 200 rocprofv3 --pmc FETCH_SIZE --output-format csv -d "$OUT/fe_pmc_fetch" -- python3 ramp_amd/tools/sample_pmc.py > "$OUT/fe_pmc_f.log" 2>&1
timeout -k 10 200 rocprofv3 --pmc WRITE_SIZE --output-format csv -d "$OUT/fe_pmc_write" -- python3 ramp_amd/tools/sample_pmc.py > "$OUT/fe_pmc_w.log" 2>&1
python3 ramp_amd/tools/pmc_summary.py "$OUT/fe_pmc_fetch" "$OUT/fe_pmc_write" "$OUT/fe_pmc_traffic.json" > "$OUT/fe_pmc_sum.log" 2>&1
rm -rf "$OUT/fe_pmc_fetch" "$OUT/fe_pmc_write"
find "$OUT/fe_stats" -name '*kernel_stats.csv' -exec cp {} "$OUT/fe_kernel_stats.csv" \;
rm -rf "$OUT/fe_stats"
echo pmc-done
timeout -k 10 400 python bench.py --full > "$OUT/fe_bench.json" 2> "$OUT/fe_bench.err"
tail -c 600 "$OUT/fe_bench.json"
