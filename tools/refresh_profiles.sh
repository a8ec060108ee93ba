#!/bin/bash
# usage (on the GPU box, from the repo root): bash tools/refresh_profiles.sh r01_f [out_dir, default prof_out]
# bench line with cpu_baseline and roofline (bench.py --full), rocprofv3 kernel stats of the same command, and the two PMC passes for the
# roofline's `traffic`.
set -e
tag=$1
out=${2:-prof_out}
cd "$(dirname "$0")/.."
mkdir -p "$out"
python bench.py --full > "$out/${tag}_bench.json"
echo "bench done"
rocprofv3 --kernel-trace --stats --output-format csv -d "$out/${tag}_prof" -- python bench.py --full --no-cpu-baseline > "$out/${tag}_prof.log" 2>&1
echo "stats done"
rocprofv3 --kernel-trace --pmc FETCH_SIZE --output-format csv -d "$out/${tag}_fetch" -- python bench.py --steps 2 --warmup 1 > "$out/${tag}_fetch.log" 2>&1
echo "fetch done"
rocprofv3 --kernel-trace --pmc WRITE_SIZE --output-format csv -d "$out/${tag}_write" -- python bench.py --steps 2 --warmup 1 > "$out/${tag}_write.log" 2>&1
echo "write done"
stats=$(ls "$out/${tag}_prof"/*/*kernel_stats.csv | head -1)
cp "$stats" "$out/${tag}_bench_kernel_stats.csv"
python tools/prof_summary.py "$out/${tag}_bench_kernel_stats.csv" "$out/${tag}_bench_kernel_stats.md" "${tag}: python bench.py --full --no-cpu-baseline (20 timed + 5 warm-up steps) under rocprofv3 --kernel-trace --stats" 25
python tools/pmc_traffic.py "$out/${tag}_fetch" "$out/${tag}_write" "gemm_nt4dma_kernel<true, true, 0, 0, false, false>" "$out/${tag}_traffic.json" "rocprofv3 --kernel-trace --pmc FETCH_SIZE|WRITE_SIZE -- python bench.py --steps 2 --warmup 1"
tail -c 600 "$out/${tag}_bench.json"
