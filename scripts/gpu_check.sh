#!/bin/bash
# Runs on a GPU machine from the repository root: tests, smoke, bench, rocprof kernel trace.  Outputs under $1 (default gpu_check_out/).
set -u
O=${1:-gpu_check_out}
mkdir -p $O
export TMPDIR=/tmp
export HSA_ENABLE_IPC_MODE_LEGACY=0
rocminfo 2>/dev/null | grep -E "Marketing Name|gfx" | head -4 > $O/device.txt
nproc >> $O/device.txt
timeout 1200 python -m pytest tests -q -m gpu > $O/pytest_gpu.log 2>&1; echo "pytest exit $?" >> $O/pytest_gpu.log
tail -25 $O/pytest_gpu.log
timeout 300 python -c "import __graft_entry__ as g; g.smoke()" > $O/smoke.log 2>&1; echo "smoke exit $?" >> $O/smoke.log
tail -3 $O/smoke.log
timeout 600 python bench.py --full --steps 100 --warmup 10 > $O/bench.log 2>&1; echo "bench exit $?" >> $O/bench.log
tail -4 $O/bench.log
rm -rf $O/prof && timeout 600 rocprofv3 --kernel-trace --stats --output-format csv -d $O/prof -o bench -- python bench.py --full --steps 20 --warmup 5 --no-cpu-baseline --kernel-iters 20 > $O/rocprof.log 2>&1
find $O/prof -name "*kernel_stats*" | head -3
f=$(find $O/prof -name "*kernel_stats.csv" | head -1); [ -n "$f" ] && head -12 "$f"
for ctr in FETCH_SIZE WRITE_SIZE; do
  rm -rf $O/pmc_$ctr
  GP_BENCH_CALIBRATE=1 timeout 600 rocprofv3 --pmc $ctr --kernel-trace --output-format csv -d $O/pmc_$ctr -o pmc -- python bench.py --full --steps 5 --warmup 2 --no-cpu-baseline --kernel-iters 5 > $O/pmc_$ctr.log 2>&1
done
ff=$(find $O/pmc_FETCH_SIZE -name "*counter_collection.csv" | head -1); fw=$(find $O/pmc_WRITE_SIZE -name "*counter_collection.csv" | head -1)
[ -n "$ff" ] && [ -n "$fw" ] && python scripts/pmc_summary.py "$ff" "$fw" 1000000 $O/hbm_traffic.json | tee $O/pmc_summary.txt
