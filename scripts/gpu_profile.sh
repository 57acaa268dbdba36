#!/bin/bash
# Bench + rocprofv3 kernel trace + PMC traffic passes for the bench workload.
# Outputs go to $OUT (default: out/).
cd "${GRAFT_REPO_ROOT:-$(dirname "$0")/..}"
OUT=${OUT:-out}
mkdir -p "$OUT"; export TMPDIR=/tmp
set -o pipefail
timeout -k 10 600 python bench.py --full > $OUT/bench.log 2> $OUT/bench.err && cat $OUT/bench.log &&
timeout -k 10 600 rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/prof_trace -o trace -- python bench.py --full --steps 100 --warmup 10 --no-cpu-baseline --no-packed-line --no-knn-line > $OUT/rocprof_trace.log 2>&1 &&
timeout -k 10 300 rocprofv3 --pmc FETCH_SIZE --output-format csv -d $OUT/pmc_fetch -o pmc -- python scripts/pmc_step.py > $OUT/pmc_fetch.log 2>&1 &&
timeout -k 10 300 rocprofv3 --pmc WRITE_SIZE --output-format csv -d $OUT/pmc_write -o pmc -- python scripts/pmc_step.py > $OUT/pmc_write.log 2>&1 &&
N=8192 B=32 timeout -k 10 300 python bench.py --full --n-agents 8192 --n-envs 32 --steps 20 --warmup 3 --no-cpu-baseline --no-knn-line > $OUT/bench_n8192.log 2>&1 && cat $OUT/bench_n8192.log &&
timeout -k 10 300 python bench.py --workload coverage --steps 50 --warmup 5 > $OUT/bench_coverage.log 2> $OUT/bench_coverage.err && cat $OUT/bench_coverage.log &&
timeout -k 10 300 rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/prof_cov -o cov -- python bench.py --workload coverage --steps 50 --warmup 5 --no-cpu-baseline > $OUT/rocprof_cov.log 2>&1 &&
timeout -k 10 300 rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/prof_knn -o knn -- python scripts/time_knn.py > $OUT/rocprof_knn.log 2>&1 &&
python scripts/knn_trace.py $OUT/prof_knn/knn_kernel_trace.csv
echo "rc=$?"
