#!/bin/bash
# Cross-build A/B of the bench lines: bench.py --full (driver window: 20 steps after 5
# warm-up steps, no CPU baseline) alternating HEAD's library (build/lib_old) and the
# working tree's (or NEWLIB's), ROUNDS times; one JSON line per run into
# $OUT/ab_bench_{old,new}.jsonl (OUT defaults to out/).
set -e
OUT=${OUT:-out}
mkdir -p "$OUT"
: > $OUT/ab_bench_old.jsonl
: > $OUT/ab_bench_new.jsonl
for i in $(seq ${ROUNDS:-2}); do
  GYMFLOCK_LIB=$PWD/build/lib_old/libgymflock.so timeout -k 10 300 python bench.py --full --steps 20 --warmup 5 --no-cpu-baseline "$@" >> $OUT/ab_bench_old.jsonl
  GYMFLOCK_LIB=${NEWLIB:-$PWD/gym-flock_amd/lib/libgymflock.so} timeout -k 10 300 python bench.py --full --steps 20 --warmup 5 --no-cpu-baseline "$@" >> $OUT/ab_bench_new.jsonl
done
python scripts/ab_bench_report.py $OUT/ab_bench_old.jsonl $OUT/ab_bench_new.jsonl
