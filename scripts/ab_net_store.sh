#!/bin/bash
# Interleaved A/B of the headline bench line: the parent commit's library (PARENT_LIB, a
# libgymflock.so built from it) against this tree's library with GYMFLOCK_NET_STORE=full
# and =delta. One warm-up run of each first, then RUNS rounds of every variant, for the
# default window (200 timed steps) and for --steps 20. One JSON line per run goes to
# $OUT/ab_net_store.jsonl (the bench line plus "variant" and "window"); every run has its
# own time limit and the script stops at the first run that fails.
# EXTRA_LIBS="name=path ...": further libraries of this tree (built with another
# -DGF_NET_GROUP_BYTES), each run with GYMFLOCK_NET_STORE=delta beside the others.
# usage: PARENT_LIB=build/lib_parent/libgymflock.so [RUNS=5] [OUT=out] [VARIANTS="parent full delta"]
#        [EXTRA_LIBS=...] [WINDOWS="200 20"] scripts/ab_net_store.sh
set -o pipefail
cd "$(dirname "$0")/.." || exit 1
RUNS=${RUNS:-5}
OUT=${OUT:-out}
VARIANTS=${VARIANTS:-parent full delta}
WINDOWS=${WINDOWS:-200 20}
mkdir -p "$OUT"
LOG="$OUT/ab_net_store.jsonl"
: > "$LOG"
declare -A LIBS
for kv in $EXTRA_LIBS; do
  LIBS[${kv%%=*}]=${kv#*=}
  VARIANTS="$VARIANTS ${kv%%=*}"
done

run() {  # variant window
  local variant=$1 window=$2 steps=$2 line
  [ "$window" = warmup ] && steps=20
  local -a envs
  case $variant in
    parent) envs=("GYMFLOCK_LIB=${PARENT_LIB:?set it to the parent commit libgymflock.so}") ;;
    full) envs=(GYMFLOCK_NET_STORE=full) ;;
    delta) envs=(GYMFLOCK_NET_STORE=delta) ;;
    *) envs=("GYMFLOCK_LIB=${LIBS[$variant]:?no library for variant $variant}" GYMFLOCK_NET_STORE=delta) ;;
  esac
  line=$(env "${envs[@]}" timeout -k 10 180 python bench.py --gpus 1 --steps "$steps" 2>>"$OUT/ab_net_store.err" | tail -1) || return 1
  [ -n "$line" ] || return 1
  python scripts/ab_net_store_report.py --tag "$variant" "$window" "$line" >>"$LOG"
}

for v in $VARIANTS; do run "$v" warmup || exit 1; done
for ((i = 0; i < RUNS; ++i)); do
  for w in $WINDOWS; do
    for v in $VARIANTS; do run "$v" "$w" || exit 1; done
  done
done
python scripts/ab_net_store_report.py "$LOG" | tee "$OUT/ab_net_store_report.txt"
