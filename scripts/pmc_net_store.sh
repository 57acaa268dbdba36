#!/bin/bash
# HBM traffic and VALU instructions of the plain step per store mode: one rocprofv3 --pmc
# pass per counter (FETCH_SIZE, WRITE_SIZE, SQ_INSTS_VALU), each a run of its own with no
# tracing beside it, of scripts/pmc_step.py (one launch per step, STEPS launches; a delta
# handle's first launch is the forced full store that fills the record).
# LIBS="name=path ...": libraries to run beside this tree's (parent: GYMFLOCK_NET_STORE
# unset; any other name: with =delta, e.g. another -DGF_NET_GROUP_BYTES).
# COUNTERS="A B ...": the counters (default FETCH_SIZE WRITE_SIZE SQ_INSTS_VALU; any other,
# such as SQ_INSTS_VMEM_WR, is reported beside them). MODES="full delta": which store modes
# of this tree's library to run.
# usage: [N=1024 B=256] [STEPS=6] [OUT=out] [LIBS=...] [COUNTERS=...] [MODES=...] scripts/pmc_net_store.sh
set -o pipefail
cd "$(dirname "$0")/.." || exit 1
OUT=${OUT:-out}
export N=${N:-1024} B=${B:-256} STEPS=${STEPS:-6}
D="$OUT/pmc_net_store_${N}x${B}"
mkdir -p "$D"
pass() {  # name counter env...
  local name=$1 ctr=$2
  shift 2
  env "$@" timeout -k 10 180 rocprofv3 --pmc "$ctr" --output-format csv -d "$D/${name}_$ctr" -o pmc -- \
    python scripts/pmc_step.py >"$D/${name}_$ctr.log" 2>&1
}
export COUNTERS=${COUNTERS:-FETCH_SIZE WRITE_SIZE SQ_INSTS_VALU}
MODES=${MODES-full delta}
NAMES="$MODES"
for ctr in $COUNTERS; do
  for m in $MODES; do pass "$m" "$ctr" "GYMFLOCK_NET_STORE=$m" || exit 1; done
  for kv in $LIBS; do
    name=${kv%%=*}
    if [ "$name" = parent ]; then pass "$name" "$ctr" "GYMFLOCK_LIB=${kv#*=}" || exit 1
    else pass "$name" "$ctr" "GYMFLOCK_LIB=${kv#*=}" GYMFLOCK_NET_STORE=delta || exit 1; fi
  done
done
for kv in $LIBS; do NAMES="$NAMES ${kv%%=*}"; done
python scripts/pmc_net_store_report.py "$D" $NAMES | tee "$D/report.json"
