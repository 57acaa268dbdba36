#!/bin/bash
# HBM traffic and VALU instructions of the plain step per store mode: one rocprofv3 --pmc
# pass per counter (FETCH_SIZE, WRITE_SIZE, SQ_INSTS_VALU), each a run of its own with no
# tracing beside it, of scripts/pmc_step.py (one launch per step, STEPS launches; a delta
# handle's first launch is the forced full store that fills the record).
# LIBS="name=path ...": libraries to run beside this tree's (parent: GYMFLOCK_NET_STORE
# unset; any other name: with =delta, e.g. another -DGF_NET_GROUP_BYTES).
# usage: [N=1024 B=256] [STEPS=6] [OUT=out] [LIBS=...] scripts/pmc_net_store.sh
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
NAMES="full delta"
for ctr in FETCH_SIZE WRITE_SIZE SQ_INSTS_VALU; do
  pass full "$ctr" GYMFLOCK_NET_STORE=full || exit 1
  pass delta "$ctr" GYMFLOCK_NET_STORE=delta || exit 1
  for kv in $LIBS; do
    name=${kv%%=*}
    if [ "$name" = parent ]; then pass "$name" "$ctr" "GYMFLOCK_LIB=${kv#*=}" || exit 1
    else pass "$name" "$ctr" "GYMFLOCK_LIB=${kv#*=}" GYMFLOCK_NET_STORE=delta || exit 1; fi
  done
done
for kv in $LIBS; do NAMES="$NAMES ${kv%%=*}"; done
python scripts/pmc_net_store_report.py "$D" $NAMES | tee "$D/report.json"
