#!/bin/bash
# scripts/ab_net_store_synth.py (bench / static / dense workloads, full against delta in
# one process) run in turn with several libraries, RUNS rounds of all of them, so that the
# libraries' delta figures can be set side by side: the parent's library against this
# tree's, or this tree's built with several -DGF_NET_COMPACT_MAX.
# One JSON file per run in $OUT/synth/<name>_<round>.json, a table of the per-run medians
# at the end. Every run has its own time limit; the script stops at the first that fails.
# usage: LIBS="parent=build/lib_parent/libgymflock.so new=gym-flock_amd/lib/libgymflock.so ..."
#        [RUNS=2] [OUT=out] [N=1024 B=256 ROUNDS=5 STEPS=30] scripts/ab_synth_libs.sh
set -o pipefail
cd "$(dirname "$0")/.." || exit 1
RUNS=${RUNS:-2}
OUT=${OUT:-out}
export ROUNDS=${ROUNDS:-5}
mkdir -p "$OUT/synth"
for ((i = 0; i < RUNS; ++i)); do
  for kv in ${LIBS:?name=path ...}; do
    GYMFLOCK_LIB=${kv#*=} timeout -k 10 240 python scripts/ab_net_store_synth.py >"$OUT/synth/${kv%%=*}_$i.json" || exit 1
  done
done
python - "$OUT/synth" <<'EOF' | tee "$OUT/synth/report.txt"
import glob, json, os, sys
runs = {}
for p in sorted(glob.glob(os.path.join(sys.argv[1], "*_[0-9]*.json"))):
    runs.setdefault(os.path.basename(p).rsplit("_", 1)[0], []).append(json.load(open(p)))
print("us per step, per run: median (min-max) of the run's rounds")
for w in ("bench", "static", "dense"):
    for mode in ("delta", "full"):
        for name, rs in runs.items():
            print("%-7s %-5s %-8s %s" % (w, mode, name, "  ".join(
                "%.1f (%.1f-%.1f)" % (r[w][mode + "_us"]["median"], r[w][mode + "_us"]["min"], r[w][mode + "_us"]["max"])
                for r in rs)))
    print("%-7s networks identical: %s" % (w, all(r[w]["networks_identical"] for rs in runs.values() for r in rs)))
EOF
