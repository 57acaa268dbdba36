#!/usr/bin/env python3
"""Per-launch counters of the step kernel from the passes of scripts/pmc_net_store.sh, as
JSON: for every variant the launches' FETCH_SIZE / WRITE_SIZE (KiB), SQ_INSTS_VALU and
the HBM bytes (2 * FETCH_SIZE + WRITE_SIZE) * 1024 (gfx950: FETCH_SIZE reports half the
bytes of a wide read, MI355X_MICROARCH.md, HBM), the first launch (a delta handle's forced
full store) apart from the mean of the others. COUNTERS in the environment (as
pmc_net_store.sh exports it) names the counters that were collected.

usage: pmc_net_store_report.py DIR VARIANT..."""
import csv
import glob
import json
import os
import sys


def launches(d, name, ctr):
    paths = glob.glob(os.path.join(d, "%s_%s" % (name, ctr), "**", "*counter_collection.csv"), recursive=True)
    assert paths, "no counter csv for %s %s" % (name, ctr)
    rows = []
    for r in csv.DictReader(open(paths[0])):
        if r["Counter_Name"] == ctr and "flock_step_kernel" in r["Kernel_Name"]:
            rows.append((int(r.get("Dispatch_Id", len(rows))), r["Kernel_Name"], float(r["Counter_Value"])))
    rows.sort()
    return rows


def main():
    d, names = sys.argv[1], sys.argv[2:]
    out = {}
    for n in names:
        e = {}
        for ctr in os.environ.get("COUNTERS", "FETCH_SIZE WRITE_SIZE SQ_INSTS_VALU").split():
            rows = launches(d, n, ctr)
            vals = [v for _, _, v in rows]
            e["kernel"] = rows[-1][1]
            e[ctr] = {"first_launch": vals[0], "later_mean": sum(vals[1:]) / len(vals[1:]), "later": vals[1:]}
        for k in ("first_launch", "later_mean") if "FETCH_SIZE" in e and "WRITE_SIZE" in e else ():
            e["hbm_bytes_" + k] = (2 * e["FETCH_SIZE"][k] + e["WRITE_SIZE"][k]) * 1024
        out[n] = e
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
