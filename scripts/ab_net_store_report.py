#!/usr/bin/env python3
"""Report of scripts/ab_net_store.sh: per (window, variant) the runs' ms_per_step, their
median and range, and the acceptance test for making the delta store the default:
every delta run below every parent run, the median difference at least twice the largest
spread of one variant's runs, and full's range overlapping the parent's.

usage: ab_net_store_report.py LOG.jsonl
       ab_net_store_report.py --tag VARIANT WINDOW 'BENCH JSON LINE'   (one tagged log line)"""
import json
import statistics
import sys


def main():
    if sys.argv[1] == "--tag":
        d = json.loads(sys.argv[4])
        print(json.dumps({"variant": sys.argv[2], "window": sys.argv[3], **d}))
        return
    runs = {}
    for ln in open(sys.argv[1]):
        d = json.loads(ln)
        if d["window"] == "warmup":
            continue
        runs.setdefault(d["window"], {}).setdefault(d["variant"], []).append(
            (1e3 * d["ms_per_step"], 1e3 * (d.get("roofline") or {}).get("region_ms_per_step", float("nan"))))
    for window, by in runs.items():
        print("window: %s timed steps" % window)
        stat = {}
        for v, r in by.items():
            us = sorted(x[0] for x in r)
            stat[v] = (statistics.median(us), us[0], us[-1])
            print("  %-7s us/step median %.1f range %.1f-%.1f spread %.1f  runs %s  (device region us/step: %s)" % (
                v, stat[v][0], us[0], us[-1], us[-1] - us[0], " ".join("%.1f" % x for x in us),
                " ".join("%.1f" % x[1] for x in r)))
        if "parent" in stat and "delta" in stat:
            spread = max(s[2] - s[1] for s in stat.values())
            gain = stat["parent"][0] - stat["delta"][0]
            print("  delta vs parent: median difference %.1f us (ratio %.3f), largest spread %.1f us" % (
                gain, stat["parent"][0] / stat["delta"][0], spread))
            print("  every delta run below every parent run: %s" % (stat["delta"][2] < stat["parent"][1]))
            print("  median difference >= 2 x largest spread: %s" % (gain >= 2 * spread))
            print("  median difference / largest spread: %.1f" % (gain / spread if spread > 0 else float("inf")))
            if "full" in stat:
                print("  full overlaps parent: %s" % (stat["full"][1] <= stat["parent"][2]
                                                        and stat["parent"][1] <= stat["full"][2]))


if __name__ == "__main__":
    main()
