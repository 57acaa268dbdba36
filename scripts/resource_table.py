#!/usr/bin/env python3
"""Condense hipcc's -Rpass-analysis=kernel-resource-usage remarks (stderr of a compile of
gym-flock_amd/csrc/flock_kernels.hip) into one line per kernel, sorted by name:

    kernel<template arguments>  VGPRs  AGPRs  scratch  occupancy  LDS  SGPRs  spills

usage: resource_table.py LISTING [--drop-last-arg]
--drop-last-arg removes the step kernel's last template argument (DN, added with the delta
network store; false for every instantiation that existed before), so that the listing
can be compared line by line with one made before the argument existed."""
import re
import sys


def main():
    path = sys.argv[1]
    drop = "--drop-last-arg" in sys.argv[2:]
    rows, cur = [], None
    for ln in open(path):
        m = re.search(r"remark: (?:\S+:\d+:\d+: )?(.+?): (.+?) \[-Rpass-analysis", ln)
        if not m:
            continue
        key, val = m.group(1).strip(), m.group(2).strip()
        if key == "Function Name":
            cur = {"name": val}
            rows.append(cur)
        elif cur is not None:
            cur[key] = val
    out = []
    for r in rows:
        name = r["name"]
        m = re.match(r"_ZN2gf12_GLOBAL__N_1(\d+)", name)
        if m:
            n = int(m.group(1))
            rest = name[len(m.group(0)):]
            kern, rest = rest[:n], rest[n:]
            args = []
            if rest.startswith("I"):
                for a in re.findall(r"L([bi])(\d+)E", rest.split("EEv")[0] + "E"):
                    args.append(a[1])
            if drop and kern == "flock_step_kernel" and len(args) == 9:
                if args[-1] != "0":
                    kern += "[DN]"
                args = args[:-1]
            name = kern + ("<" + ",".join(args) + ">" if args else "")
        out.append("%-46s VGPRs %3s AGPRs %s scratch %s occupancy %s LDS %s SGPRs %s spills %s/%s" % (
            name, r.get("VGPRs"), r.get("AGPRs"), r.get("ScratchSize [bytes/lane]"), r.get("Occupancy [waves/SIMD]"),
            r.get("LDS Size [bytes/block]"), r.get("TotalSGPRs"), r.get("SGPRs Spill"), r.get("VGPRs Spill")))
    print("\n".join(sorted(out)))


if __name__ == "__main__":
    main()
