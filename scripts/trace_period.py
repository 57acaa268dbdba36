"""Per-launch figures of flock_step_kernel from a rocprofv3 --kernel-trace csv of
`python bench.py`: the last 400 launches are the 200 timed steps (two launches per step);
span / 200 steps is the step period the bench measures.
usage: trace_period.py TRACE_DIR LABEL"""
import csv, glob, statistics, sys
paths = glob.glob(sys.argv[1] + "/**/*kernel_trace.csv", recursive=True)
rows = [r for r in csv.DictReader(open(paths[0])) if "flock_step_kernel" in r["Kernel_Name"]]
rows.sort(key=lambda r: int(r["Start_Timestamp"]))
st = [int(r["Start_Timestamp"]) for r in rows]
en = [int(r["End_Timestamp"]) for r in rows]
dur = [e - s for s, e in zip(st, en)]
tail = slice(len(rows) - 400, len(rows))  # the timed window: 200 steps of two launches
gaps = [b - a for a, b in zip(st[tail][:-1], st[tail][1:])]
print("%s: launches %d; last 400: median duration %.1f us, median start-to-start %.1f us, span/200 steps %.1f us, grids %s" % (
    sys.argv[2], len(rows), statistics.median(dur[tail]) / 1e3, statistics.median(gaps) / 1e3,
    (en[-1] - st[tail][0]) / 200e3, sorted({r.get("Grid_Size", r.get("Grid_Size_X", "?")) for r in rows[tail]})))
