"""Time of the Coverage reset on the device (cov_reset_device) and what it costs the rest.

Writes profiles/cov_reset/cov_reset_timing.json (or --out): recorded figures, nothing is
asserted. Without --part the script touches no GPU itself: it runs each part as a child
process under its own `timeout` and stops at the first part that fails or runs out of time.
Device figures are host-clock times of calls that end synchronised, after a warm-up call.

  m  512 CoverageARL envs (R=4, max_nodes 1000, maps sampled from tests/golden/grid_slice10.npy):
       masked   8 of 512 envs reset, streams continued: uniform starts (nearby = 0), the
                nearby_starts region (nearby = 20), and the region after a new map for the 8
                (COV_RESET_NEW_MAPS)
       all      every env: cov_reset_device seeded with nearby = 0 (cov_reset_seeded's draws)
                and continued with nearby = 20, against cov_reset_seeded
  d  the drop-in CoverageARLEnv.reset() (a new sampled map each time) with
     reset_mode="reference" (the region grown by a Python set loop over the motion edges)
     and reset_mode="device"
  ab with --parent-lib PATH (a libgymflock.so built from the parent commit): that library
     and this tree's, interleaved on one box in child processes: `bench.py --workload
     coverage` (robot-steps/s) and cov_reset_seeded for 512 envs. Recorded: every run, the
     gap between the two builds' medians and the spread of the parent's own runs.

Usage:  python scripts/cov_reset_timing.py [--out PATH] [--repeats 20] [--parent-lib PATH] [--rounds 3]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "gym-flock_amd")]

PART_TIMEOUT = {"m": 240, "d": 240, "s": 120}  # seconds, each part's own limit
BENCH_TIMEOUT = 300
GRID = os.path.join(ROOT, "tests", "golden", "grid_slice10.npy")
B, R, M = 512, 4, 1000


def timed(run, repeats):
    """Median / min / max milliseconds of run() (which ends synchronised), after one warm-up."""
    run()
    ts = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        run()
        ts.append(1e3 * (time.perf_counter() - t0))
    return {"ms": statistics.median(ts), "min_ms": min(ts), "max_ms": max(ts), "repeats": repeats}


def arl_handle():
    from gym_flock import _native as nat
    h = nat.CoverageHandle(R, B, M, 50, 5.0)
    h.load_occupancy(np.load(GRID))
    n, _, _ = h.generate_submaps(map_seed=0)
    return h, n


def part_m(repeats):
    h, n = arl_handle()
    out = {"n_envs": B, "n_robots": R, "max_nodes": M, "targets_min_mean_max": [int(n.min()), float(n.mean()), int(n.max())]}
    bufs = (np.zeros((B, R), np.int32), np.zeros((B, M - R), np.uint8), np.zeros((B, M - R), np.uint8),
            np.zeros(B, np.int32))
    h.reset_seeded(0, 0.5)
    mask = np.zeros(B, bool)
    mask[::64] = True
    out["masked_8_of_512"] = {
        "uniform": timed(lambda: h.reset_device(mask, 0.5, 0, out=bufs), repeats),
        "nearby_20": timed(lambda: h.reset_device(mask, 0.5, 5 * R, out=bufs), repeats),
        "nearby_20_new_maps": timed(lambda: h.reset_device(mask, 0.5, 5 * R, new_maps=True, out=bufs), repeats),
    }
    h.generate_submaps(map_seed=0)
    out["all_512"] = {
        "cov_reset_seeded": timed(lambda: h.reset_seeded(0, 0.5), repeats),
        "reset_device_seeded_uniform": timed(lambda: h.reset_device(None, 0.5, 0, seed=0, out=bufs), repeats),
        "reset_device_continued_nearby_20": timed(lambda: h.reset_device(None, 0.5, 5 * R, out=bufs), repeats),
        "reset_device_continued_nearby_20_no_outputs": timed(
            lambda: h.reset_device(None, 0.5, 5 * R, out=(None, None, None, None)), repeats),
    }
    h.close()
    return out


def part_d(repeats):
    from gym_flock.envs.spatial import CoverageARLEnv
    grid = np.load(GRID)
    out = {}
    for mode in ("reference", "device"):
        np.random.seed(0)
        env = CoverageARLEnv(occupancy=grid, reset_mode=mode)
        env.seed(1)
        out[mode] = timed(env.reset, repeats)
        env.close()
    return out


def part_s(repeats):
    """cov_reset_seeded for 512 envs with whichever library GYMFLOCK_LIB names (the A/B)."""
    h, _ = arl_handle()
    out = timed(lambda: h.reset_seeded(0, 0.5, fetch=False) or h.sync(), 5 * repeats)
    h.close()
    return out


def child(part, repeats, env=None):
    cmd = ["timeout", "-k", "10", str(PART_TIMEOUT[part]), sys.executable, os.path.abspath(__file__), "--part", part,
           "--repeats", str(repeats)]
    p = subprocess.run(cmd, stdout=subprocess.PIPE, env=env)
    if p.returncode != 0:
        raise SystemExit("part %s ended with status %d: stopping" % (part, p.returncode))
    return json.loads(p.stdout.decode().strip().splitlines()[-1])


def bench(env):
    cmd = ["timeout", "-k", "10", str(BENCH_TIMEOUT), sys.executable, os.path.join(ROOT, "bench.py"), "--workload",
           "coverage", "--gpus", "1", "--steps", "200", "--warmup", "20", "--no-cpu-baseline"]
    p = subprocess.run(cmd, stdout=subprocess.PIPE, env=env)
    if p.returncode != 0:
        raise SystemExit("bench.py ended with status %d: stopping" % p.returncode)
    line = [ln for ln in p.stdout.decode().splitlines() if ln.startswith("{")][-1]
    return json.loads(line)["value"]


def part_ab(parent_lib, rounds, repeats):
    envs = {"parent": dict(os.environ, GYMFLOCK_LIB=os.path.abspath(parent_lib)), "new": dict(os.environ)}
    envs["new"].pop("GYMFLOCK_LIB", None)
    runs = {k: {"bench_robot_steps_per_s": [], "cov_reset_seeded_512_ms": []} for k in envs}
    for _ in range(rounds):
        for k in ("parent", "new"):
            runs[k]["bench_robot_steps_per_s"].append(bench(envs[k]))
            runs[k]["cov_reset_seeded_512_ms"].append(child("s", repeats, envs[k])["ms"])
    out = {"rounds": rounds, "runs": runs}
    for key in ("bench_robot_steps_per_s", "cov_reset_seeded_512_ms"):
        p, n = runs["parent"][key], runs["new"][key]
        mp, mn = statistics.median(p), statistics.median(n)
        out[key] = {"parent_median": mp, "new_median": mn, "gap_rel": (mn - mp) / mp,
                    "parent_spread_rel": (max(p) - min(p)) / mp, "new_spread_rel": (max(n) - min(n)) / mn}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cov_reset", "cov_reset_timing.json"))
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--part", choices=["m", "d", "s"])
    ap.add_argument("--parent-lib")
    ap.add_argument("--rounds", type=int, default=3)
    args = ap.parse_args()
    if args.part:
        print(json.dumps({"m": part_m, "d": part_d, "s": part_s}[args.part](args.repeats)), flush=True)
        return
    res = {"batched": child("m", args.repeats), "dropin_arl_reset": child("d", args.repeats)}
    if args.parent_lib:
        res["parent_vs_new"] = part_ab(args.parent_lib, args.rounds, args.repeats)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res, indent=1))


if __name__ == "__main__":
    main()
