"""CoverageARL-v0 reset cost for a batch of envs (run on the GPU box):

  host      the NumPy restatement of the subgraph sampler (tests/coverage_arl_numpy.py) on
            one core for np.random.seed(s), s = 0..B-1: ms per env, tries per env;
  submaps   VecCoverage(B, 4, max_nodes=1000, episode_length=50, res=5.0) with the occupancy
            pool loaded: generate_submaps(map_seed=0) (every call the same B maps) and
            generate_submaps() (the streams continue: other maps every call), ms per call;
            the first call's sizes and try counts are checked against the host's;
  reset     reset(seed, new_maps=True): the sampled maps, the reset draws and the reset
            observation, ms per call;
  citymaps  Coverage-v0's city-map generator on the same box (VecCoverage(B, 4,
            max_nodes=1000).generate_maps), the yardstick of the README's maps row.

Every library call ends in a device synchronise, so a host clock around CALLS calls is the
device time plus the call's host work. Each figure is the median of WINDOWS windows of
CALLS calls after a warm-up window. Without --mode the script runs every mode as a child
process under its own time limit, stops at the first that fails, and writes the figures to
--out (default profiles/arl/arl_reset_probe.json).

  python scripts/arl_reset_probe.py [--grid tests/golden/grid_slice10.npy] [--envs 512]
"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.abspath(os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
sys.path[:0] = [ROOT, os.path.join(ROOT, "gym-flock_amd"), os.path.join(ROOT, "tests")]

MODES = (("host", 600), ("submaps", 180), ("reset", 180), ("citymaps", 180))


def windows(fn, calls, n_windows):
    """ms per call: the median, minimum and maximum over n_windows windows of `calls`
    calls, after one warm-up window."""
    for _ in range(calls):
        fn()
    ms = []
    for _ in range(n_windows):
        t0 = time.perf_counter()
        for _ in range(calls):
            fn()
        ms.append(1e3 * (time.perf_counter() - t0) / calls)
    return {"median_ms": float(np.median(ms)), "min_ms": float(min(ms)), "max_ms": float(max(ms)),
            "windows": n_windows, "calls_per_window": calls}


def host(args, grid):
    import coverage_arl_numpy as an
    radius = 0.5 * 10 * 1.2
    _, pool, lo, hi, sub = an.load_graph(grid, radius)
    sizes, tries, ms = [], [], []
    for s in range(args.envs):
        rs = np.random.RandomState(s)
        t0 = time.perf_counter()
        idx, k = an.sample_submap(pool, lo, hi, sub, radius, rs)
        ms.append(1e3 * (time.perf_counter() - t0))
        sizes.append(len(idx))
        tries.append(k)
    return {"envs": args.envs, "ms_per_env_mean": float(np.mean(ms)), "ms_per_env_median": float(np.median(ms)),
            "ms_all_envs": float(np.sum(ms)), "tries_mean": float(np.mean(tries)), "tries_max": int(max(tries)),
            "n_targets": sizes, "tries": tries}


def vec_arl(args, grid):
    from gym_flock.vec import VecCoverage
    v = VecCoverage(args.envs, 4, max_nodes=1000, episode_length=50, res=5.0)
    v.load_occupancy(grid)
    return v


def submaps(args, grid):
    v = vec_arl(args, grid)
    n, st, tries = v.generate_submaps(map_seed=0)
    out = {"envs": args.envs, "n_targets": n.tolist(), "tries": tries.tolist(), "tries_mean": float(tries.mean()),
           "tries_max": int(tries.max())}
    if args.check:
        ref = json.load(open(args.check))["host"]
        assert ref["n_targets"] == out["n_targets"] and ref["tries"] == out["tries"], "device maps differ from the host's"
        out["matches_host"] = True
    out["seeded"] = windows(lambda: v.generate_submaps(map_seed=0), args.calls, args.windows)
    out["continued"] = windows(lambda: v.generate_submaps(), args.calls, args.windows)
    v.close()
    return out


def reset(args, grid):
    v = vec_arl(args, grid)
    v.reset(seed=11, new_maps=True, map_seed=0)
    out = {"envs": args.envs,
           "seeded": windows(lambda: v.reset(seed=11, new_maps=True, map_seed=0), args.calls, args.windows),
           "continued": windows(lambda: v.reset(seed=11, new_maps=True), args.calls, args.windows),
           "same_maps": windows(lambda: v.reset(seed=11), args.calls, args.windows)}
    v.close()
    return out


def citymaps(args, grid):
    from gym_flock.vec import VecCoverage
    v = VecCoverage(args.envs, 4, max_nodes=1000)
    v.generate_maps(map_seed=0)
    out = {"envs": args.envs, "seeded": windows(lambda: v.generate_maps(map_seed=0), args.calls, args.windows),
           "continued": windows(lambda: v.generate_maps(), args.calls, args.windows)}
    v.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--grid", default=os.path.join(ROOT, "tests", "golden", "grid_slice10.npy"))
    ap.add_argument("--envs", type=int, default=512)
    ap.add_argument("--calls", type=int, default=300)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "arl", "arl_reset_probe.json"))
    ap.add_argument("--mode", choices=[m for m, _ in MODES])
    ap.add_argument("--check", help="(child) the figures so far: the device maps are checked against its host entry")
    args = ap.parse_args()
    grid = np.load(args.grid)
    if args.mode:
        print(json.dumps({args.mode: globals()[args.mode](args, grid)}))
        return 0
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    figures = {}
    for mode, limit in MODES:
        cmd = [sys.executable, os.path.abspath(__file__), "--mode", mode, "--grid", args.grid, "--envs", str(args.envs),
               "--calls", str(args.calls), "--windows", str(args.windows)]
        if mode == "submaps":
            cmd += ["--check", args.out]
        try:
            p = subprocess.run(cmd, stdout=subprocess.PIPE, timeout=limit)
        except subprocess.TimeoutExpired:
            print("%s: no result within %d s; stopping" % (mode, limit), file=sys.stderr)
            return 124
        if p.returncode != 0:
            print("%s: exit status %d; stopping" % (mode, p.returncode), file=sys.stderr)
            return p.returncode
        figures.update(json.loads(p.stdout.decode().strip().splitlines()[-1]))
        with open(args.out, "w") as f:
            json.dump(figures, f, indent=1)
        brief = {k: v for k, v in figures[mode].items() if k not in ("n_targets", "tries")}
        print(mode, json.dumps(brief), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
