"""Time per step of the hidden-node expert (ExploreEnv's demonstrations) on a batch: the
host-paced route against the fused call (cov_explore_expert).

Batch (scripts/explore_timing.py's): 512 envs x 4 robots x max_nodes = 1000, CoverageARL maps
from grid_slice10 (res 5.0), horizon 19, reset(seed=0, new_maps=True, map_seed=100); the
episode never ends, so late steps are fallback draws, as in the reference's loop.

Each mode runs in a child process of its own (one library per process), the modes interleaved,
REPEATS times; every mode starts from the same reset and times STEPS expert steps after
WARM warm-up steps, wall clock from the first call until the device is done:
  a  step(greedy=True) through the host-paced route: cov_controller_greedy with the fetch of
     needs_random, the fallback draws on the host, cov_set_actions, the resident step and the
     hidden pass. With --parent-lib it runs on that library (the commit before the fused
     call), else on this one with the fused route switched off;
  b  step(greedy=True) on this library: the fused call with n_steps = 1;
  c  explore_expert_steps(50), fetching rewards and done;
  d  the same, also recording actions and the flat row of every step into device tensors;
  e  as d with every=10;
  A, C  modes a and c on the FIRST 50 steps after a reset (ExploreEnv's episode length), where
     most robots still have a discovered target to head for: the mean over 5 episodes, each
     after reset(seed=0) on the same maps (their time matrices stay valid).
Also recorded from mode c's records: the fallback share (draws per robot-step) and, from the
getters between chunks, the mean number of targets the expert may still head for (T minus
the masked ones).

  python scripts/explore_expert_timing.py [--parent-lib PATH] [--repeats 3] [--out PATH]
Writes profiles/explore_expert/explore_expert_timing.json (or --out).
"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B, R, M, CHUNK = 512, 4, 1000, 50


def child(mode, steps, warm):
    import numpy as np
    torch = None
    if mode in ("d", "e"):
        import torch  # before gym_flock
        assert torch.cuda.is_available()
    sys.path[:0] = [ROOT, os.path.join(ROOT, "gym-flock_amd")]
    from gym_flock.vec import VecCoverage
    grid = np.load(os.path.join(ROOT, "tests", "golden", "grid_slice10.npy"))
    v = VecCoverage(B, R, max_nodes=M, episode_length=10 ** 9, res=5.0, hide_nodes=True, horizon=19)
    v.load_occupancy(grid)
    v.reset(seed=0, new_maps=True, map_seed=100)
    res = {"mode": mode, "lib": os.environ.get("GYMFLOCK_LIB", "in-tree"), "steps": steps, "warm": warm}
    if mode in ("a", "A"):
        v._explore_fused = lambda: False
    if mode in ("A", "C"):
        def episode():
            if mode == "A":
                for _ in range(CHUNK):
                    v.step(greedy=True)
                return 0
            return int(v.explore_expert_steps(CHUNK, record=("rewards", "done", "needs_random"))["needs_random"].sum())

        episode()  # builds the time matrices
        spent, draws, n_ep = 0.0, 0, 5
        for _ in range(n_ep):
            v.reset(seed=0)
            v.sync()
            t0 = time.perf_counter()
            draws += episode()
            v.sync()
            spent += time.perf_counter() - t0
        res["us_per_step"] = 1e6 * spent / (n_ep * CHUNK)
        if mode == "C":
            res["draws_per_robot_step"] = draws / float(n_ep * CHUNK * B * R)
        v.close()
        print("RESULT " + json.dumps(res))
        return
    if mode in ("a", "b"):
        for _ in range(warm):
            v.step(greedy=True)
        v.sync()
        t0 = time.perf_counter()
        for _ in range(steps):
            v.step(greedy=True)
        v.sync()
        res["us_per_step"] = 1e6 * (time.perf_counter() - t0) / steps
    else:
        every = 10 if mode == "e" else 1
        dev = None
        if torch is not None:
            tdt = {np.float64: torch.float64, np.uint8: torch.uint8, np.int32: torch.int32, np.float32: torch.float32}
            sh = v.h.rollout_shapes(CHUNK, every)
            dev = {k: torch.zeros(sh[k][0], dtype=tdt[sh[k][1]], device="cuda") for k in ("rewards", "done", "actions", "flat_obs")}
            torch.cuda.synchronize()
            ptrs = {k: t.data_ptr() for k, t in dev.items()}
            res["record_bytes_per_step"] = sum(t.numel() * t.element_size() for t in dev.values()) / CHUNK

        def run():
            if dev is None:
                return v.explore_expert_steps(CHUNK, record=("rewards", "done"))
            v.explore_expert_steps(CHUNK, every=every, device_ptrs=ptrs)

        for _ in range(max(warm // CHUNK, 1)):
            run()
        v.sync()
        n = max(steps // CHUNK, 1)
        t0 = time.perf_counter()
        for _ in range(n):
            run()
        v.sync()
        res["us_per_step"] = 1e6 * (time.perf_counter() - t0) / (n * CHUNK)
        if mode == "c":  # what the expert faced, from a fresh episode of the same length
            v.reset(seed=0, new_maps=True, map_seed=100)
            T = v.n_targets.astype(np.int64)
            draws, left = 0, []
            for _ in range((warm + steps) // CHUNK):
                masked = np.array([np.count_nonzero((v.h.visited(b)[:T[b]] == 1) | (v.h.discovered(b)[R:R + T[b]] == 0))
                                   for b in range(0, B, 16)])
                left.append(float(np.mean(T[::16] - masked)))
                draws += int(v.explore_expert_steps(CHUNK, record=("needs_random",))["needs_random"].sum())
            res["draws_per_robot_step"] = draws / float((warm + steps) // CHUNK * CHUNK * B * R)
            res["mean_targets_left_at_chunk_starts"] = left
            res["targets_mean"] = float(T.mean())
    v.close()
    print("RESULT " + json.dumps(res))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "explore_expert", "explore_expert_timing.json"))
    ap.add_argument("--parent-lib", default=None, help="libgymflock.so of the commit before cov_explore_expert, for mode a")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--steps", type=int, default=500)
    ap.add_argument("--warm", type=int, default=100)
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        child(a.child, a.steps, a.warm)
        return
    runs = {m: [] for m in "abcdeAC"}
    extra = {}
    for _ in range(a.repeats):
        for m in "abcdeAC":
            env = dict(os.environ)
            if m in ("a", "A") and a.parent_lib:
                env["GYMFLOCK_LIB"] = os.path.abspath(a.parent_lib)
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", m, "--steps", str(a.steps),
                                "--warm", str(a.warm)], env=env, capture_output=True, timeout=600)
            if p.returncode != 0:
                sys.stderr.write(p.stderr.decode()[-3000:])
                raise SystemExit("mode %s failed (exit %d)" % (m, p.returncode))
            r = json.loads([ln for ln in p.stdout.decode().splitlines() if ln.startswith("RESULT ")][-1][7:])
            runs[m].append(r["us_per_step"])
            for k in ("draws_per_robot_step", "mean_targets_left_at_chunk_starts", "targets_mean", "record_bytes_per_step"):
                if k in r:
                    extra["%s_%s" % (m, k)] = r[k]
    out = {"batch": {"envs": B, "robots": R, "max_nodes": M, "chunk": CHUNK, "steps": a.steps, "warm": a.warm},
           "mode_a_library": "parent" if a.parent_lib else "this library, fused route off",
           "us_per_step": runs,
           "median_us_per_step": {m: sorted(v)[len(v) // 2] for m, v in runs.items()},
           "spread_us_per_step": {m: max(v) - min(v) for m, v in runs.items()}}
    out.update(extra)
    med = out["median_us_per_step"]
    out["a_over_b"], out["a_over_c"] = med["a"] / med["b"], med["a"] / med["c"]
    out["first_episode_A_over_C"] = med["A"] / med["C"]
    out["full_pass_and_rows_us_per_step_d_minus_c"] = med["d"] - med["c"]
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
