"""What does the hidden-node pass (cov_set_hidden, ExploreEnv) cost per step?

Batch: 512 envs x 4 robots x max_nodes = 1000 on CoverageARL maps (grid_slice10), resident
random actions, one launch per step (cov_set_streams(1)), the same handle with hiding off
and on, alternating. Per mode the device time per step from HIP events around every step
(cov_kernel_timing: the step kernel, plus the hidden pass when on) and the wall time of
K enqueued steps until the device is done (the method of scripts/cov_launch_probe.py).
Drop-in: wall time of CoverageARLEnv.step and ExploreEnv.step with random actions.

  python scripts/explore_timing.py            (JSON on stdout)
"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "gym-flock_amd")]
import gym_flock  # noqa: E402
from gym_flock.vec import VecCoverage  # noqa: E402


def batch(grid, reps):
    B, R, M = 512, 4, 1000
    v = VecCoverage(B, R, max_nodes=M, episode_length=10 ** 9, res=5.0, hide_nodes=True, horizon=19)
    v.load_occupancy(grid)
    v.reset(seed=0, new_maps=True, map_seed=100)
    v.set_actions(np.random.RandomState(7).randint(0, 4, size=(B, R)))
    v.h.set_streams(1)
    step = v.h._step_resident
    out = {"envs": B, "robots": R, "max_nodes": M, "targets_mean": float(v.n_targets.mean()),
           "n_motion_mean": float(v.h.n_motion().mean()), "off": [], "on": []}
    for _ in range(reps):
        for mode in ("off", "on"):
            v.h.set_hidden(mode == "on")
            for _ in range(2000):  # clocks up
                step()
            v.sync()
            v.h.timing_start(1)
            for _ in range(500):
                step()
            ms, n = v.h.timing_stop()
            res = {"device_us_per_step": 1e3 * ms, "timed_steps": int(n)}
            for K in (100, 300):
                v.sync()
                t0 = time.perf_counter()
                for _ in range(K):
                    step()
                t1 = time.perf_counter()
                v.sync()
                t2 = time.perf_counter()
                res["enqueue_us_per_step_%d" % K] = 1e6 * (t1 - t0) / K
                res["wall_us_per_step_%d" % K] = 1e6 * (t2 - t0) / K
            out[mode].append(res)
    v.close()
    return out


def dropin(grid, env_id, steps=2000):
    np.random.seed(3)
    env = gym_flock.make(env_id, occupancy=grid)
    env.seed(4)
    env.reset()
    rs = np.random.RandomState(1)
    acts = rs.randint(0, 4, size=(steps, env.n_robots, 1))
    for t in range(200):  # warm
        if env.step(acts[t])[2]:
            env.reset()
    spent, n = 0.0, 0
    for t in range(steps):
        t0 = time.perf_counter()
        done = env.step(acts[t])[2]
        spent += time.perf_counter() - t0
        n += 1
        if done:
            env.reset()
    env.close()
    return {"env": env_id, "steps": n, "step_us": 1e6 * spent / n}


def main():
    grid = np.load(os.path.join(ROOT, "tests", "golden", "grid_slice10.npy"))
    out = {"batch": batch(grid, int(os.environ.get("REPS", "3"))),
           "dropin": [dropin(grid, i) for i in ("CoverageARL-v0", "ExploreEnv-v0", "CoverageARL-v0", "ExploreEnv-v0")]}
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
