"""What does the reference's ExploreFullEnv configuration cost on the device?

CoverageARLEnv with ExploreFullEnv's arguments on grid_slice10 (perimeter_delta 12: one map
of 5,659 targets and 20,910 motion edges, 100 robots, hidden nodes, horizon 19), seeds
np.random.seed(5) / env.seed(6) as tests/golden/coverage_explore_full.npz. Wall times, each
ending in a device synchronise (the calls fetch their results):
  - the constructor (pool, motion graph) and reset();
  - the first controller(greedy=True): buffers, edge schedule, time matrix, greedy actions;
  - the time matrix rebuilt alone (cov_set_tm_plan marks it stale), REPS times;
  - later steps: controller(greedy=True), then step(), each timed, STEPS times.
With --oracle also the same map's time matrix by oracle/coverage.py's NumPy restatement of
construct_time_matrix on one core (minutes), and whether the device's matrix equals it.

  python scripts/explore_full_timing.py [--oracle]            (JSON on stdout)
"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "gym-flock_amd")]
from gym_flock.envs.spatial import CoverageARLEnv  # noqa: E402
from oracle import coverage as oc  # noqa: E402

REPS, STEPS = 5, 10
KW = dict(hide_nodes=True, n_node_feat=4, n_robots=100, episode_length=50, pad_nodes=False, max_nodes=1500,
          nearby_starts=True, num_subgraphs=1, check_connected=True, downsample_rate=10, perimeter_delta=12.0,
          horizon=19)


def main():
    grid = np.load(os.path.join(ROOT, "tests", "golden", "grid_slice10.npy"))
    out = {"config": {k: v for k, v in KW.items()}}
    np.random.seed(5)
    t0 = time.perf_counter()
    env = CoverageARLEnv(occupancy=grid, **KW)
    out["init_s"] = time.perf_counter() - t0
    env.seed(6)
    np.random.seed(5)
    t0 = time.perf_counter()
    env.reset()
    out["reset_s"] = time.perf_counter() - t0
    h = env._h
    R, T = env.n_robots, env.n_targets
    out.update(n_targets=int(T), max_nodes=int(env.max_nodes), n_motion=int(h.n_motion()[0]))
    t0 = time.perf_counter()
    a = env.controller(random=False, greedy=True)
    out["first_greedy_call_s"] = time.perf_counter() - t0
    rebuild = []
    for _ in range(REPS):
        h.set_tm_plan(0)  # marks the matrix stale
        h.sync()
        t0 = time.perf_counter()
        h.controller_greedy()
        rebuild.append(time.perf_counter() - t0)
    out["time_matrix_rebuild_s"] = rebuild
    ctrl, step = [], []
    for _ in range(STEPS):
        t0 = time.perf_counter()
        a = env.controller(random=False, greedy=True)
        t1 = time.perf_counter()
        env.step(a)
        t2 = time.perf_counter()
        ctrl.append(t1 - t0)
        step.append(t2 - t1)
    out["later_controller_s"] = ctrl
    out["later_step_s"] = step
    out["later_step_with_controller_s_median"] = float(np.median(np.array(ctrl) + np.array(step)))
    if "--oracle" in sys.argv:
        snd, rcv = h.motion_edges(0)
        t0 = time.perf_counter()
        ec, ep = oc.time_matrix(T, snd - R, rcv - R, horizon=KW["horizon"])
        out["numpy_time_matrix_one_core_s"] = time.perf_counter() - t0
        cost, prev = h.time_matrix(0, T)
        out["device_matrix_equals_numpy"] = bool(np.array_equal(cost, ec) and np.array_equal(prev, ep))
        out["time_matrix_speedup"] = out["numpy_time_matrix_one_core_s"] / float(np.median(rebuild))
    env.close()
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
