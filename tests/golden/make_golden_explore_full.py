"""ExploreFullEnv golden vectors from the reference (run where the reference is installed;
make_golden._install_shims() provides the gym stand-in).

Writes tests/golden/coverage_explore_full.npz: ExploreFullEnv() on grid_slice10 (the whole
5,659-target pool as one map, 100 robots, horizon 19) under np.random.seed(5) / env.seed(6):
the map, the reset state, the static observation once (edges, receivers, stored senders),
then N_STEPS greedy steps. Per step: actions, reward, done, the hidden node rows bit-packed
(every value is 0 or 1), the kept-slot mask of the hidden senders (sender != -1) bit-packed,
discovered_nodes and the visited flags bit-packed, closest_targets and the robots'
positions; one np_random draw afterwards. The time matrix is 32 M entries, so it is stored
as a digest: per source the count of entries below MAX_COST and their sum, and the full
cost and predecessor rows of 8 sources (first, last, 6 evenly spaced between).

The first controller call builds the reference's time matrix: about 150 s and 1 GB.

Usage:  python tests/golden/make_golden_explore_full.py
"""
import importlib
import os
import sys
import time

import numpy as np

OUT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, OUT)
from make_golden import _install_shims  # noqa: E402

N_STEPS = 6
MAP_SEED, ENV_SEED = 5, 6


def _bits(a):
    a = np.asarray(a)
    assert set(np.unique(a)) <= {0, 1}
    return np.packbits(a.astype(np.uint8).ravel())


def gen_explore_full():
    ef = importlib.import_module("gym_flock.envs.spatial.coverage_explore_full")
    cov = importlib.import_module("gym_flock.envs.spatial.coverage")
    np.random.seed(MAP_SEED)
    env = ef.ExploreFullEnv()
    env.seed(ENV_SEED)
    np.random.seed(MAP_SEED)
    obs = env.reset()
    R, T, M = env.n_robots, env.n_targets, env.max_nodes
    rec = {"map_seed": MAP_SEED, "env_seed": ENV_SEED, "n_robots": R, "n_targets": T, "max_nodes": M,
           "targets": env.x[R:, :2].copy(), "x0": env.x.copy(),
           "visited0": _bits(env.visited[:, 0]), "start_region": _bits(np.array(env.start_region, bool)),
           "nodes0": _bits(obs["nodes"]), "kept0": _bits(np.array(obs["senders"]) != -1),
           "edges0": obs["edges"].astype(np.float32), "receivers0": np.array(obs["receivers"], np.int32),
           "stored_senders0": np.array(env.senders, np.int32),
           "step0": np.array(obs["step"]), "discovered0": _bits(env.discovered_nodes[:, 0])}
    keys = ("actions", "reward", "done", "nodes", "kept", "step", "discovered", "visited", "closest", "xr")
    seq = {k: [] for k in keys}
    for t in range(N_STEPS):
        t0 = time.time()
        a = env.controller(random=False, greedy=True).flatten()
        if t == 0:
            print("first controller call: %.1f s" % (time.time() - t0))
        o, r, done, _ = env.step(np.array(a).reshape(-1, 1))
        # the static parts never change: stored once above
        assert np.array_equal(o["edges"].astype(np.float32)[:env.n_motion_edges], rec["edges0"][:env.n_motion_edges])
        assert np.array_equal(np.array(env.senders, np.int32)[:env.n_motion_edges],
                              rec["stored_senders0"][:env.n_motion_edges])
        seq["actions"].append(np.array(a, np.int32))
        seq["reward"].append(r)
        seq["done"].append(done)
        seq["nodes"].append(_bits(o["nodes"]))
        seq["kept"].append(_bits(np.array(o["senders"]) != -1))
        seq["step"].append(np.array(o["step"]))
        seq["discovered"].append(_bits(env.discovered_nodes[:, 0]))
        seq["visited"].append(_bits(env.visited[:, 0]))
        seq["closest"].append(np.array(env.closest_targets, np.int32))
        seq["xr"].append(env.x[:R, :2].copy())
    rec.update({k: np.array(v) for k, v in seq.items()})
    rec["probe"] = env.np_random.uniform()
    cost, prev = np.asarray(env.graph_cost), np.asarray(env.graph_previous)
    assert cost.shape == (T, T) and prev.shape == (T, T)
    fin = cost < cov.MAX_COST
    rec["tm_count"] = fin.sum(axis=1).astype(np.int32)
    rec["tm_sum"] = np.where(fin, cost, 0).sum(axis=1).astype(np.int64)
    rows = np.unique(np.round(np.linspace(0, T - 1, 8)).astype(np.int64))
    assert len(rows) == 8
    rec["tm_rows"] = rows.astype(np.int32)
    rec["tm_cost_rows"] = cost[rows].astype(np.int16)  # graph_cost[source, :]
    rec["tm_prev_rows"] = prev[rows].astype(np.int16)  # graph_previous[source, :]
    assert np.array_equal(rec["tm_cost_rows"], cost[rows]) and np.array_equal(rec["tm_prev_rows"], prev[rows])
    rec["tm_max_finite"] = int(cost[fin].max())
    path = os.path.join(OUT, "coverage_explore_full.npz")
    np.savez_compressed(path, **rec)
    print("T=%d M=%d motion edges %d reward %s largest finite hop count %d inf share %.3f file %d bytes" % (
        T, M, env.n_motion_edges, seq["reward"], rec["tm_max_finite"], 1.0 - fin.mean(), os.path.getsize(path)))


if __name__ == "__main__":
    _install_shims()
    gen_explore_full()
