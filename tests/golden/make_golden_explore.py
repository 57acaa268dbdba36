"""ExploreEnv-v0 golden vectors from the reference (run where the reference is installed;
make_golden._install_shims() provides the gym stand-in).

Writes tests/golden/coverage_explore.npz: two episodes of ExploreEnv() on grid_slice10, one
greedy (g_*: map seed 5, env seed 6) and one random (r_*: map seed 3, env seed 4, actions
from RandomState(env_seed + 77)), each run until done. Per episode the map, the reset
state and observation, and per step the hidden observation (nodes as uint8: every value is
0 or 1; the senders with unseen edges hidden), receivers, edges, step, reward, done,
discovered_nodes, the visited flags, the actions and the robots' nodes; after the greedy
episode one np_random draw (the stream position after the expert's fallback draws).

Usage:  python tests/golden/make_golden_explore.py
"""
import importlib
import os
import sys

import numpy as np

OUT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, OUT)
from make_golden import _install_shims  # noqa: E402


def _episode(ex, pre, policy, map_seed, env_seed):
    np.random.seed(map_seed)
    env = ex.ExploreEnv()
    env.seed(env_seed)
    np.random.seed(map_seed)
    obs = env.reset()
    R = env.n_robots
    assert obs["nodes"].dtype == np.float64 and set(np.unique(obs["nodes"])) <= {0.0, 1.0}
    rec = {"map_seed": map_seed, "env_seed": env_seed, "n_robots": R, "n_targets": env.n_targets,
           "max_nodes": env.max_nodes, "targets": env.x[R:, :2].copy(), "x0": env.x.copy(),
           "visited0": env.visited[:, 0].astype(np.uint8), "start_region": np.array(env.start_region, bool),
           "nodes0": obs["nodes"].astype(np.uint8), "edges0": obs["edges"].astype(np.float32),
           "senders0": np.array(obs["senders"], np.int32), "receivers0": np.array(obs["receivers"], np.int32),
           "step0": np.array(obs["step"]), "discovered0": env.discovered_nodes[:, 0].astype(np.uint8),
           "stored_senders0": np.array(env.senders, np.int32)}
    rs = np.random.RandomState(env_seed + 77)
    keys = ("actions", "reward", "done", "nodes", "edges", "senders", "receivers", "step", "discovered", "visited",
            "closest", "xr")
    seq = {k: [] for k in keys}
    done, fallback = False, 0
    while not done:
        if policy == "random":
            a = rs.randint(0, 4, size=(R,))
        else:
            pos = env.np_random.get_state()[2]
            a = env.controller(random=False, greedy=True).flatten()
            fallback += (env.np_random.get_state()[2] - pos) % 624
        o, r, done, _ = env.step(np.array(a).reshape(-1, 1))
        assert o["nodes"].dtype == np.float64 and set(np.unique(o["nodes"])) <= {0.0, 1.0}
        seq["actions"].append(np.array(a, np.int32))
        seq["reward"].append(r)
        seq["done"].append(done)
        seq["nodes"].append(o["nodes"].astype(np.uint8))
        seq["edges"].append(o["edges"].astype(np.float32))
        seq["senders"].append(np.array(o["senders"], np.int32))
        seq["receivers"].append(np.array(o["receivers"], np.int32))
        seq["step"].append(np.array(o["step"]))
        seq["discovered"].append(env.discovered_nodes[:, 0].astype(np.uint8))
        seq["visited"].append(env.visited[:, 0].astype(np.uint8))
        seq["closest"].append(np.array(env.closest_targets, np.int32))
        seq["xr"].append(env.x[:R].copy())
    rec.update({k: np.array(v) for k, v in seq.items()})
    if policy == "greedy":
        rec["probe"] = env.np_random.uniform()
    print("episode %s: T=%d steps %d reward %d fallback draws %d" % (policy, env.n_targets, len(seq["reward"]),
                                                                     int(np.sum(seq["reward"])), fallback))
    return {pre + k: v for k, v in rec.items()}


def gen_explore():
    ex = importlib.import_module("gym_flock.envs.spatial.coverage_explore")
    out = {}
    out.update(_episode(ex, "g_", "greedy", 5, 6))
    out.update(_episode(ex, "r_", "random", 3, 4))
    np.savez_compressed(os.path.join(OUT, "coverage_explore.npz"), **out)


if __name__ == "__main__":
    _install_shims()
    gen_explore()
