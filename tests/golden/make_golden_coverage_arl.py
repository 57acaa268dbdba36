"""CoverageARL-v0 / CoverageFull-v0 golden vectors from the reference (run where the
reference is installed; make_golden._install_shims() provides the gym stand-in).

Writes tests/golden/coverage_arl.npz:
  * the target pool of grid_slice10 (from_occupancy make_map.py:234-271, load_graph
    coverage_arl.py:46-62): the 1714 raw targets, the 1266 all_targets, min_xy, max_xy,
    subgraph_size;
  * for seeds 0-39, np.random.seed(s); env._generate_targets() (coverage_arl.py:64-83):
    the number of tries (np.random.uniform calls), the accepted map as int16 indices
    into the pool, and one np.random.uniform() drawn afterwards (the stream position);
    for seeds 0-9 the second map of the same stream;
  * two episodes of CoverageARLEnv() at its default arguments, one greedy (g_*) and one
    random (r_*), recorded like coverage_r6_*;
  * one update_state call (us_*);
  * one CoverageFullEnv run: reset, 12 random steps, 8 greedy steps (full_*).

Usage:  python tests/golden/make_golden_coverage_arl.py
"""
import importlib
import os
import sys

import numpy as np

OUT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, OUT)
from make_golden import _install_shims  # noqa: E402


class _CountUniform:
    """Counts np.random.uniform calls (one per try of _generate_targets)."""

    def __enter__(self):
        self.n = 0
        self.orig = np.random.uniform

        def counted(*a, **k):
            self.n += 1
            return self.orig(*a, **k)

        np.random.uniform = counted
        return self

    def __exit__(self, *exc):
        np.random.uniform = self.orig


def _obs_rec(o):
    return (o["nodes"].copy(), o["edges"].copy(), np.array(o["senders"]).copy(), np.array(o["receivers"]).copy(),
            np.array(o["step"]).copy())


def _run(env, obs, policies, env_seed, pre):
    """The reset observation and one record per step of `policies` ("random" steps draw
    from RandomState(env_seed + 77), "greedy" ones call controller(greedy=True))."""
    R = env.n_robots
    rec = {"n_robots": R, "n_targets": env.n_targets, "max_nodes": env.max_nodes,
           "targets": env.x[R:, :2].copy(), "motion_senders": np.array(env.motion_edges[0]),
           "motion_receivers": np.array(env.motion_edges[1]), "x0": env.x.copy(),
           "visited0": env.visited[:, 0].copy(), "start_region": np.array(env.start_region, bool)}
    for k, v in zip(("nodes0", "edges0", "senders0", "receivers0", "step0"), _obs_rec(obs)):
        rec[k] = v
    rs = np.random.RandomState(env_seed + 77)
    acts, xs, rews, dones, nodes, edges, snd, rcv, stp, vis, cls = ([] for _ in range(11))
    for policy in policies:
        if policy == "random":
            a = rs.randint(0, 4, size=(R,))
        else:
            a = env.controller(random=False, greedy=True).flatten()
        acts.append(np.array(a).astype(np.int32))
        o, r, d, _ = env.step(np.array(a).reshape(-1, 1))
        xs.append(env.x[:R].copy())
        rews.append(r)
        dones.append(d)
        n, e, s, q, st = _obs_rec(o)
        nodes.append(n), edges.append(e), snd.append(s), rcv.append(q), stp.append(st)
        vis.append(env.visited[:, 0].copy())
        cls.append(np.array(env.closest_targets).astype(np.int32))
    rec.update(actions=np.array(acts), xr=np.array(xs), reward=np.array(rews), done=np.array(dones),
               nodes=np.array(nodes, dtype=np.float32), edges=np.array(edges, dtype=np.float32),
               senders=np.array(snd, dtype=np.int32), receivers=np.array(rcv, dtype=np.int32),
               step=np.array(stp), visited=np.array(vis, dtype=np.int8), closest=np.array(cls))
    return {pre + k: v for k, v in rec.items()}


def gen_coverage_arl():
    arl = importlib.import_module("gym_flock.envs.spatial.coverage_arl")
    full = importlib.import_module("gym_flock.envs.spatial.coverage_full")
    mm = importlib.import_module("gym_flock.envs.spatial.make_map")
    out = {}
    np.random.seed(0)
    env = arl.CoverageARLEnv()
    pool = env.all_targets
    out.update(pool_raw=mm.from_occupancy(10, 2.0), all_targets=pool.copy(), min_xy=env.min_xy.copy(),
               max_xy=env.max_xy.copy(), subgraph_size=env.subgraph_size.copy())
    where = {tuple(p): k for k, p in enumerate(pool.tolist())}
    tries, maps, probe, tries2, maps2 = [], [], [], [], []
    for s in range(40):
        np.random.seed(s)
        with _CountUniform() as c:
            t, _ = env._generate_targets()
        tries.append(c.n)
        maps.append(np.array([where[tuple(p)] for p in t.tolist()], np.int16))
        if s < 10:
            with _CountUniform() as c:
                t2, _ = env._generate_targets()
            tries2.append(c.n)
            maps2.append(np.array([where[tuple(p)] for p in t2.tolist()], np.int16))
            np.random.seed(s)
            env._generate_targets()
        probe.append(np.random.uniform())
    out.update(tries=np.array(tries, np.int32), map_len=np.array([len(m) for m in maps], np.int32),
               map_idx=np.concatenate(maps), probe=np.array(probe),
               next_tries=np.array(tries2, np.int32), next_len=np.array([len(m) for m in maps2], np.int32),
               next_idx=np.concatenate(maps2))
    print("sampler: tries", tries, "sizes", [len(m) for m in maps])

    for pre, policy, map_seed, env_seed in (("g_", "greedy", 5, 6), ("r_", "random", 3, 4)):
        np.random.seed(map_seed)
        env = arl.CoverageARLEnv()
        env.seed(env_seed)
        np.random.seed(map_seed)
        obs = env.reset()
        rec = _run(env, obs, [policy] * 50, env_seed, pre)
        rec[pre + "map_seed"], rec[pre + "env_seed"] = map_seed, env_seed
        out.update(rec)
        print("episode %s: T=%d motion edges %d reward %d" % (policy, env.n_targets, env.n_motion_edges,
                                                              int(np.sum(rec[pre + "reward"]))))

    # update_state (coverage_arl.py:42-44) on the random episode's final env
    state = env.x[env.n_robots:][[7, 3, 100, 42]] + np.array([[0.3, -0.2], [1.9, 0.4], [-2.1, 2.2], [0.0, 0.0]])
    env.update_state(state)
    out.update(us_state=state, us_x=env.x[:env.n_robots].copy())

    np.random.seed(11)
    env = full.CoverageFullEnv()
    env.seed(12)
    obs = env.reset()
    rec = _run(env, obs, ["random"] * 12 + ["greedy"] * 8, 12, "full_")
    out.update(rec)
    print("full: T=%d motion edges %d nodes %s edges %s reward %d" % (
        env.n_targets, env.n_motion_edges, obs["nodes"].shape, obs["edges"].shape, int(np.sum(rec["full_reward"]))))
    np.savez_compressed(os.path.join(OUT, "coverage_arl.npz"), **out)


if __name__ == "__main__":
    _install_shims()
    gen_coverage_arl()
