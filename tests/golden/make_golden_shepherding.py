"""Shepherding-v0 golden vectors from the reference (run where the reference is installed;
make_golden._install_shims() provides the gym stand-in, and a namespace package stands in
for gym_flock.envs.shepherding).

Writes tests/golden/shepherding_ep0.npz (driven by the reference's controller()) and
shepherding_ep1.npz (driven by RandomState(seed + 77).uniform(-2, 2) float32 actions):
60 steps each from seed(s); reset(). Per file: every state x (61,N,3), every action
(60,n_shepherds,2), the controller() output of every state (61,n_shepherds,2), every
reward (60), the reward of the reset state, the adjacency of every tenth state (7,N,N),
the seed used and free_run_sensitivity.

A seed is used only if over its whole episode
  - no state has a pair with |r2 - 4| or |r2 - 2| below 1e-9,
  - no state has a sheep within 1e-9 of the goal radius,
  - no controller call has a line-of-sight angle within 1e-9 rad of its 2 or 5 degree
    threshold (every pair the device tests, not only those the reference reaches);
otherwise the next seed is tried. With these guards a one-ulp difference in cos / sin /
atan2 cannot flip a comparison, and the tests compare everything.

free_run_sensitivity: the largest absolute state deviation over the episode between the
reference and the restatement (tests/shepherding_numpy.py) re-run from the same start with
the same actions and every cos and sin result moved one ulp by np.nextafter, the larger of
the two directions.

Usage:  python tests/golden/make_golden_shepherding.py
"""
import importlib
import os
import sys
import types

import numpy as np

OUT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, OUT)
sys.path.insert(0, os.path.dirname(OUT))
from make_golden import REF, _install_shims  # noqa: E402
import shepherding_numpy as sn  # noqa: E402

STEPS = 60
GAP = 1e-9


class GuardError(Exception):
    pass


def _guard(env):
    ns = env.n_shepherds
    if sn.pair_gap(env.x) < GAP:
        raise GuardError("a pair within %g of a radius threshold" % GAP)
    if sn.goal_gap(env.x, ns, env.goal_region_radius) < GAP:
        raise GuardError("a sheep within %g of the goal radius" % GAP)
    if sn.controller(env.x, ns)[2] < GAP:
        raise GuardError("a line-of-sight angle within %g of its threshold" % GAP)


def _nudged(fn, direction):
    return lambda a: np.nextafter(fn(a), direction)


def _episode(sh, seed, policy):
    env = sh.ShepherdingEnv()
    env.seed(seed)
    env.reset()
    ns = env.n_shepherds
    rs = np.random.RandomState(seed + 77)
    xs, us, cs, rews, adjs = [env.x.copy()], [], [], [], [env._compute_adj_mat()]
    reward0 = env._instant_cost()
    _guard(env)
    for t in range(STEPS):
        c = env.controller()
        cs.append(c)
        u = c if policy == "controller" else rs.uniform(-2, 2, size=(ns, 2)).astype(np.float32)
        (obs, adj), r, done, _ = env.step(u)
        assert not done and obs.shape == (env.n_agents, 4)
        _guard(env)
        xs.append(env.x.copy())
        us.append(u)
        rews.append(r)
        if (t + 1) % 10 == 0:
            adjs.append(adj)
    cs.append(env.controller())
    xs = np.array(xs)
    sens = 0.0
    for direction in (np.inf, -np.inf):
        x = xs[0]
        for t in range(STEPS):
            x = sn.step(x, us[t], ns, env.dt, env.action_scalar, _nudged(np.cos, direction),
                        _nudged(np.sin, direction))[0]
            sens = max(sens, np.abs(x - xs[t + 1]).max())
    return dict(seed=seed, policy=policy, n_shepherds=ns, n_sheep=env.n_sheep, dt=env.dt,
                comm_radius=env.comm_radius, action_scalar=env.action_scalar,
                goal_region_radius=env.goal_region_radius, x=xs, u=np.array(us), controller=np.array(cs),
                reward=np.array(rews), reward0=reward0, adj=np.array(adjs), adj_steps=np.arange(0, STEPS + 1, 10),
                free_run_sensitivity=sens)


def gen_shepherding():
    sh = importlib.import_module("gym_flock.envs.shepherding.shepherding")
    seed = 0
    for k, policy in enumerate(("controller", "random")):
        while True:
            try:
                rec = _episode(sh, seed, policy)
                break
            except GuardError as e:
                print("seed %d: %s, trying the next" % (seed, e))
                seed += 1
        path = os.path.join(OUT, "shepherding_ep%d.npz" % k)
        np.savez_compressed(path, **rec)
        print("episode %d (%s): seed %d, mean reward %.3f, free_run_sensitivity %.3g, %d bytes"
              % (k, policy, seed, rec["reward"].mean(), rec["free_run_sensitivity"], os.path.getsize(path)))
        assert os.path.getsize(path) < 256 << 10
        seed += 1


if __name__ == "__main__":
    _install_shims()
    m = types.ModuleType("gym_flock.envs.shepherding")
    m.__path__ = [os.path.join(REF, "gym_flock", "envs", "shepherding")]
    sys.modules["gym_flock.envs.shepherding"] = m
    gen_shepherding()
