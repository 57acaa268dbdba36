"""Shepherding-v0 across episode ends, from the reference (run where the reference is
installed, as make_golden_shepherding.py): the driver's loop on one np_random stream,

    seed(s); reset(); 20 x (u = controller(); step(u)); reset(); 20 x ...; reset(); 20 x ...; reset()

four resets and three episodes of 20 steps. Writes tests/golden/shepherding_episodes.npz:
the four reset states x0 (4,N,3), the state after every step x (60,N,3) (x[19], x[39], x[59]
are terminal: the next reset keeps their headings), every action u (60,n_shepherds,2) and
reward (60), the reward of every reset state reward0 (4), the stream position after each
reset pos (4), the stream after the last one (final_key (624), final_pos), the seed and
free_run_sensitivity.

A seed is used only if every state, the reset states included, passes
make_golden_shepherding.py's guards (GAP = 1e-9 on the pair, goal and line-of-sight
thresholds); otherwise the next seed is tried. With them a one-ulp difference in cos / sin
/ atan2 cannot flip a comparison, so rewards are compared exactly.

free_run_sensitivity: as in make_golden_shepherding.py but over the whole run: the largest
absolute state deviation between the reference and the restatement (tests/
shepherding_numpy.py) re-run from RandomState(s) with the recorded actions and every cos and
sin result, those of the resets included, moved one ulp by np.nextafter, the larger of the
two directions.

Usage:  python tests/golden/make_golden_shepherding_episodes.py
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
from make_golden_shepherding import GuardError, _guard, _nudged  # noqa: E402
import shepherding_numpy as sn  # noqa: E402

EPISODES, LENGTH = 3, 20


def _record(sh, seed):
    env = sh.ShepherdingEnv()
    env.seed(seed)
    x0, xs, us, rews, rew0, pos = [], [], [], [], [], []

    def reset():
        env.reset()
        _guard(env)
        x0.append(env.x.copy())
        rew0.append(env._instant_cost())
        pos.append(env.np_random.get_state()[2])

    reset()
    for _ in range(EPISODES):
        for _ in range(LENGTH):
            u = env.controller()
            (obs, adj), r, done, _ = env.step(u)
            assert not done
            _guard(env)
            xs.append(env.x.copy())
            us.append(u)
            rews.append(r)
        reset()
    st = env.np_random.get_state()
    x0, xs = np.array(x0), np.array(xs)
    ns, n = env.n_shepherds, env.n_agents
    sens = 0.0
    for direction in (np.inf, -np.inf):
        cos, sin = _nudged(np.cos, direction), _nudged(np.sin, direction)
        rs = np.random.RandomState(seed)
        x = np.zeros((n, 3))

        def restated_reset(k):
            length = np.sqrt(rs.uniform(0, env.r_max, size=(n,)))
            angle = np.pi * rs.uniform(0, 2, size=(n,))
            x[:, 0] = length * cos(angle) + env.goal_offset[0]
            x[:, 1] = length * sin(angle) + env.goal_offset[1]
            return max(sens, np.abs(x - x0[k]).max())

        sens = restated_reset(0)
        for e in range(EPISODES):
            for t in range(LENGTH):
                k = e * LENGTH + t
                x = sn.step(x, us[k], ns, env.dt, env.action_scalar, cos, sin)[0]
                sens = max(sens, np.abs(x - xs[k]).max())
            sens = restated_reset(e + 1)
        assert rs.get_state()[2] == st[2] and np.array_equal(rs.get_state()[1], st[1])
    return dict(seed=seed, n_shepherds=ns, n_sheep=env.n_sheep, episode_length=LENGTH, r_max=env.r_max,
                goal_offset=np.asarray(env.goal_offset, np.float64), goal_region_radius=env.goal_region_radius,
                x0=x0, x=xs, u=np.array(us), reward=np.array(rews), reward0=np.array(rew0),
                pos=np.array(pos, np.int32), final_key=np.asarray(st[1], np.uint32), final_pos=np.int32(st[2]),
                free_run_sensitivity=sens)


def gen():
    sh = importlib.import_module("gym_flock.envs.shepherding.shepherding")
    seed = 0
    while True:
        try:
            rec = _record(sh, seed)
            break
        except GuardError as e:
            print("seed %d: %s, trying the next" % (seed, e))
            seed += 1
    path = os.path.join(OUT, "shepherding_episodes.npz")
    np.savez_compressed(path, **rec)
    print("seed %d, mean reward %.3f, positions %s, free_run_sensitivity %.3g, %d bytes"
          % (seed, rec["reward"].mean(), rec["pos"].tolist(), rec["free_run_sensitivity"], os.path.getsize(path)))
    assert os.path.getsize(path) < 256 << 10


if __name__ == "__main__":
    _install_shims()
    m = types.ModuleType("gym_flock.envs.shepherding")
    m.__path__ = [os.path.join(REF, "gym_flock", "envs", "shepherding")]
    sys.modules["gym_flock.envs.shepherding"] = m
    gen()
