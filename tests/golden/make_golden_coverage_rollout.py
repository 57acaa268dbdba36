"""Golden vectors for cov_expert_rollout from the reference (run where the reference is
installed; make_golden._install_shims() provides the gym stand-in).

The reference driver's loop `reset(); while not done: a = controller(greedy=True); step(a)` over
several episodes on ONE map: CoverageARLEnv with _generate_targets returning its first sampled
map with graph_changed=True once and the same map with False from then on, so every later
reset() takes coverage.py:398-424's branch for an unchanged map (the nearby-starts region, the
start draw and the unvisited draw from np_random where it stands).

Writes tests/golden/coverage_expert_rollout.npz (not coverage_rollout.npz: the single-episode
tests take every coverage_r*.npz for one of make_golden_coverage.py's episodes). Run "a": np.random.seed(5), episode_length=12,
env.seed(6), reset() and four greedy episodes with reset() between them (T = 215, 4 robots,
max_nodes 1000; 11 steps per episode, since reset()'s own _get_obs_reward counts one; the
stream position wraps past 624 inside the run). Run "b": np.random.seed(3), episode_length=7,
env.seed(4) (T = 255), without the rows, which keeps the file small. Per run, prefix a_ / b_:
  targets, motion_senders, motion_receivers (global indices), n_robots, max_nodes, res,
  frac_active, nearby, episode_length, map_seed, env_seed;
  per reset k (5 of them: the first, the three between the episodes and one after the last
  episode, which is what a rollout with in-launch resets does after its last done step): region (T) bool, start (R) target-local, visited (T) int8 as
  reset() leaves it (the robots' own nodes included), rng_key / rng_pos after the reset;
  row0: the first reset's flat row;
  per step t: actions (R), reward, done, row (15 * max_nodes + 1) float32: the flat row the
  expert sees for step t + 1 (after a done step: the next reset's row);
  rng_key_end / rng_pos_end: np_random after the last step, before the trailing reset.

Usage:  python tests/golden/make_golden_coverage_rollout.py
"""
import importlib
import os
import sys

import numpy as np

OUT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, OUT)
from make_golden import _install_shims  # noqa: E402

KEYS = ["nodes", "edges", "senders", "receivers", "step"]  # coverage.py:90


def _row(obs):
    return np.concatenate([np.asarray(obs[k]).ravel() for k in KEYS]).astype(np.float32)


def _run(arl, map_seed, env_seed, episode_length, episodes, pre, with_rows=True):
    class OneMap(arl.CoverageARLEnv):
        _kept = None

        def _generate_targets(self):
            if self._kept is None:
                self._kept = super()._generate_targets()[0]
                return self._kept, True
            return self._kept, False

    np.random.seed(map_seed)
    env = OneMap(episode_length=episode_length)
    env.seed(env_seed)
    R = env.n_robots
    rec = {}
    regions, starts, visiteds, keys, poss = [], [], [], [], []
    acts, rews, dones, rows = [], [], [], []

    def reset():
        obs = env.reset()
        regions.append(np.array(env.start_region, bool))
        starts.append(np.array(env.closest_targets).astype(np.int32) - R)
        visiteds.append(env.visited[R:R + env.n_targets, 0].astype(np.int8))
        st = env.np_random.get_state()
        keys.append(np.array(st[1], np.uint32)), poss.append(int(st[2]))
        return obs

    obs = reset()
    rec["row0"] = _row(obs)
    for ep in range(episodes):
        done = False
        while not done:
            a = np.array(env.controller(random=False, greedy=True)).flatten().astype(np.int32)
            obs, r, done, _ = env.step(a.reshape(-1, 1))
            acts.append(a), rews.append(float(r)), dones.append(bool(done))
            if done and ep + 1 == episodes:
                st = env.np_random.get_state()  # after the last step, before the trailing reset
            if done:
                obs = reset()
            rows.append(_row(obs))
    rec.update(targets=env.x[R:R + env.n_targets, :2].copy(), motion_senders=np.array(env.motion_edges[0], np.int32),
               motion_receivers=np.array(env.motion_edges[1], np.int32), n_robots=R, max_nodes=env.max_nodes,
               res=float(env.res), frac_active=float(env.frac_active_targets), nearby=R * 5,
               episode_length=episode_length, map_seed=map_seed, env_seed=env_seed,
               region=np.array(regions), start=np.array(starts), visited=np.array(visiteds),
               rng_key=np.array(keys), rng_pos=np.array(poss, np.int32),
               actions=np.array(acts), reward=np.array(rews), done=np.array(dones), row=np.array(rows),
               rng_key_end=np.array(st[1], np.uint32), rng_pos_end=int(st[2]))
    if not with_rows:
        del rec["row0"], rec["row"]
    print("run %s: T=%d steps=%d episode ends at %s regions %s stream positions %s -> %d" % (
        pre, env.n_targets, len(acts), np.nonzero(dones)[0].tolist(), [int(r.sum()) for r in regions], poss, st[2]))
    return {pre + k: v for k, v in rec.items()}


def gen_coverage_rollout():
    arl = importlib.import_module("gym_flock.envs.spatial.coverage_arl")
    out = {}
    out.update(_run(arl, 5, 6, 12, 4, "a_"))
    out.update(_run(arl, 3, 4, 7, 4, "b_", with_rows=False))
    path = os.path.join(OUT, "coverage_expert_rollout.npz")
    np.savez_compressed(path, **out)
    print("wrote %s (%d bytes)" % (path, os.path.getsize(path)))


if __name__ == "__main__":
    _install_shims()
    gen_coverage_rollout()
