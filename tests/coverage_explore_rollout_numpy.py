"""NumPy restatement of the hidden-node expert rollout (cov_explore_expert /
VecCoverage.explore_expert_steps). TEST INFRASTRUCTURE ONLY.

One env's closed loop, built from pieces that are pinned elsewhere and nothing new:
  - the masked greedy choice and the hidden observation (tests/coverage_explore_numpy.py),
  - the step, the motion graph tables and the time matrix (oracle/coverage.py),
  - a numpy RandomState per env for the fallback robots' np_random.choice(4), drawn for the
    robots that need one, in robot order, in one call (coverage.py:861-864).
Per step: controller(greedy=True) with hide_nodes on the state as it stands, the draws, step(),
then the discovery and the hidden observation from the robots' new positions.

The oracle's action-edge features divide by its module constant RES = 5.5, so the flat rows
are the engine's only for handles with res 5.5; everything else holds for any res.
"""
import numpy as np

import coverage_explore_numpy as en
from oracle import coverage as oc


class ExploreRollout:
    """One env with hidden nodes, stepped by its own expert."""

    def __init__(self, targets, n_robots, max_nodes, motion_radius=oc.RES * 1.2, horizon=oc.HORIZON,
                 episode_length=oc.EPISODE_LENGTH):
        self.targets = np.asarray(targets, np.float64)
        self.R, self.T, self.M = int(n_robots), len(self.targets), int(max_nodes)
        self.episode_length = int(episode_length)
        self.o = oc.CoverageOracle(self.targets, self.R, self.M, motion_radius=motion_radius)
        s, q = self.o.motion[0] - self.R, self.o.motion[1] - self.R
        self.cost, self.prev = oc.time_matrix(self.T, s, q, horizon=horizon)

    def reset(self, start, visited_targets, rng):
        """start (R) target-local; visited_targets (>= T) 0 / 1 before the robots' own visits
        (cov_reset's argument); rng: the env's RandomState where the reset left it."""
        self.rng = rng
        unvisited = np.nonzero(np.asarray(visited_targets)[:self.T] == 0)[0] + self.R
        obs = self.o.reset(np.asarray(start, np.int64), unvisited)
        self.disc = en.initial_discovered(self.M, self.R)
        return self._hide(obs)

    def _hide(self, obs):
        self.disc, nodes4, hsnd = en.hidden_obs(self.disc, obs["nodes"], obs["senders"], obs["receivers"], self.o.xr,
                                                self.targets)
        self.obs = {"nodes": nodes4, "edges": obs["edges"], "senders": hsnd, "receivers": obs["receivers"],
                    "step": obs["step"]}
        return self.obs

    def flat_row(self):
        """The hidden FlattenDictWrapper row of the last observation, float32."""
        return oc.flatten_obs(self.obs).astype(np.float32)

    def visited(self):
        return self.o.visited[self.R:].astype(np.uint8)

    def step(self):
        """One expert step. Returns a dict: actions (R), needs_random (R) bool, reward, done,
        left (T minus the masked targets: what the expert may still head for), plain (the
        unmasked greedy choice (actions, needs_random) of the same state)."""
        R, T = self.R, self.T
        cur = self.o.closest()
        recv = oc.action_receivers(cur, self.o.nbr, self.o.cnt, R)
        vis, disc = self.o.visited[R:], self.disc[R:R + T]
        a, rnd = en.masked_greedy_actions(self.cost, self.prev, cur, vis, disc, recv, R)
        plain = oc.greedy_actions(self.cost, self.prev, cur, vis, recv, R)
        left = T - int(np.count_nonzero((vis == 1) | (disc == 0)))
        if rnd.any():
            k = np.nonzero(rnd)[0]
            a[k] = self.rng.choice(4, size=len(k))
        obs, reward, _ = self.o.step(a)
        done = self.o.step_counter == self.episode_length or np.sum(self.o.visited[R:]) == T
        self._hide(obs)
        return {"actions": a.astype(np.int32), "needs_random": rnd, "reward": float(reward), "done": bool(done),
                "left": left, "plain": plain, "closest": self.o.closest()}


def rollout(envs, n_steps, every=1):
    """n_steps of every env (a list of ExploreRollout after reset). Returns the records in
    cov_rollout's shapes (done and needs_random as bool), `left` (n_steps, B) and `differs`
    (n_steps, B): whether the masked choice differs from the unmasked one."""
    B, R = len(envs), envs[0].R
    out = {"rewards": np.zeros((n_steps, B)), "done": np.zeros((n_steps, B), bool),
           "actions": np.zeros((n_steps, B, R), np.int32), "needs_random": np.zeros((n_steps, B, R), bool),
           "flat_obs": np.zeros((n_steps // every, B, 16 * envs[0].M + 1), np.float32),
           "left": np.zeros((n_steps, B), np.int64), "differs": np.zeros((n_steps, B), bool),
           "closest": np.zeros((n_steps, B, R), np.int64)}
    for t in range(n_steps):
        for b, e in enumerate(envs):
            s = e.step()
            out["rewards"][t, b], out["done"][t, b] = s["reward"], s["done"]
            out["actions"][t, b], out["needs_random"][t, b] = s["actions"], s["needs_random"]
            out["left"][t, b], out["closest"][t, b] = s["left"], s["closest"]
            out["differs"][t, b] = bool(np.any(s["plain"][1] != s["needs_random"]) or
                                        np.any((s["plain"][0] != s["actions"]) & ~s["needs_random"]))
            if (t + 1) % every == 0:
                out["flat_obs"][(t + 1) // every - 1, b] = e.flat_row()
    return out
