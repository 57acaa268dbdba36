"""NumPy restatement of the recorded expert rollout across episode ends (cov_expert_rollout /
VecCoverage.expert_rollout). TEST INFRASTRUCTURE ONLY.

One env's loop `reset(); while not done: a = controller(greedy=True); step(a)`, built from
pieces that are pinned elsewhere and nothing new:
  - the step, the motion graph tables, the time matrix, the greedy choice and the flat row
    (oracle/coverage.py),
  - a numpy RandomState per env for the fallback robots' np_random.choice(4), drawn for the
    robots that need one, in robot order, in one call (coverage.py:861-864),
  - the reset draws on an unchanged map from the same stream (tests/coverage_reset_numpy.py:
    reset_draws / grow_region; coverage.py:398-424 with graph_changed == False).

The oracle's action-edge features divide by its module constant RES = 5.5 and its done flag
uses its EPISODE_LENGTH; for another res the 8R tail features are recomputed here from the
same distances, and the done flag is taken from the env's own episode length.
"""
import numpy as np

import coverage_reset_numpy as rn
from oracle import coverage as oc


class CoverageRollout:
    """One env that hides nothing, stepped by its own expert and reset by its own stream."""

    def __init__(self, targets, n_robots, max_nodes, res=oc.RES, horizon=oc.HORIZON,
                 episode_length=oc.EPISODE_LENGTH, frac_active=0.5, nearby=0):
        self.targets = np.asarray(targets, np.float64)
        self.R, self.T, self.M = int(n_robots), len(self.targets), int(max_nodes)
        self.res, self.episode_length = float(res), int(episode_length)
        self.frac_active, self.nearby = float(frac_active), int(nearby)
        self.o = oc.CoverageOracle(self.targets, self.R, self.M, motion_radius=self.res * 1.2)
        self.s, self.q = self.o.motion[0] - self.R, self.o.motion[1] - self.R  # target-local motion edges
        self.cost, self.prev = oc.time_matrix(self.T, self.s, self.q, horizon=horizon)
        self.n_resets, self.status, self.resets = 0, 0, []

    def _keep(self, obs):
        if self.res != oc.RES:  # the 8R action-edge features with this env's res (:292)
            R = self.R
            recv = oc.action_receivers(self.o.closest(), self.o.nbr, self.o.cnt, R).reshape(-1)
            d = self.o.xr[np.repeat(np.arange(R), oc.N_ACTIONS)] - self.targets[recv - R]
            dist = np.sqrt(d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1])
            obs["edges"][-8 * R:, 0] = np.concatenate([dist, dist]) / self.res
        self.obs = obs
        return obs

    def reset(self, start, visited_targets, rng):
        """start (R) target-local; visited_targets (>= T) 0 / 1 before the robots' own visits
        (cov_reset's argument); rng: the env's RandomState where the reset left it."""
        self.rng = rng
        unvisited = np.nonzero(np.asarray(visited_targets)[:self.T] == 0)[0] + self.R
        return self._keep(self.o.reset(np.asarray(start, np.int64), unvisited))

    def reset_drawn(self):
        """reset() on the unchanged map from the env's own stream (cov_reset_device's draws).
        Returns the draws; a region with fewer nodes than robots leaves the env as it is (its
        stream advanced by the scalar draw)."""
        before = self.rng.get_state()
        d = rn.reset_draws(self.rng, self.T, self.R, self.frac_active, self.nearby, self.s, self.q)
        after = self.rng.get_state()
        # the stream around the draws; regenerated: the key was regenerated inside them
        d["rng_before"], d["rng_after"] = before, after
        d["regenerated"] = not np.array_equal(before[1], after[1])
        self.status |= d["status"]
        if d["start"] is not None:
            self.n_resets += 1
            unvisited = np.nonzero(d["visited"] == 0)[0] + self.R
            self._keep(self.o.reset(d["start"].astype(np.int64), unvisited))
            d["visited_after"] = self.visited()
        self.resets.append(d)
        return d

    def flat_row(self):
        """The FlattenDictWrapper row of the last observation, float32."""
        return oc.flatten_obs(self.obs).astype(np.float32)

    def visited(self):
        return self.o.visited[self.R:].astype(np.uint8)

    def step(self):
        """One expert step. Returns a dict: actions (R), needs_random (R) bool, reward, done,
        end ("" / "limit" / "all": why the episode ended; both hold: "all")."""
        R, T = self.R, self.T
        cur = self.o.closest()
        recv = oc.action_receivers(cur, self.o.nbr, self.o.cnt, R)
        a, rnd = oc.greedy_actions(self.cost, self.prev, cur, self.o.visited[R:], recv, R)
        if rnd.any():
            k = np.nonzero(rnd)[0]
            a[k] = self.rng.choice(4, size=len(k))
        obs, reward, _ = self.o.step(a)
        self._keep(obs)
        all_seen = np.sum(self.o.visited[R:]) == T
        limit = self.o.step_counter == self.episode_length
        return {"actions": a.astype(np.int32), "needs_random": rnd, "reward": float(reward),
                "done": bool(all_seen or limit), "end": "all" if all_seen else "limit" if limit else ""}


def rollout(envs, n_steps, every=1, auto_reset=False):
    """n_steps of every env (a list of CoverageRollout after reset). Returns the records in
    cov_rollout's shapes (done and needs_random as bool), `end` (n_steps, B) of "" / "limit" /
    "all", and with auto_reset n_resets (B), reset_status (B) and `resets`: per env the list of
    its in-run draws (reset_drawn)."""
    B, R = len(envs), envs[0].R
    out = {"rewards": np.zeros((n_steps, B)), "done": np.zeros((n_steps, B), bool),
           "actions": np.zeros((n_steps, B, R), np.int32), "needs_random": np.zeros((n_steps, B, R), bool),
           "flat_obs": np.zeros((n_steps // every, B, 15 * envs[0].M + 1), np.float32),
           "end": np.zeros((n_steps, B), "U5")}
    for e in envs:
        e.n_resets, e.status, e.resets = 0, 0, []
    for t in range(n_steps):
        for b, e in enumerate(envs):
            s = e.step()
            out["rewards"][t, b], out["done"][t, b], out["end"][t, b] = s["reward"], s["done"], s["end"]
            out["actions"][t, b], out["needs_random"][t, b] = s["actions"], s["needs_random"]
            if auto_reset and s["done"]:
                e.reset_drawn()
            if (t + 1) % every == 0:
                out["flat_obs"][(t + 1) // every - 1, b] = e.flat_row()
    if auto_reset:
        out["n_resets"] = np.array([e.n_resets for e in envs], np.int32)
        out["reset_status"] = np.array([e.status for e in envs], np.int32)
        out["resets"] = [e.resets for e in envs]
    return out
