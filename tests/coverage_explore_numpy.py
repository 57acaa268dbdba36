"""NumPy restatement of the reference's hidden-node observation (hide_nodes=True,
gym_flock/envs/spatial/coverage.py:334-346 with utils.py:27-39) and of the masked greedy
choice (:817-821), for the ExploreEnv tests. TEST INFRASTRUCTURE ONLY.

Indexing is the reference's: agents 0..R-1 are robots, R..R+T-1 targets, and an index of
-1 (the unused edge slots) wraps to node max_nodes - 1 as NumPy's indexing does.
"""
import numpy as np

from oracle import coverage as oc

HIDDEN_RADIUS = 4.0 * 5.5  # 4.0 * DELTA, the module constant, whatever the env's res


def seen_nodes(xr, x, rad=HIDDEN_RADIUS):
    """_nodes_within_radius(rad, xr, x): node j is seen when the sum over the robots of its
    distances r (those above rad zeroed) is positive, i.e. some robot has 0 < r <= rad."""
    r = np.linalg.norm(np.asarray(xr, np.float64)[:, None, :] - np.asarray(x, np.float64)[None, :, :], axis=2)
    r[r > rad] = 0
    return np.sum(r, axis=0) > 0


def initial_discovered(max_nodes, n_robots):
    d = np.zeros(max_nodes, np.uint8)
    d[:n_robots] = 1
    return d


def hidden_obs(discovered, nodes3, senders, receivers, xr, targets):
    """One observation's hidden part from the unhidden one. discovered (max_nodes) is the
    set before this observation; nodes3 (max_nodes, 3), senders / receivers (4 max_nodes)
    are the ordinary observation's, xr (R, 2) the robots and targets (T, 2) the map.
    Returns (discovered after, nodes (max_nodes, 4) float64, out_senders int32)."""
    xr, targets = np.asarray(xr, np.float64), np.asarray(targets, np.float64)
    R, n_agents = len(xr), len(xr) + len(targets)
    senders, receivers = np.asarray(senders).astype(np.int64).ravel(), np.asarray(receivers).astype(np.int64).ravel()
    disc = np.asarray(discovered).astype(np.float64).ravel().copy()
    seen = seen_nodes(xr, np.vstack([xr, targets]))
    disc[:n_agents] = (disc[:n_agents] + seen) > 0
    nodes = np.zeros((len(disc), 4))
    nodes[:, :3] = np.asarray(nodes3, np.float64).reshape(len(disc), 3)
    nodes = nodes * disc[:, None]
    frontier = receivers[(1.0 - disc[senders]) * disc[receivers] > 0.0]
    nodes[frontier, 3] = 1.0
    seen_edges = disc[senders] * disc[receivers]
    seen_edges[-8 * R:] = 1.0
    out = np.where(seen_edges > 0, senders, -1)
    return disc.astype(np.uint8), nodes, out.astype(np.int32)


def masked_greedy_actions(cost, prev, cur, visited_targets, discovered_targets, recv, n_robots):
    """controller(greedy=True) with hide_nodes (:808-872) without its random fallback: the
    visited targets, then the undiscovered ones are masked, each through np.where on a
    (T, 1) column, which also masks column 0 whenever that mask is not empty. Returns
    (actions, needs_random) as oracle.coverage.greedy_actions does."""
    R = n_robots
    c = np.asarray(cur) - R
    r = np.asarray(cost, np.float64)[c, :].copy()
    for rows in (np.nonzero(np.asarray(visited_targets) == 1)[0], np.nonzero(np.asarray(discovered_targets) == 0)[0]):
        if len(rows):
            r[:, rows] = oc.MAX_COST
            r[:, 0] = oc.MAX_COST
    goal = np.argmin(r, axis=1)
    acts = np.zeros(R, np.int32)
    rand = np.zeros(R, bool)
    for i in range(R):
        if r[i, goal[i]] == oc.MAX_COST or prev[goal[i], c[i]] == -1:
            rand[i] = True
            continue
        acts[i] = int(np.nonzero(np.asarray(recv[i]) == prev[goal[i], c[i]] + R)[0][0])
    return acts, rand
