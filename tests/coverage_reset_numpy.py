"""NumPy restatement of cov_reset_device's draws for one env (TEST INFRASTRUCTURE ONLY).

The reference's reset() (gym_flock/envs/spatial/coverage.py:398-414, :596-599) with
nearby_starts: one scalar np_random.choice(n_targets), the start region grown through the
motion graph (get_n_nearest :655-673), then choice(region members, n_robots, replace=False)
and choice(all targets, int(T * frac), replace=False), all from the env's np_random where it
stands. Written against numpy's own RandomState, so it is the reference's arithmetic; the
loop form of the scalar draw on oracle/mt19937.py is what the device kernel does.
"""
import numpy as np

REGION_SHORT, REGION_SMALL = 1, 2


def grow_region(i, nearby, n_targets, senders, receivers):
    """get_n_nearest(i, nearby) on target-local motion edges: region = {i}; while it holds
    fewer than `nearby` nodes, add every out-neighbour of the set as it stood. Returns
    (bool mask (T), rounds, short): short when a round adds nothing (the reference would
    loop forever)."""
    s, q = np.asarray(senders, np.int64), np.asarray(receivers, np.int64)
    region = np.zeros(n_targets, bool)
    region[i] = True
    rounds, short = 0, False
    while region.sum() < nearby:
        nxt = region.copy()
        nxt[q[region[s]]] = True
        rounds += 1
        if nxt.sum() == region.sum():
            short = True
            break
        region = nxt
    return region, rounds, short


def reset_draws(rs, n_targets, n_robots, frac_active, nearby, senders=None, receivers=None):
    """The draws of one reset from the RandomState rs (advanced in place). senders /
    receivers: the motion edges, target-local. Returns a dict: start (R) target-local or None
    when the region has fewer nodes than robots (numpy raises: nothing more is drawn),
    visited (T) uint8 before the robots' own visits, region (T) bool, status, rounds, i."""
    T, R = int(n_targets), int(n_robots)
    status, rounds, i = 0, 0, None
    if nearby > 0:
        i = int(rs.choice(T))
        region, rounds, short = grow_region(i, nearby, T, senders, receivers)
        status |= REGION_SHORT if short else 0
    else:
        region = np.ones(T, bool)
    members = np.nonzero(region)[0]
    if len(members) < R:
        return {"start": None, "visited": None, "region": region, "status": status | REGION_SMALL,
                "rounds": rounds, "i": i}
    start = rs.choice(members, size=(R,), replace=False)
    drop = rs.choice(np.arange(T) + R, size=(int(T * frac_active),), replace=False)
    visited = np.ones(T, np.uint8)
    visited[drop - R] = 0
    return {"start": start.astype(np.int32), "visited": visited, "region": region, "status": status,
            "rounds": rounds, "i": i}


def scalar_choice_loop(state, n):
    """np_random.choice(n) as the device draws it, on oracle/mt19937.py's stream
    state = [key list, pos]: numpy's masked rejection on 32-bit words with the mask of n - 1;
    n == 1 draws nothing."""
    from oracle import mt19937 as mt
    if n <= 1:
        return 0
    top = n - 1
    mask = top
    for sh in (1, 2, 4, 8, 16):
        mask |= mask >> sh
    while True:
        v = mt._next(state) & mask
        if v <= top:
            return v


def radius_edges(targets, radius):
    """The motion graph of a target set as the device builds it (utils.py:8-24): ordered
    pairs with 0 < |p_i - p_j| <= radius in row-major order, target-local."""
    t = np.asarray(targets, np.float64)
    d = np.sqrt(((t[:, None, :] - t[None, :, :]) ** 2).sum(axis=2))
    s, q = np.nonzero((d > 0) & (d <= radius))
    return s, q
