"""Plain-NumPy restatement of the CoverageARL-v0 target pool and subgraph sampler (test
infrastructure: tests/test_coverage_arl_cpu.py pins it against tests/golden/coverage_arl.npz,
scripts/arl_reset_probe.py times it as the host yardstick).

Reference: make_map.from_occupancy (make_map.py:234-271), CoverageARLEnv.load_graph
(coverage_arl.py:46-62) and CoverageARLEnv._generate_targets (coverage_arl.py:64-83).
"""
import numpy as np

XYZ_MIN = (-321.0539855957031, -276.5395050048828)  # make_map.py:264
MIN_GRAPH_SIZE = 200


def largest_component(points, radius):
    """Mask of the largest connected component of the radius graph 0 < |p - q| <= radius.
    Components are numbered in order of their lowest node (as scipy's connected_components
    does), so argmax(bincount(labels)) takes the largest count with the lowest root."""
    n = len(points)
    d = points[:, None, :] - points[None, :, :]
    r = np.sqrt(d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1])
    adj = (r > 0) & (r <= radius)
    labels = -np.ones(n, np.int64)
    n_comp = 0
    for s in range(n):
        if labels[s] >= 0:
            continue
        labels[s] = n_comp
        frontier = np.array([s])
        while len(frontier):
            nxt = np.nonzero(adj[frontier].any(axis=0) & (labels < 0))[0]
            labels[nxt] = n_comp
            frontier = nxt
        n_comp += 1
    return labels == np.argmax(np.bincount(labels))


def occupancy_targets(arr, downsample_rate=10, perimeter_delta=2.0, xyz_min=XYZ_MIN):
    """from_occupancy: cells in meshgrid(xs, ys).flatten() order (second index outer, first
    inner), free cells whose nearest occupied cell is within perimeter_delta, as points
    ((cell * res) + xyz_min) + res / 2, rotated (x, y) = (t_y, -t_x)."""
    occ = np.asarray(arr) != 0
    n0, n1 = occ.shape
    k = int(np.floor(perimeter_delta))
    pad = np.zeros((n0 + 2 * k, n1 + 2 * k), bool)
    pad[k:k + n0, k:k + n1] = occ
    near = np.zeros((n0, n1), bool)
    for di in range(-k, k + 1):
        for dj in range(-k, k + 1):
            if np.sqrt(float(di * di + dj * dj)) <= perimeter_delta:
                near |= pad[k + di:k + di + n0, k + dj:k + dj + n1]
    keep = near & ~occ
    jj, ii = np.nonzero(keep.T)  # j outer, i inner
    res = 0.5 * downsample_rate
    tx = (ii * res + xyz_min[0]) + res / 2
    ty = (jj * res + xyz_min[1]) + res / 2
    return np.stack([ty, -1.0 * tx], axis=1)


def load_graph(arr, motion_radius, downsample_rate=10, perimeter_delta=2.0, check_connected=True,
               num_subgraphs=3.0, xyz_min=XYZ_MIN):
    """load_graph: (raw targets, all_targets, min_xy, max_xy, subgraph_size), the last three
    (1, 2) arrays."""
    raw = occupancy_targets(arr, downsample_rate, perimeter_delta, xyz_min)
    pool = raw[largest_component(raw, motion_radius)] if check_connected else raw
    min_xy = np.min(pool, axis=0).reshape((1, 2))
    max_xy = np.max(pool, axis=0).reshape((1, 2))
    return raw, pool, min_xy, max_xy, (max_xy - min_xy) / num_subgraphs


def sample_submap(pool, min_xy, max_xy, subgraph_size, motion_radius, rng=np.random, min_targets=MIN_GRAPH_SIZE,
                  max_tries=None):
    """_generate_targets: (indices into the pool of the accepted map, tries). rng is
    np.random (the reference's global stream) or a RandomState. Returns (None, tries)
    after max_tries tries without a window."""
    tries = 0
    while max_tries is None or tries < max_tries:
        graph_start = rng.uniform(low=min_xy, high=max_xy - subgraph_size)
        tries += 1
        graph_end = graph_start + subgraph_size
        idx = np.nonzero(np.all(np.logical_and(graph_start <= pool, pool < graph_end), axis=1))[0]
        if len(idx) < min_targets:
            continue
        idx = idx[largest_component(pool[idx], motion_radius)]
        if len(idx) >= min_targets:
            return idx, tries
    return None, tries
