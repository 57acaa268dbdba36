"""Inputs shared by tests/test_coverage_large_cpu.py and tests/test_coverage_large_gpu.py
(test infrastructure): occupancy grids whose pools sit at the edges of the pool's capacity,
and the 300-target path whose hop counts pass the one-byte entries."""
import functools

import numpy as np

import coverage_arl_numpy as an

# inner block of free cells -> pool size: one past the former cap of 4096, the cap, one past it
WALLED = {(17, 241): 4097, (64, 128): 8192, (3, 2731): 8193}


def walled_grid(a, b):
    """All ones with an a x b block of zeros inside: with perimeter_delta = max(a, b) + 2
    every free cell is within reach of a wall, so the pool is the whole block."""
    g = np.ones((a + 2, b + 2), np.uint8)
    g[1:-1, 1:-1] = 0
    return g


def walled_pool(a, b):
    """The pool of walled_grid(a, b) as from_occupancy orders and places it: the second
    index outer, the first inner, ((cell * 5.0) + xyz_min) + 2.5, rotated (x, y) = (t_y, -t_x)."""
    jj, ii = np.meshgrid(np.arange(1, b + 1), np.arange(1, a + 1), indexing="ij")
    tx = (ii.ravel() * 5.0 + an.XYZ_MIN[0]) + 2.5
    ty = (jj.ravel() * 5.0 + an.XYZ_MIN[1]) + 2.5
    return np.stack([ty, -1.0 * tx], axis=1)


@functools.lru_cache(maxsize=None)
def walled_reference(a, b, num_subgraphs=3.0):
    """coverage_arl_numpy.load_graph of walled_grid(a, b) at motion radius 6.0 (res 5.0),
    computed once per process (seconds and ~2 GB at 8,192 points): (raw, pool, min_xy,
    max_xy, subgraph_size). Treat the arrays as read-only."""
    return an.load_graph(walled_grid(a, b), 6.0, perimeter_delta=max(a, b) + 2, num_subgraphs=num_subgraphs)


def line(n=300, spacing=5.5):
    """n targets on a line: hop counts up to n - 1."""
    return np.stack([np.arange(n) * spacing, np.zeros(n)], axis=1)
