"""Inputs for the Coverage map tests at the edges of cov_generate_maps (shared by
tests/test_oracle_coverage_maps.py, which proves on the CPU that each input does what it is
meant to, and tests/test_coverage_maps_edges_gpu.py, which runs them on the device): exactly
cocircular and collinear city sets, the non-default arenas, and cities placed so that one
lattice point's squared distance to its nearest waypoint lies inside the rounding window of
the near-road test.

Not a test module: it only builds inputs and restates nothing of the algorithm (that is
oracle/coverage_maps.py)."""
import numpy as np

from oracle import coverage_maps as cmo


def circle_points(r2, scale=1.0):
    """The integer points of x^2 + y^2 = r2 in (x, y) order, times scale: exactly cocircular
    in floating point when the scaled coordinates are exact. (The order matters to the map:
    a road's waypoints start at its lower-numbered city.)"""
    r = int(np.floor(np.sqrt(r2)))
    pts = [(x, y) for x in range(-r, r + 1) for y in range(-r, r + 1) if x * x + y * y == r2]
    return np.array(pts, float) * scale


def cocircular12():
    """x^2 + y^2 = 25 times 10: 12 cities, every triple's circumcircle is empty."""
    return circle_points(25, 10.0)


def cocircular20():
    """x^2 + y^2 = 625 times 2: 20 cities, all 190 pairs are roads."""
    return circle_points(625, 2.0)


def collinear12():
    x = np.linspace(-100.0, 100.0, 12)
    return np.stack([x, x / 2], axis=1)


def square_plus_line():
    """A square (cocircular) plus 8 collinear cities below it."""
    sq = [[-60, -60], [60, -60], [60, 60], [-60, 60]]
    return np.array(sq + [[-110 + 20 * i, -110] for i in range(8)], float)


# (xmax, ymax, spacing, motion_radius): non-square arenas (NJ comes from arange(-ny, nx)),
# another spacing, link radius equal to, twice and below the spacing (K = 2, 3, 1)
ARENAS = [
    (57.3, 33, 5.5, 6.6),
    (100, 80, 4.0, 4.8),
    (120.5, 7.25, 5.5, 6.6),
    (60, 90, 5.5, 5.5),
    (60, 90, 5.5, 11.0),
    (60, 40, 5.5, 7.0),
    (60, 90, 5.5, 5.4),
]


def arena_cities(xmax, ymax, n=12, seed=9):
    rs = np.random.RandomState(seed)
    return np.stack([rs.uniform(-xmax, xmax, n), rs.uniform(-ymax, ymax, n)], axis=1)


def targets_from_first_edges(c, n_edges, motion_radius=5.5 * 1.2):
    """The map built from only the first n_edges Delaunay edges in (i, j) order (what an
    edge list of that capacity would keep), default arena."""
    c = np.asarray(c, float)
    lat, _, _ = cmo.lattice(-120, 120, -120, 120)
    edges, _ = cmo.delaunay_edges(c)
    roads = cmo.waypoints(c, edges[:n_edges], motion_radius)
    dx = lat[:, None, 0] - roads[None, :, 0]
    dy = lat[:, None, 1] - roads[None, :, 1]
    t = lat[np.sqrt(np.min(dx * dx + dy * dy, axis=1)) <= motion_radius / 1.4]
    return t[cmo._components_largest(t, motion_radius)]


# The rounding window of the near-road test. motion_radius 7.0 makes near_radius exactly 5.0;
# the lattice point P = (0, 0) (default arena: coordinates are exact multiples of 5.5) and a
# city at P + (3, 4) + a few ulps.
BOUNDARY_MOTION_RADIUS = 7.0
BOUNDARY_POINT = np.array([0.0, 0.0])


def _sq(city):
    dx, dy = BOUNDARY_POINT[0] - city[0], BOUNDARY_POINT[1] - city[1]
    return dx * dx + dy * dy


def boundary_offsets(steps=6):
    """City positions near (3, 4), found by stepping each coordinate up to `steps` doubles:
    'exact' (squared distance to P exactly 25), 'above_near' (squared distance above 25
    whose square root still rounds to 5.0: near) and 'above_far' (the root is the next
    double above 5.0: not near). All three squared distances lie within 2^-50 of 25."""
    up5 = np.nextafter(5.0, np.inf)
    out = {"exact": np.array([3.0, 4.0])}
    xs, ys = [3.0], [4.0]
    for _ in range(steps):
        xs.append(np.nextafter(xs[-1], np.inf))
        ys.append(np.nextafter(ys[-1], np.inf))
    for x in xs:
        for y in ys:
            s = _sq((x, y))
            if s > 25.0 and np.sqrt(s) == 5.0:
                out.setdefault("above_near", np.array([x, y]))
            elif np.sqrt(s) == up5:
                out.setdefault("above_far", np.array([x, y]))
    return out


def boundary_cities(first):
    """12 cities: `first` (near (3, 4)) and 11 in the square [25, 110]^2 beyond it, so it is
    a hull vertex, every road leaves it away from P (its other waypoints are farther from P
    than the city) and P's lattice neighbours (5.5, 0), (0, 5.5) are near it either way."""
    rs = np.random.RandomState(21)
    return np.concatenate([np.asarray(first, float)[None], rs.uniform(25, 110, size=(11, 2))])


def has_point(targets, p):
    return bool(np.any(np.all(targets == np.asarray(p, float)[None], axis=1)))
