"""The restatement of the device map algorithm (oracle/coverage_maps.py) pinned on the
CPU: against the reference's recorded maps (tests/golden/coverage_maps.npz, made by
tests/golden/make_golden_coverage.py from /root/reference), against scipy's Delaunay
(the reference's make_map.py:213-219) on many city sets, against numpy's own
np.linalg.norm for the road lengths (make_map.py:227), and the library's host lattice
(cov_map_lattice, no device) against generate_lattice's recorded points. And the inputs of
tests/test_coverage_maps_edges_gpu.py (tests/coverage_map_inputs.py): that the restatement
is pinned for their city counts and arenas, and that each input is the edge it claims."""
import os
import sys

import numpy as np
import pytest

from conftest import GOLDEN
from oracle import coverage_maps as cmo

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import coverage_map_inputs as cmi  # noqa: E402


def _fixture_maps():
    f = np.load(os.path.join(GOLDEN, "coverage_maps.npz"))
    lat, out, o = f["lattice"], [], 0
    for n in f["many_len"]:
        out.append(lat[f["many_idx"][o:o + n]])
        o += n
    return f, out


def test_restated_maps_match_reference_maps():
    """The first 30 recorded seeds (the GPU test runs all 100), and the second map of the
    first 4 streams."""
    f, many = _fixture_maps()
    for s in range(30):
        t, amb = cmo.generate_targets(cmo.cities(np.random.RandomState(s)))
        assert not amb
        np.testing.assert_array_equal(t, many[s], err_msg="seed %d" % s)
    lat = f["lattice"]
    o = 0
    for s, n in enumerate(f["next_len"][:4]):
        rs = np.random.RandomState(s)
        cmo.cities(rs)
        t, _ = cmo.generate_targets(cmo.cities(rs))
        np.testing.assert_array_equal(t, lat[f["next_idx"][o:o + n]])
        o += n


def test_cities_are_numpy_uniform():
    for s in (0, 7, 2**31 + 5):
        np.testing.assert_array_equal(cmo.cities(np.random.RandomState(s)),
                                      np.random.RandomState(s).uniform(-120, 120, size=(12, 2)))


def test_bruteforce_delaunay_equals_scipy():
    """The empty-circumcircle triangles' edges equal scipy's vertex_neighbor_vertices
    (Qhull) on 400 random city sets, none of them near-degenerate."""
    from scipy.spatial import Delaunay
    for s in range(400):
        c = cmo.cities(np.random.RandomState(50000 + s))
        ind, ptr = Delaunay(c).vertex_neighbor_vertices
        ref = sorted((i, int(j)) for i in range(len(c)) for j in ptr[ind[i]:ind[i + 1]] if i < j)
        got, amb = cmo.delaunay_edges(c)
        assert not amb
        assert got == ref, s


def test_cocircular_cities_are_reported():
    """Four cities on one circle (exactly cocircular in floating point: a square) are
    flagged instead of decided."""
    c = np.array([[0.0, 0.0], [10.0, 0.0], [10.0, 10.0], [0.0, 10.0], [30.0, 40.0], [-20.0, 35.0]])
    _, amb = cmo.delaunay_edges(c)
    assert amb


def test_road_length_is_numpy_norm():
    """np.linalg.norm of a (1, 2) difference is sqrt(x.dot(x)); the restatement's fused
    multiply-add form equals it on 20,000 city pairs (and differs from the unfused sum
    on some of them, so the form matters)."""
    rs = np.random.RandomState(3)
    differ = 0
    for _ in range(20000):
        p1, p2 = rs.uniform(-120, 120, size=(1, 2)), rs.uniform(-120, 120, size=(1, 2))
        d = p1 - p2
        ref = np.linalg.norm(d)
        assert cmo.road_length(p1[0], p2[0]) == ref
        differ += float(np.sqrt(d[0, 0] * d[0, 0] + d[0, 1] * d[0, 1])) != ref
    assert differ > 0


@pytest.mark.parametrize("arena", [(120, 120, 5.5), (57.3, 33, 5.5), (100, 80, 4.0), (120.5, 7.25, 5.5)])
def test_library_lattice_equals_generate_lattice(arena):
    """cov_map_lattice (the library's host code) against the restated generate_lattice,
    and at the reference's arena against its recorded lattice."""
    nat = pytest.importorskip("gym_flock._native")
    try:
        nat.load()
    except ImportError as e:
        pytest.skip(str(e))
    xm, ym, s = arena
    got = nat.map_lattice(nat.map_config_default(xmax=xm, ymax=ym, spacing=s))
    np.testing.assert_array_equal(got, cmo.lattice(-xm, xm, -ym, ym, s)[0])
    if arena == (120, 120, 5.5):
        np.testing.assert_array_equal(got, np.load(os.path.join(GOLDEN, "coverage_maps.npz"))["lattice"])


@pytest.mark.parametrize("n_cities", [3, 5, 20, 32])
def test_bruteforce_delaunay_equals_scipy_other_city_counts(n_cities):
    """As above for the city counts the device tests draw: 24 random sets each."""
    from scipy.spatial import Delaunay
    for s in range(24):
        c = cmo.cities(np.random.RandomState(60000 + 100 * n_cities + s), n_cities)
        ind, ptr = Delaunay(c).vertex_neighbor_vertices
        ref = sorted((i, int(j)) for i in range(len(c)) for j in ptr[ind[i]:ind[i + 1]] if i < j)
        got, amb = cmo.delaunay_edges(c)
        assert not amb
        assert got == ref, s


class _Given:
    """np.random stand-in for the host generator: the cities are given."""

    def __init__(self, c):
        self.c = c

    def uniform(self, lo, hi, size):
        assert tuple(size) == self.c.shape
        return self.c


@pytest.mark.parametrize("arena", cmi.ARENAS, ids=lambda a: "x".join(str(v) for v in a))
def test_restated_maps_equal_host_generator_other_arenas(arena):
    """Non-square arenas, spacing 4 and link radii from below the spacing to twice it: the
    restatement against the scipy host generator (oracle/maps_host.py), same cities."""
    from oracle.maps_host import generate_targets as host_targets
    xm, ym, sp, mr = arena
    c = cmi.arena_cities(xm, ym)
    t, amb = cmo.generate_targets(c, xm, ym, mr, sp)
    assert not amb
    np.testing.assert_array_equal(t, host_targets(xm, ym, sp, mr, rng=_Given(c)))
    assert (len(t) == 1) == (mr < sp)  # no link at all below the spacing


def test_cocircular_inputs_have_every_pair_as_a_road():
    """12 and 20 exactly cocircular cities: 66 and 190 roads, flagged; the 20-city map from
    only the first 96 roads (a planar triangulation's bound for 32 cities) is another map."""
    for c, n_edges, n_wp in ((cmi.cocircular12(), 66, 666), (cmi.cocircular20(), 190, 1846)):
        edges, amb = cmo.delaunay_edges(c)
        assert amb and len(edges) == n_edges == len(c) * (len(c) - 1) // 2
        assert len(cmo.waypoints(c, edges, 5.5 * 1.2)) == n_wp
    c = cmi.cocircular20()
    full, _ = cmo.generate_targets(c)
    np.testing.assert_array_equal(full, cmi.targets_from_first_edges(c, 190))
    cut = cmi.targets_from_first_edges(c, 96)
    assert (len(full), len(cut)) == (293, 278)
    assert len(cmo.generate_targets(cmi.cocircular12())[0]) == 277


def test_collinear_inputs():
    """12 collinear cities: no triangle, no road, flagged, 2 targets; the square plus a line
    of 8: 24 roads, flagged, 328 targets."""
    edges, amb = cmo.delaunay_edges(cmi.collinear12())
    assert amb and edges == []
    assert len(cmo.generate_targets(cmi.collinear12())[0]) == 2
    edges, amb = cmo.delaunay_edges(cmi.square_plus_line())
    assert amb and len(edges) == 24
    assert len(cmo.generate_targets(cmi.square_plus_line())[0]) == 328


def test_boundary_city_decides_the_lattice_point():
    """motion_radius 7.0: near_radius is exactly 5.0. The three city positions give squared
    distances to P of exactly 25, 25 + 1 ulp (root 5.0) and 25 + 2 ulp (root above 5.0), all
    within 2^-50 of 25; P is a target in the first two maps and not in the third, and the
    three maps differ in nothing else."""
    mr = cmi.BOUNDARY_MOTION_RADIUS
    assert mr / 1.4 == 5.0
    off = cmi.boundary_offsets()
    assert sorted(off) == ["above_far", "above_near", "exact"]
    ulp = np.spacing(25.0)
    sq = {k: cmi._sq(v) for k, v in off.items()}
    assert (sq["exact"], sq["above_near"], sq["above_far"]) == (25.0, 25.0 + ulp, 25.0 + 2 * ulp)
    assert np.sqrt(sq["above_near"]) == 5.0 < np.sqrt(sq["above_far"])
    assert all(25.0 * (1 - 2.0 ** -50) < s <= 25.0 * (1 + 2.0 ** -50) for s in sq.values())
    maps = {}
    for k, v in off.items():
        maps[k], amb = cmo.generate_targets(cmi.boundary_cities(v), motion_radius=mr)
        assert not amb
        assert cmi.has_point(maps[k], cmi.BOUNDARY_POINT) == (k != "above_far")
    np.testing.assert_array_equal(maps["exact"], maps["above_near"])
    keep = ~np.all(maps["exact"] == cmi.BOUNDARY_POINT[None], axis=1)
    np.testing.assert_array_equal(maps["exact"][keep], maps["above_far"])
