"""cov_generate_maps (gym-flock_amd/csrc/coverage_maps.hip) where random cities in a square
default arena never take it: exactly cocircular and collinear cities (the near-degenerate
branches, more roads than a planar triangulation has), every refusal status inside a batch,
3 to 32 cities drawn on the device, one env of a batch, non-square arenas with other
spacings and link radii, the rounding window of the near-road test, and road lengths that
would overflow the waypoint count. Everything is compared bit for bit with the restatement
of the device algorithm (oracle/coverage_maps.py), which tests/test_oracle_coverage_maps.py
pins on the CPU for these very inputs (tests/coverage_map_inputs.py). Needs an MI355X."""
import os
import sys

import numpy as np
import pytest

from conftest import GOLDEN
from oracle import coverage_maps as cmo
from oracle.maps_host import generate_targets as host_targets

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import coverage_map_inputs as cmi  # noqa: E402

pytestmark = pytest.mark.gpu

nat = pytest.importorskip("gym_flock._native")

REFUSED = nat.COV_MAP_TOO_MANY | nat.COV_MAP_TOO_FEW | nat.COV_MAP_OVERFLOW


def _same_map(h, b, n, st, c, **kw):
    """Env b's map (n targets, status st) is the restatement's map of the cities c."""
    ref, amb = cmo.generate_targets(c, **kw)
    assert n == len(ref), (b, n, len(ref))
    np.testing.assert_array_equal(h.targets(b, n), ref, err_msg="env %d" % b)
    assert not (st & REFUSED) and bool(st & nat.COV_MAP_NEAR_DEGENERATE) == amb, (b, st, amb)
    return ref, amb


class _Given:
    """np.random stand-in for the host generator: the cities are given."""

    def __init__(self, c):
        self.c = c

    def uniform(self, lo, hi, size):
        assert tuple(size) == self.c.shape
        return self.c


# ---- a. cocircular and collinear cities

@pytest.mark.parametrize("name", ["cocircular12", "cocircular20", "square_plus_line"])
def test_degenerate_cities_match_restatement(name):
    """Every triple of cocircular cities has an empty circumcircle, decided 'unsure': all
    NC (NC - 1) / 2 pairs are roads (66 for 12 cities; 190 for 20, twice what a planar
    triangulation of 32 cities has), and the status says NEAR_DEGENERATE. A road list of 96
    entries, which the kernel once had, gives 278 targets for the 20 cities instead of 293
    (measured on an MI355X with that kernel; the same count on the CPU in
    test_oracle_coverage_maps.py). The square plus a line of 8 takes the collinear skip and
    the unsure branch in one map."""
    c = getattr(cmi, name)()
    h = nat.CoverageHandle(6, 1, 500)
    n, st, co = h.generate_maps(cities=c[None], env=0, map_config=nat.map_config_default(n_cities=len(c)))
    np.testing.assert_array_equal(co[0], c)
    ref, amb = _same_map(h, 0, n[0], st[0], c)
    assert amb and 200 < len(ref) < 400
    h.close()


def test_collinear_cities_too_few():
    """12 collinear cities have no triangle and no road: 2 targets. With 6 robots the map is
    refused (TOO_FEW, and NEAR_DEGENERATE from the collinear triples); 2 robots get it."""
    c = cmi.collinear12()
    ref, amb = cmo.generate_targets(c)
    assert amb and len(ref) == 2
    h = nat.CoverageHandle(6, 1, 500)
    with pytest.raises(nat.GymFlockError) as e:
        h.generate_maps(cities=c[None], env=0)
    assert e.value.code == nat.GF_EINVAL and "env 0" in str(e.value) and "fewer than the robots" in str(e.value)
    assert e.value.status[0] == nat.COV_MAP_TOO_FEW | nat.COV_MAP_NEAR_DEGENERATE
    assert e.value.n_targets[0] == 2
    h.close()
    h = nat.CoverageHandle(2, 1, 500)
    n, st, _ = h.generate_maps(cities=c[None], env=0)
    _same_map(h, 0, n[0], st[0], c)
    h.close()


# ---- b. a refused env inside a batch

def test_overflow_in_a_batch_leaves_the_other_envs_their_maps():
    """world_radius 10 bounds the waypoints at 162; env 1's given cities span +-100 and need
    241. Env 1 alone is OVERFLOW and left without a map; envs 0 and 2 keep theirs."""
    R = 6
    mc = nat.map_config_default(xmax=30, ymax=30)
    mc.world_radius = 10.0
    c = np.stack([np.random.RandomState(100).uniform(-10, 10, (12, 2)),
                  np.random.RandomState(5).uniform(-100, 100, (12, 2)),
                  np.random.RandomState(102).uniform(-10, 10, (12, 2))])
    refs = [cmo.generate_targets(c[b], 30, 30) for b in (0, 2)]
    assert all(len(t) >= R and not amb for t, amb in refs)
    assert len(cmo.waypoints(c[1], cmo.delaunay_edges(c[1])[0], 6.6)) == 241
    h = nat.CoverageHandle(R, 3, 500)
    with pytest.raises(nat.GymFlockError) as e:
        h.generate_maps(cities=c, map_config=mc)
    assert e.value.code == nat.GF_EINVAL and "env 1" in str(e.value) and "more road waypoints" in str(e.value)
    np.testing.assert_array_equal(e.value.status, [0, nat.COV_MAP_OVERFLOW, 0])
    np.testing.assert_array_equal(e.value.n_targets, [len(refs[0][0]), 0, len(refs[1][0])])
    for b, (t, _) in zip((0, 2), refs):
        np.testing.assert_array_equal(h.targets(b, len(t)), t)
    with pytest.raises(nat.GymFlockError) as e:
        h.targets(1, 1)
    assert e.value.code == nat.GF_ESTATE and "no target map" in str(e.value)
    h.close()


# ---- c. other city counts, drawn on the device

@pytest.mark.parametrize("n_cities", [3, 5, 20, 32])
def test_device_drawn_city_counts(n_cities):
    """3 to 32 cities (adjacency masks up to bit 31, 2 n draws per env): the cities are
    RandomState(b)'s, the maps the restatement's, and the next call continues each stream
    after exactly 2 n uniforms."""
    B = 2
    mc = nat.map_config_default(n_cities=n_cities)
    h = nat.CoverageHandle(6, B, 1900)
    rs = [np.random.RandomState(b) for b in range(B)]
    for seed in (0, None):
        n, st, c = h.generate_maps(map_seed=seed, map_config=mc)
        for b in range(B):
            np.testing.assert_array_equal(c[b], cmo.cities(rs[b], n_cities))
            ref, _ = _same_map(h, b, n[b], st[b], c[b])
            if seed == 0 and b == 0:
                assert len(ref) == {3: 34, 5: 141, 20: 689, 32: 936}[n_cities]
    h.close()


# ---- d. one env of a batch

def test_one_env_of_a_batch():
    """generate_maps(env=k) on a handle of 4: only env k's stream, cities, map and graph
    move, for device-drawn and for given cities."""
    f = np.load(os.path.join(GOLDEN, "coverage_maps.npz"))
    lat, nxt, o = f["lattice"], [], 0
    for m in f["next_len"]:
        nxt.append(lat[f["next_idx"][o:o + m]])
        o += m
    B = 4
    h = nat.CoverageHandle(6, B, 1000)
    rs = [np.random.RandomState(b) for b in range(B)]
    n, _, c = h.generate_maps(map_seed=0)
    for b in range(B):
        np.testing.assert_array_equal(c[b], cmo.cities(rs[b]))
    cur = [h.targets(b, n[b]) for b in range(B)]
    nm = h.n_motion()

    def others_unchanged(k):
        got = h.n_motion()
        for b in range(B):
            if b != k:
                np.testing.assert_array_equal(h.targets(b, len(cur[b])), cur[b])
                assert got[b] == nm[b]

    n2, st2, c2 = h.generate_maps(env=2)  # env 2's second map; the other streams stay
    assert n2.shape == (1,) and st2[0] == 0
    np.testing.assert_array_equal(c2[0], cmo.cities(rs[2]))
    np.testing.assert_array_equal(h.targets(2, n2[0]), nxt[2])
    others_unchanged(2)

    n3, st3, c3 = h.generate_maps()  # envs 0, 1, 3: their second map; env 2: its third
    for b in range(B):
        np.testing.assert_array_equal(c3[b], cmo.cities(rs[b]))
        if b == 2:
            _same_map(h, b, n3[b], st3[b], c3[b])
        else:
            np.testing.assert_array_equal(h.targets(b, n3[b]), nxt[b])
    cur = [h.targets(b, n3[b]) for b in range(B)]
    nm = h.n_motion()

    given = cmo.cities(np.random.RandomState(77))
    n4, st4, c4 = h.generate_maps(cities=given[None], env=3)
    np.testing.assert_array_equal(c4[0], given)
    _same_map(h, 3, n4[0], st4[0], given)
    others_unchanged(3)
    _, _, c5 = h.generate_maps()  # no stream moved for the given cities, env 3's included
    for b in range(B):
        np.testing.assert_array_equal(c5[b], cmo.cities(rs[b]))
    h.close()


# ---- e. non-default arenas, spacings and link radii

@pytest.mark.parametrize("arena", cmi.ARENAS, ids=lambda a: "x".join(str(v) for v in a))
def test_other_arenas_spacings_and_link_radii(arena):
    """Non-square arenas (the cell grid's NJ comes from arange(-ny, nx)), spacing 4, and link
    radii from below the spacing (K = 1: no link, one target) to twice it (K = 3)."""
    xm, ym, sp, mr = arena
    c = cmi.arena_cities(xm, ym)
    ref, amb = cmo.generate_targets(c, xm, ym, mr, sp)
    assert not amb and 1 <= len(ref) <= 400
    np.testing.assert_array_equal(ref, host_targets(xm, ym, sp, mr, rng=_Given(c)))
    # the handle's own motion graph (built after the map) stays within degree 4
    h = nat.CoverageHandle(2, 1, 500, res=sp, motion_radius=mr if mr < sp * 1.4 else sp * 1.2)
    mc = nat.map_config_default(mr, xm, ym, spacing=sp)
    if len(ref) >= 2:
        n, st, _ = h.generate_maps(cities=c[None], env=0, map_config=mc)
        _same_map(h, 0, n[0], st[0], c, xmax=xm, ymax=ym, motion_radius=mr, spacing=sp)
    else:
        with pytest.raises(nat.GymFlockError) as e:
            h.generate_maps(cities=c[None], env=0, map_config=mc)
        assert e.value.code == nat.GF_EINVAL and e.value.status[0] == nat.COV_MAP_TOO_FEW
        assert e.value.n_targets[0] == len(ref) == 1
    h.close()


# ---- f. the rounding window of the near-road test

def test_near_road_rounding_window():
    """near_radius exactly 5.0 and a city at the lattice point P + (3, 4): squared distance
    exactly 25 (near), 1 ulp above with a root that rounds to 5.0 (near) and 2 ulps above
    with a root above 5.0 (not near). All three lie between the kernel's n2lo and n2hi, where
    the square root decides; P is in the map in the first two and out in the third."""
    mr = cmi.BOUNDARY_MOTION_RADIUS
    mc = nat.map_config_default(mr)
    assert mc.near_radius == 5.0
    h = nat.CoverageHandle(6, 1, 500, motion_radius=mr)
    for key, first in sorted(cmi.boundary_offsets().items()):
        c = cmi.boundary_cities(first)
        n, st, _ = h.generate_maps(cities=c[None], env=0, map_config=mc)
        ref, _ = _same_map(h, 0, n[0], st[0], c, motion_radius=mr)
        got = h.targets(0, n[0])
        assert cmi.has_point(got, cmi.BOUNDARY_POINT) == cmi.has_point(ref, cmi.BOUNDARY_POINT) == (key != "above_far")
    h.close()


# ---- waypoint counts that do not fit an int, cities that are not numbers

def test_non_finite_given_cities_are_refused():
    """A NaN or infinite given city: GF_EINVAL before any launch; the handle works after."""
    good = cmo.cities(np.random.RandomState(3))
    h = nat.CoverageHandle(6, 2, 1000)
    for bad in (np.nan, np.inf, -np.inf):
        c = np.stack([good, good])
        c[1, 11, 1] = bad
        with pytest.raises(nat.GymFlockError) as e:
            h.generate_maps(cities=c)
        assert e.value.code == nat.GF_EINVAL and "NaN or an infinity" in str(e.value)
    n, st, _ = h.generate_maps(cities=np.stack([good, good]))
    for b in range(2):
        _same_map(h, b, n[b], st[b], good)
    h.close()


def test_unbounded_waypoint_counts_are_overflow():
    """A road 1e12 long, or roads cut every 1e-8: int(dist / road_radius) is far above the
    capacity (and above INT_MAX for the first). Both are COV_MAP_OVERFLOW, nothing is
    written, and the handle works after."""
    good = cmo.cities(np.random.RandomState(3))
    far = good.copy()
    far[4] = [1e12, 0.0]
    tiny = nat.map_config_default()
    tiny.road_radius = 1e-8
    h = nat.CoverageHandle(6, 1, 1000)
    for c, mc in ((far, None), (good, tiny)):
        with pytest.raises(nat.GymFlockError) as e:
            h.generate_maps(cities=c[None], env=0, map_config=mc)
        assert e.value.code == nat.GF_EINVAL and "more road waypoints" in str(e.value)
        assert e.value.status[0] & REFUSED == nat.COV_MAP_OVERFLOW and e.value.n_targets[0] == 0
    n, st, _ = h.generate_maps(cities=good[None], env=0)
    _same_map(h, 0, n[0], st[0], good)
    h.close()
