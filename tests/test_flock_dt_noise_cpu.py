"""The restatements behind the device's dt draws and variant resets (flock_dt_noise_numpy)
against NumPy's legacy RandomState and the reference's fixtures; no GPU.

Pins, before any device run: legacy_normal word for word (cache, straddled doubles, key
regenerations), the chain RandomState(41) -> reset -> 20 dts of variant_stochastic.npz, the
tolerance the GPU tests hold the device to (computed here from the oracle alone), and the
grid / leader resets against the variants' fixtures."""
import os

import numpy as np
import pytest

from conftest import GOLDEN

import flock_dt_noise_numpy as fdn
import flock_reset_numpy as frr


def same_state(a, b):
    assert a[0] == b[0] == "MT19937"
    np.testing.assert_array_equal(np.asarray(a[1], np.uint32), np.asarray(b[1], np.uint32))
    assert int(a[2]) == int(b[2]) and int(a[3]) == int(b[3]), (a[2:4], b[2:4])
    assert np.float64(a[4]).tobytes() == np.float64(b[4]).tobytes(), (a[4], b[4])


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


@pytest.mark.parametrize("seed", range(8))
def test_normal_is_randomstate_normal(seed):
    """1,001 draws: the odd count leaves has_gauss = 1."""
    rs = np.random.RandomState(seed)
    s = fdn.Stream(rs)
    got = np.array([s.normal(fdn.MEAN, fdn.SIGMA) for _ in range(1001)])
    want = np.array([rs.normal(fdn.MEAN, fdn.SIGMA) for _ in range(1001)])
    np.testing.assert_array_equal(bits(got), bits(want))
    assert s.has_gauss == 1
    same_state(s.state(), rs.get_state())


@pytest.mark.parametrize("pos", [0, 1, 622, 623, 624])
@pytest.mark.parametrize("cached", [False, True])
def test_normal_from_every_kind_of_position(pos, cached):
    """Positions at which a double straddles the key's regeneration (623), starts it (624)
    or ends on its last word (622), with and without a cached Gaussian."""
    key = np.random.RandomState(100 + pos).get_state()[1]
    state = ("MT19937", key, pos, 1, -0.4375) if cached else ("MT19937", key, pos, 0, 0.0)
    rs = fdn.random_state(state)
    s = fdn.Stream(state)
    got = np.array([s.normal() for _ in range(9)])
    want = np.array([rs.normal(fdn.MEAN, fdn.SIGMA) for _ in range(9)])
    np.testing.assert_array_equal(bits(got), bits(want))
    if cached:
        assert got[0] == fdn.MEAN + fdn.SIGMA * -0.4375
    same_state(s.state(), rs.get_state())


def test_sigma_zero_still_consumes_the_stream():
    rs = np.random.RandomState(3)
    s = fdn.Stream(rs)
    assert [s.normal(0.12, 0.0) for _ in range(3)] == [rs.normal(0.12, 0.0) for _ in range(3)] == [0.12] * 3
    same_state(s.state(), rs.get_state())


@pytest.fixture(scope="module")
def stochastic():
    return np.load(os.path.join(GOLDEN, "variant_stochastic.npz"))


def test_fixture_chain(stochastic):
    """RandomState(41): the reset at N = 10 takes 27 tries and gives the fixture's x0; the
    next 20 normals are its dt[:20]; the stream then stands at pos 448 without a cache."""
    f = stochastic
    rs = np.random.RandomState(int(f["seed"]))
    r = frr.reset_rejection(rs, 10)
    assert r["tries"] == 27 and r["accepted"]
    np.testing.assert_array_equal(bits(r["x"]), bits(f["x0"]))
    s = fdn.Stream(r["state"])
    got = np.array([s.normal() for _ in range(20)])
    np.testing.assert_array_equal(bits(got), bits(f["dt"][:20]))
    np.testing.assert_array_equal(bits([rs.normal(fdn.MEAN, fdn.SIGMA) for _ in range(20)]), bits(f["dt"][:20]))
    assert (s.pos, s.has_gauss) == (448, 0)
    same_state(s.state(), rs.get_state())


def test_tolerance_against_the_fixture_states(stochastic):
    """D, from the oracle alone: its closed loop with every dt moved by its bound, 64 sign
    patterns. The oracle's own distance from the fixture's states (summation order) has to
    lie well inside the 4 D the GPU test allows the device."""
    f = stochastic
    d, base = fdn.rollout_sensitivity(f["x0"], f["dt"][:20])
    own = float(np.abs(base - f["x"][:20]).max())
    print("D = %.3e (dt bound at most %.3e), oracle's own distance from the fixture %.3e"
          % (d, fdn.dt_bound(f["dt"][:20]).max(), own))
    assert 0 < d < 1e-12
    assert own <= d


def test_grid_resets_equal_the_fixtures():
    f = np.load(os.path.join(GOLDEN, "variant_twoflocks.npz"))
    rs = np.random.RandomState(int(f["seed"]))
    s = fdn.Stream(rs)
    x = fdn.twoflocks_reset(s, 20)
    np.testing.assert_array_equal(bits(x), bits(f["x0"]))
    rs.uniform(size=2)
    same_state(s.state(), rs.get_state())
    g = np.load(os.path.join(GOLDEN, "variant_obstacle.npz"))
    np.testing.assert_array_equal(bits(fdn.obstacle_reset(100)), bits(g["x0"]))
    assert fdn.twoflocks_ok(20) and fdn.twoflocks_ok(100) and not fdn.twoflocks_ok(25) and not fdn.twoflocks_ok(9)


def test_leader_reset_equals_the_fixture():
    f = np.load(os.path.join(GOLDEN, "variant_leader.npz"))
    r = fdn.leader_reset(np.random.RandomState(int(f["seed"])), 12)
    np.testing.assert_array_equal(bits(r["x"]), bits(f["x0"]))
    assert r["x"][0, 2] == r["x"][0, 3] == r["x"][1, 2] == r["x"][1, 3] == r["w"]
    # every decision of the loop far from its threshold: the device's cos / sin cannot flip one
    assert r["dist_margin"].min() > frr.MARGIN and r["a_margin"].min() > frr.MARGIN
