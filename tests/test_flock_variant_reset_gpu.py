"""The variants' resets on the device (fe_reset_variant, flock_vreset_kernel;
VecFlockingRelative.reset_device(kind=...)) against the reference's fixtures and the
restatements in flock_dt_noise_numpy. Needs an MI355X.

The grid resets (TwoFlocks, Obstacle) are exact: products and sums of a few doubles in the
reference's order. Leader is the relative rejection reset, so its try count, stream and
velocities are exact and its positions carry the device's cos / sin, held to
test_flock_reset_gpu's POS_RTOL."""
import os

import numpy as np
import pytest

from conftest import GOLDEN

import flock_dt_noise_numpy as fdn

pytestmark = pytest.mark.gpu

nat = pytest.importorskip("gym_flock._native")
from gym_flock.init_states import synthetic_batch  # noqa: E402
from gym_flock.vec import VecFlockingRelative  # noqa: E402
from test_flock_reset_gpu import POS_RTOL  # noqa: E402


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def same_stream(v, b, want, what=""):
    got = v.h.get_rng_state(b)
    np.testing.assert_array_equal(got[1], want[1], err_msg=what)
    assert got[2:4] == tuple(want[2:4]) and got[4] == want[4], (what, got[2:], want[2:])


def check_leader(x, r, what):
    """Velocities (the leaders' w among them) bit for bit, positions at the device's cos / sin."""
    np.testing.assert_array_equal(bits(x[:, 2:]), bits(r["x"][:, 2:]), err_msg=what)
    np.testing.assert_allclose(x[:, :2], r["x"][:, :2], rtol=POS_RTOL, atol=0, err_msg=what)


def test_twoflocks_fixture():
    f = np.load(os.path.join(GOLDEN, "variant_twoflocks.npz"))
    v = VecFlockingRelative(1, 20, variant="twoflocks")
    tries, status = v.reset_device(seed=51, kind="twoflocks")
    assert tries[0] == 1 and status[0] == 0
    np.testing.assert_array_equal(bits(v.get_state()[0]), bits(f["x0"]))
    rs = np.random.RandomState(51)
    rs.uniform(size=2)
    same_stream(v, 0, rs.get_state())
    np.testing.assert_allclose(v.state_values(0), f["sv0"], rtol=1e-5, atol=1e-8)  # compute_helpers() ran
    v.close()


def test_obstacle_fixture():
    f = np.load(os.path.join(GOLDEN, "variant_obstacle.npz"))
    v = VecFlockingRelative(1, 100, variant="obstacle")
    tries, status = v.reset_device(kind="obstacle")  # no draws: no stream needed
    assert tries[0] == 1 and status[0] == 0
    np.testing.assert_array_equal(bits(v.get_state()[0]), bits(f["x0"]))
    with pytest.raises(nat.GymFlockError) as e:
        v.h.get_rng(0)
    assert e.value.code == nat.GF_ESTATE
    v.reset_device(seed=7, kind="obstacle")  # seeds the stream, draws nothing
    np.testing.assert_array_equal(bits(v.get_state()[0]), bits(f["x0"]))
    same_stream(v, 0, np.random.RandomState(7).get_state())
    v.close()


def test_leader_fixture():
    f = np.load(os.path.join(GOLDEN, "variant_leader.npz"))
    r = fdn.leader_reset(np.random.RandomState(31), 12)
    v = VecFlockingRelative(1, 12, variant="leader")
    tries, status = v.reset_device(seed=31, kind="leader")
    assert tries[0] == r["tries"] and status[0] == 0
    x = v.get_state()[0]
    check_leader(x, r, "leader fixture")
    assert x[0, 2] == x[0, 3] == x[1, 2] == x[1, 3] == r["w"] == f["x0"][0, 2]
    np.testing.assert_array_equal(bits(x[:, 2:]), bits(f["x0"][:, 2:]))
    same_stream(v, 0, r["state"])
    v.close()


@pytest.mark.parametrize("kind,n", [("leader", 12), ("twoflocks", 30)])
def test_batch_of_three_and_a_masked_reset(kind, n):
    """Env b on RandomState(seed + b); then a masked, continued reset of env 1 alone: the
    other envs' state, stream, tries and status stay bit-identical."""
    B, seed = 3, 900
    v = VecFlockingRelative(B, n, variant=kind)
    tries, status = v.reset_device(seed=seed, kind=kind)
    x = v.get_state()
    want = []
    for b in range(B):
        rs = np.random.RandomState(seed + b)
        if kind == "leader":
            r = fdn.leader_reset(rs, n)
            check_leader(x[b], r, "env %d" % b)
            assert tries[b] == r["tries"]
        else:
            s = fdn.Stream(rs)
            r = dict(x=fdn.twoflocks_reset(s, n), state=s.state())
            np.testing.assert_array_equal(bits(x[b]), bits(r["x"]))
            assert tries[b] == 1
        assert status[b] == 0
        same_stream(v, b, r["state"], "env %d" % b)
        want.append(r)
    streams = [v.h.get_rng_state(b) for b in range(B)]
    tries2, status2 = v.reset_device(envs=[1], kind=kind)  # continued
    x2 = v.get_state()
    for b in (0, 2):
        np.testing.assert_array_equal(bits(x2[b]), bits(x[b]))
        same_stream(v, b, streams[b], "env %d untouched" % b)
        assert tries2[b] == tries[b] and status2[b] == status[b]
    rs = fdn.random_state(want[1]["state"])
    if kind == "leader":
        r = fdn.leader_reset(rs, n)
        check_leader(x2[1], r, "env 1 again")
        assert tries2[1] == r["tries"]
        same_stream(v, 1, r["state"], "env 1 again")
    else:
        s = fdn.Stream(rs)
        np.testing.assert_array_equal(bits(x2[1]), bits(fdn.twoflocks_reset(s, n)))
        same_stream(v, 1, s.state(), "env 1 again")
    v.close()


def test_refusals():
    v = VecFlockingRelative(2, 25)
    v.reset(x=synthetic_batch(2, 25, seed0=1))
    with pytest.raises(nat.GymFlockError) as e:
        v.reset_device(seed=1, kind="twoflocks")  # side = 2 does not divide 25
    assert e.value.code == nat.GF_EINVAL
    v.close()
    v = VecFlockingRelative(2, 12)
    x0 = synthetic_batch(2, 12, seed0=2)
    v.reset(x=x0)
    with pytest.raises(nat.GymFlockError) as e:
        v.reset_device(kind="obstacle")  # 12 is no multiple of 5
    assert e.value.code == nat.GF_EINVAL
    v2 = VecFlockingRelative(2, 20)
    with pytest.raises(nat.GymFlockError) as e:
        v2.h.reset_device(kind="obstacle", n_special=3)
    assert e.value.code == nat.GF_EINVAL
    with pytest.raises(nat.GymFlockError) as e:
        v2.reset_device(kind="twoflocks")  # continued, but no stream yet
    assert e.value.code == nat.GF_ESTATE
    with pytest.raises(ValueError):
        v2.reset_device(kind="threeflocks")
    np.testing.assert_array_equal(bits(v.get_state()), bits(x0))  # the refused calls changed nothing
    v.close()
    v2.close()
