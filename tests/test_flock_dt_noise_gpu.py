"""FlockingStochastic-v0's per-step dt drawn on the device (fe_set_dt_noise,
flock_dt_noise_kernel, the rollout's dt table) against NumPy's legacy normal, the
reference's fixture and the engine's own single step. Needs an MI355X.

What is exact and what is not: the stream (key, position, has_gauss) is NumPy's word for
word; a dt carries the device's log and lies within flock_dt_noise_numpy.dt_bound of
NumPy's; given the device's own dts the rollout is the single step bit for bit (state,
adjacency bits, degree) and the oracle's integrate bit for bit. Against the fixture's
states the allowance is 4 D, D computed here from the oracle alone (rollout_sensitivity;
1.07e-14 with sign seed 0)."""
import os

import numpy as np
import pytest

from conftest import GOLDEN

import flock_dt_noise_numpy as fdn
import flock_rollout_numpy as frn

pytestmark = pytest.mark.gpu

nat = pytest.importorskip("gym_flock._native")
from gym_flock.init_states import synthetic_batch  # noqa: E402
from gym_flock.vec import VecFlockingRelative  # noqa: E402
from oracle import flocking_variants as fv  # noqa: E402

ALL = frn.RECORDS + ("dt",)
MEAN, SIGMA = fdn.MEAN, fdn.SIGMA


def noisy(B, n, noise=(MEAN, SIGMA)):
    return VecFlockingRelative(B, n, variant="stochastic", dt_noise=noise)


def equal_records(a, b, keys=ALL):
    for k in keys:
        assert a[k].shape == b[k].shape and a[k].dtype == b[k].dtype, k
        np.testing.assert_array_equal(np.ascontiguousarray(a[k]).view(np.uint8),
                                      np.ascontiguousarray(b[k]).view(np.uint8), err_msg=k)


def numpy_dts(state, n, mean=MEAN, sigma=SIGMA):
    """n normals of a RandomState at `state`, and its state afterwards."""
    rs = fdn.random_state(state)
    return np.array([rs.normal(mean, sigma) for _ in range(n)]), rs.get_state()


def check_stream(v, b, want, what):
    """Key, position and has_gauss exact; the cached Gaussian within the log's allowance."""
    got = v.h.get_rng_state(b)
    np.testing.assert_array_equal(got[1], want[1], err_msg=what)
    assert (got[2], got[3]) == (want[2], want[3]), (what, got[2:4], want[2:4])
    assert abs(got[4] - want[4]) <= fdn.gauss_bound(want[4]), (what, got[4], want[4])


def check_dts(got, want, what, mean=MEAN, sigma=SIGMA):
    bound = fdn.dt_bound(want, mean, sigma)
    frac = float(np.max(np.abs(got - want) / bound))
    print("%s: largest |dt - NumPy's| is %.3f of its bound" % (what, frac))
    assert (np.abs(got - want) <= bound).all(), (what, got, want)
    return frac


# ------------------------------------------------------------------ 1. the fixture's chain
def test_fixture_chain():
    """reset_device(seed=41), controller(), 20 recorded steps: variant_stochastic.npz's reset
    (27 tries), its 20 dts, its states, and RandomState(41)'s stream afterwards."""
    f = np.load(os.path.join(GOLDEN, "variant_stochastic.npz"))
    v = noisy(1, 10)
    tries, status = v.reset_device(seed=41)
    assert tries[0] == 27 and status[0] == 0
    v.controller()
    rec = v.expert_steps(20, record=ALL)
    assert rec["dt"].shape == (20, 1)
    check_dts(rec["dt"][:, 0], f["dt"][:20], "fixture chain")
    d, _ =fdn.rollout_sensitivity(f["x0"], f["dt"][:20])
    dev = float(np.abs(rec["x"][:, 0] - f["x"][:20]).max())
    print("D = %.3e, the rollout's largest distance from the fixture's states %.3e (%.2f D)" % (d, dev, dev / d))
    assert dev <= 4 * d
    rs = np.random.RandomState(41)
    fdn.frn_reset.reset_rejection(rs, 10)
    _, want = numpy_dts(rs.get_state(), 20)
    assert (want[2], want[3]) == (448, 0)
    check_stream(v, 0, want, "fixture chain")
    assert v.np_random(0).normal() == fdn.random_state(want).normal()
    v.close()


# ------------------------------------------------- 2. exact, given the device's own dts
@pytest.mark.parametrize("n,steps", [(10, 20), (65, 8), (129, 8)])
def test_rollout_is_the_single_step_with_the_recorded_dts(n, steps):
    """One size per column-chunk instantiation, three envs on different streams (their dts
    differ inside one launch). Every recorded step is the oracle's integrate of the step
    before with the recorded dt, bit for bit; a twin without the mode, stepped once per
    step with the recorded dts, gives the same states, adjacency bits and degrees bit for
    bit and the other outputs within the rollout tests' tolerances.

    The twin takes every step from the rollout's recorded state and controls (float64
    actions): the single step's controller sums in another order than the rollout's (the
    header's "controls up to summation order"), so a twin that feeds back its OWN controls
    (step(expert=True)) leaves the rollout after the first step whatever the dt is. Measured
    with a fixed dt, before this mode existed and with it alike: at N = 10 two control
    words differ by up to 13 ulp after step 1, and the states part at step 1 (relative,
    N = 10 and 65; stochastic, N = 65) or step 8 (stochastic, N = 10, where the clip at 0.5
    hides most differences). The closed loop is therefore also checked as far as it can
    be: a second twin feeds back its own controls and must stay on the rollout bit for bit
    for as long as those controls are the rollout's bits (the first step at least)."""
    B = 3
    v = noisy(B, n)
    v.reset_device(seed=200 + n, reject=False)
    x0, u0 = v.get_state(), v.controller()
    rec = v.expert_steps(steps, record=ALL)
    dt = rec["dt"]
    assert dt.shape == (steps, B) and len(np.unique(dt)) == steps * B
    assert (np.abs(dt - MEAN) < 8 * SIGMA).all()
    x, u = x0, u0
    for t in range(steps):
        for b in range(B):
            frn.same_bits(rec["x"][t, b], fv.integrate(x[b], u[b], dt[t, b], **fdn.STOCH), "integrate, step %d env %d" % (t, b))
        x, u = rec["x"][t], rec["controls"][t]
    w = VecFlockingRelative(B, n, variant="stochastic")
    w.reset(x=x0)
    w.controller()
    closed = 0  # steps the closed-loop twin was fed the rollout's own bits
    for t in range(steps):
        if not np.array_equal(w.controls().view(np.uint64), (rec["controls"][t - 1] if t else u0).view(np.uint64)):
            break
        w.step(expert=True, controller=True, network="packed", dt=dt[t])
        frn.same_bits(rec["x"][t], w.get_state(), "closed loop, step %d" % t)
        closed += 1
    print("N = %d: the closed-loop twin was fed the rollout's controls for %d of %d steps" % (n, closed, steps))
    assert closed >= 1
    for t in range(steps):
        w.set_state(rec["x"][t - 1] if t else x0)
        w.step(rec["controls"][t - 1] if t else u0, controller=True, network="packed", dt=dt[t])
        bits, deg = w.network_packed()
        frn.same_bits(rec["x"][t], w.get_state(), "state, step %d" % t)
        np.testing.assert_array_equal(rec["adj_bits"][t], bits)
        np.testing.assert_array_equal(rec["degree"][t], deg)
        frn.close(rec["state_values"][t], w.state_values(), frn.SV_RTOL, frn.SV_ATOL, "state_values")
        frn.close(rec["controls"][t], w.controls(), frn.CTRL_RTOL, frn.CTRL_ATOL, "controls")
        frn.close(rec["rewards"][t], w.rewards(), frn.REWARD_RTOL, 0.0, "rewards")
    v.close()
    w.close()


# -------------------------------------------------------------------- 3. stream mechanics
@pytest.fixture(scope="module")
def twenty():
    """(x0, the recording of 20 steps, the streams afterwards) at B = 2, N = 10."""
    v = noisy(2, 10)
    v.reset_device(seed=300, reject=False)
    x0 = v.get_state()
    v.controller()
    rec = v.expert_steps(20, record=ALL)
    states = [v.h.get_rng_state(b) for b in range(2)]
    v.close()
    for a in rec.values():
        a.setflags(write=False)
    return x0, rec, states


def same_state(a, b):
    np.testing.assert_array_equal(a[1], b[1])
    assert a[2:4] == b[2:4] and np.float64(a[4]).tobytes() == np.float64(b[4]).tobytes(), (a[2:], b[2:])


def test_two_launches_equal_one(twenty):
    """7 + 13 steps: an odd first count, so the cached Gaussian crosses the launches."""
    x0, rec, states = twenty
    v = noisy(2, 10)
    v.reset_device(seed=300, reject=False)
    v.controller()
    a = v.expert_steps(7, record=ALL)
    assert v.h.get_rng_state(0)[3] == 1
    b = v.expert_steps(13, record=ALL)
    equal_records({k: np.concatenate([a[k], b[k]]) for k in ALL}, rec)
    for e in range(2):
        same_state(v.h.get_rng_state(e), states[e])
    v.close()


def test_twenty_single_steps_draw_the_same_dts(twenty):
    x0, rec, states = twenty
    v = noisy(2, 10)
    v.reset_device(seed=300, reject=False)
    v.controller()
    for t in range(20):
        v.step(expert=True, controller=True, network="packed")
        d = v.h.dt_steps()
        assert d.shape == (1, 2)
        np.testing.assert_array_equal(d[0].view(np.uint64), rec["dt"][t].view(np.uint64), err_msg="step %d" % t)
    for e in range(2):
        same_state(v.h.get_rng_state(e), states[e])
    v.close()


def test_streams_set_at_awkward_positions():
    """A straddled double (pos 623), a regeneration before the first word (624), a cached
    Gaussian, and a key that regenerates inside the launch (3 words left)."""
    keys = [np.random.RandomState(400 + b).get_state()[1] for b in range(4)]
    states = [("MT19937", keys[0], 623, 0, 0.0), ("MT19937", keys[1], 624, 0, 0.0),
              ("MT19937", keys[2], 100, 1, 0.625), ("MT19937", keys[3], 621, 0, 0.0)]
    v = noisy(4, 10)
    v.reset(x=synthetic_batch(4, 10, seed0=410))
    v.h.set_rng(states)
    for b in range(4):
        same_state(v.h.get_rng_state(b), states[b])
    v.controller()
    rec = v.expert_steps(5, record=("dt",))
    for b in range(4):
        want, after = numpy_dts(states[b], 5)
        check_dts(rec["dt"][:, b], want, "env %d" % b)
        check_stream(v, b, after, "env %d" % b)
    assert rec["dt"][0, 2] == MEAN + SIGMA * 0.625
    v.close()


def test_sigma_zero_consumes_the_stream():
    v = noisy(2, 10, noise=(0.11, 0.0))
    v.reset_device(seed=500, reject=False)
    before = [v.h.get_rng_state(b) for b in range(2)]
    v.controller()
    rec = v.expert_steps(3, record=("dt",))
    assert (rec["dt"] == 0.11).all()
    for b in range(2):
        check_stream(v, b, numpy_dts(before[b], 3, 0.11, 0.0)[1], "env %d" % b)
    v.close()


def test_resets_and_the_cached_gaussian():
    """A continued reset leaves the cache (uniform does not touch it), a seeded one clears
    it, and a masked one leaves the other env's stream and cache alone."""
    v = noisy(2, 10)
    v.reset_device(seed=600, reject=False)
    v.controller()
    v.expert_steps(3, fetch=False)
    st = [v.h.get_rng_state(b) for b in range(2)]
    assert st[0][3] == 1 and st[1][3] == 1 and st[0][4] != 0.0
    v.reset_device(seed=None, reject=False)  # continued
    for b in range(2):
        got = v.h.get_rng_state(b)
        p = st[b][2] + 84  # one candidate at N = 10: 8 N + 4 words
        assert got[3] == 1 and got[4] == st[b][4] and got[2] == (p if p <= 624 else p - 624)
    v.controller()
    rec = v.expert_steps(1, record=("dt",))
    np.testing.assert_array_equal(rec["dt"][0], [MEAN + SIGMA * st[0][4], MEAN + SIGMA * st[1][4]])
    v.expert_steps(1, fetch=False)
    st = [v.h.get_rng_state(b) for b in range(2)]
    assert st[0][3] == 1 and st[1][3] == 1
    v.reset_device(seed=700, envs=[1], reject=False)  # masked and seeded
    same_state(v.h.get_rng_state(0), st[0])
    got = v.h.get_rng_state(1)
    rs = np.random.RandomState(701)
    fdn.frn_reset.reset_rejection(rs, 10, reject=False)
    same_state(got, rs.get_state())
    assert got[3] == 0 and got[4] == 0.0
    v.h.set_rng(st[0], env=0)  # a 5-tuple carries the cache
    same_state(v.h.get_rng_state(0), st[0])
    v.h.set_rng(st[0][:3], env=0)  # a 3-tuple clears it
    assert v.h.get_rng_state(0)[3:] == (0, 0.0)
    v.close()


# ----------------------------------------------------------------------------- 4. refusals
def test_refusals():
    n = 10
    x0 = synthetic_batch(2, n, seed0=800)
    v = noisy(2, n)
    v.reset(x=x0)
    v.controller()
    for call in (lambda: v.expert_steps(4), lambda: v.step(expert=True, controller=True)):
        with pytest.raises(nat.GymFlockError) as e:  # no stream was seeded or set
            call()
        assert e.value.code == nat.GF_ESTATE and "never seeded or set" in str(e.value)
    v.h.set_rng([np.random.RandomState(1), np.random.RandomState(2)])
    with pytest.raises(nat.GymFlockError) as e:
        v.h.dt_steps()  # before any launch
    assert e.value.code == nat.GF_ESTATE
    for bad in ((0.12, -0.018), (0.12, float("nan")), (float("inf"), 0.018)):
        with pytest.raises(nat.GymFlockError) as e:
            v.h.set_dt_noise(*bad)
        assert e.value.code == nat.GF_EINVAL, bad
    with pytest.raises(nat.GymFlockError) as e:
        v.h.step_host(None, False, None, None, None, None)
    assert e.value.code == nat.GF_ESTATE and "fe_set_dt_noise" in str(e.value)
    assert v.expert_steps(4, record=("dt",))["dt"].shape == (4, 2)  # still on, and usable
    # fe_set_dt(NULL) switches the mode off: the fixed-dt rollout of a fresh twin
    v.h.set_dt(None)
    with pytest.raises(nat.GymFlockError) as e:
        v.h.dt_steps()
    assert e.value.code == nat.GF_ESTATE
    with pytest.raises(nat.GymFlockError) as e:
        v.expert_steps(4, record=("dt",))
    assert e.value.code == nat.GF_ESTATE
    v.reset(x=x0)
    v.controller()
    w = VecFlockingRelative(2, n, variant="stochastic")
    w.reset(x=x0)
    w.controller()
    equal_records(v.expert_steps(5, record=frn.RECORDS), w.expert_steps(5, record=frn.RECORDS), keys=frn.RECORDS)
    v.close()
    w.close()
