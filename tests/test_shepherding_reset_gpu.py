"""Shepherding-v0's reset on the device (shep_reset_device, gym-flock_amd/csrc/
shepherd_rollout.hip) against NumPy's RandomState. Needs an MI355X.

The uniforms, lengths and angles are NumPy's bits, so the streams (key and position) after a
reset are compared exactly. Positions carry the device's cos / sin and one product, then the
goal offset's addition:

    |x - x_ref| <= 2e-15 * len_ref + 2**-52 * |x_ref|      (the same for y)

The first term is the project's position tolerance (tests/test_flock_reset_gpu.py: twice the
4-ulp bound of double sin / cos, 2 * 4 * 2**-53 = 8.9e-16, rounded up to 2e-15) applied to
the product length * cos(angle) before the offset; the second is the rounding of the offset
addition (half an ulp of the sum on either side). The largest error seen, as a fraction of
that bound, is printed by every check and by the last test.

The observation, adjacency and reward that the reset launch writes contain no trigonometry:
they equal tests/shepherding_numpy.py's of the device's own state bit for bit.
"""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import shepherding_numpy as sn  # noqa: E402

pytestmark = pytest.mark.gpu

nat = pytest.importorskip("gym_flock._native")
from gym_flock.vec import VecShepherding  # noqa: E402

POS_RTOL = 2e-15
# (B, n_shepherds, n_sheep): the wave shape with three empty waves in the last workgroup;
# N = 64, the wave shape's edge; N = 65, a second wave with one lane; 800 words per reset,
# a regeneration inside every reset
SHAPES = [(5, 10, 20), (4, 4, 60), (3, 3, 62), (2, 40, 160)]
SEEN = {"pos_frac": 0.0, "pos_abs": 0.0}


def numpy_reset(rs, n, r_max, goal_offset):
    """(length, x, y) of reset() :193-200 drawn from rs with NumPy's own functions."""
    length = np.sqrt(rs.uniform(0, r_max, size=(n,)))
    angle = np.pi * rs.uniform(0, 2, size=(n,))
    x = length * np.cos(angle)
    y = length * np.sin(angle)
    x += goal_offset[0]
    y += goal_offset[1]
    return length, x, y


def check_positions(got, length, x, y, what):
    for g, w in ((got[:, 0], x), (got[:, 1], y)):
        err = np.abs(g - w)
        bound = POS_RTOL * length + 2.0 ** -52 * np.abs(w)
        SEEN["pos_frac"] = max(SEEN["pos_frac"], float(np.max(err / bound)))
        SEEN["pos_abs"] = max(SEEN["pos_abs"], float(err.max()))
        assert np.all(err <= bound), "%s: error %.3e over the bound %.3e" % (what, err.max(), bound[np.argmax(err / bound)])
    print("%s: largest position error so far %.3e, %.3f of the bound" % (what, SEEN["pos_abs"], SEEN["pos_frac"]))


def check_stream(v, b, rs, what):
    key, pos = v.h.get_rng(b)
    st = rs.get_state()
    assert pos == st[2], "%s: env %d position %d, NumPy's %d" % (what, b, pos, st[2])
    np.testing.assert_array_equal(key, st[1], err_msg="%s: env %d key" % (what, b))


def check_outputs(v, what):
    """obs, adj and reward equal the restatement's of the device's own state bit for bit."""
    x, obs, adj, rew = v.get_state(), v.obs(), v.adj(), v.rewards()
    for b in range(v.n_envs):
        o, a, r = sn.observe(x[b], v.n_shepherds, goal_radius=v.goal_region_radius)
        np.testing.assert_array_equal(obs[b], o, err_msg=what)
        np.testing.assert_array_equal(adj[b], a, err_msg=what)
        assert rew[b] == r, what
    return x


def check_reset(v, x, streams, what, envs=None):
    """State x of a reset that drew from `streams` (advanced here), and the streams after."""
    for b in (range(v.n_envs) if envs is None else envs):
        length, xr, yr = numpy_reset(streams[b], v.n_agents, v.r_max, v.goal_offset)
        check_positions(x[b], length, xr, yr, "%s env %d" % (what, b))
        check_stream(v, b, streams[b], what)


@pytest.mark.parametrize("B,ns,nsheep", SHAPES)
def test_seeded_reset_of_all_envs(B, ns, nsheep):
    seed = 1000 + ns
    v = VecShepherding(B, ns, nsheep)
    x = v.reset_device(seed=seed)
    streams = [np.random.RandomState(seed + b) for b in range(B)]
    check_reset(v, x, streams, "seeded N=%d" % (ns + nsheep))
    np.testing.assert_array_equal(x[..., 2], 0.0)
    check_outputs(v, "seeded N=%d" % (ns + nsheep))
    np.testing.assert_array_equal(v.h.episode_steps(), 0)
    # a second, continued reset: the streams go on (for N = 200 across another regeneration)
    x = v.reset_device()
    check_reset(v, x, streams, "continued N=%d" % (ns + nsheep))
    check_outputs(v, "continued N=%d" % (ns + nsheep))
    v.close()


def test_seven_consecutive_resets_cross_a_regeneration():
    """120 words per reset from position 624: 624 -> 120 -> 240 -> ... -> 600 -> 96, the
    sixth reset crosses the regeneration."""
    B = 5
    v = VecShepherding(B)
    streams = [np.random.RandomState(77 + b) for b in range(B)]
    positions = []
    for k in range(7):
        x = v.reset_device(seed=77 if k == 0 else None)
        check_reset(v, x, streams, "reset %d" % k)
        positions.append(v.h.get_rng(0)[1])
    assert positions == [120, 240, 360, 480, 600, 96, 216]
    check_outputs(v, "seventh reset")
    v.close()


@pytest.mark.parametrize("B,ns,nsheep", SHAPES)
def test_streams_set_at_an_odd_position_and_at_624(B, ns, nsheep):
    """Env 0: a stream that drew 310 doubles and then 4 bytes stands at 621, odd: the
    second double of the reset takes its first word from the old key and its second from
    the regenerated one. Env 1: position 624 exactly. The others: a fresh RandomState
    (also 624) and one in mid-key."""
    streams = []
    for b in range(B):
        rs = np.random.RandomState(500 + b)
        if b == 0:
            rs.random_sample(310)
            rs.bytes(4)
            assert rs.get_state()[2] == 621
        elif b == 1:
            rs.random_sample(312)
            assert rs.get_state()[2] == 624
        elif b == 3:
            rs.random_sample(100)
        streams.append(rs)
    v = VecShepherding(B, ns, nsheep)
    v.h.set_rng(streams)
    for b in range(B):
        check_stream(v, b, streams[b], "set_rng")
    x = v.reset_device()
    check_reset(v, x, streams, "odd / 624 N=%d" % (ns + nsheep))
    check_outputs(v, "odd / 624")
    v.h.set_rng(streams[0], env=B - 1)  # one env's stream
    check_stream(v, B - 1, streams[0], "set_rng of one env")
    v.close()


def _random_state(B, n, seed):
    rs = np.random.RandomState(seed)
    x = np.empty((B, n, 3))
    x[..., :2] = rs.uniform(-3, 3, size=(B, n, 2))
    x[..., 2] = rs.uniform(-np.pi, np.pi, size=(B, n))
    return x


def _snapshot(v):
    keys, pos = v.h.get_rng()
    return dict(x=v.get_state(), obs=v.obs(), adj=v.adj(), rew=v.rewards(), keys=keys, pos=pos,
                count=v.h.episode_steps())


@pytest.mark.parametrize("B,ns,nsheep,envs", [(5, 10, 20, [1, 4]), (3, 3, 62, [2]), (6, 10, 20, [0, 1, 2, 3])])
def test_masked_reset_leaves_the_other_envs_alone(B, ns, nsheep, envs):
    n = ns + nsheep
    v = VecShepherding(B, ns, nsheep)
    v.reset_device(seed=5)
    v.set_state(_random_state(B, n, 6))
    v.step(expert=True)
    v.step(expert=True)
    before = _snapshot(v)
    np.testing.assert_array_equal(before["count"], 2)
    streams = [v.np_random(b) for b in range(B)]
    # a mask of none changes nothing
    v.reset_device(envs=np.zeros(B, bool), fetch=False)
    v.reset_device(envs=[], fetch=False)
    after = _snapshot(v)
    for k in before:
        np.testing.assert_array_equal(after[k], before[k], err_msg="empty mask: " + k)
    x = v.reset_device(envs=envs)
    after = _snapshot(v)
    others = [b for b in range(B) if b not in envs]
    for k in before:
        np.testing.assert_array_equal(after[k][others], before[k][others], err_msg="unselected: " + k)
    np.testing.assert_array_equal(after["count"][envs], 0)
    check_reset(v, x, streams, "masked", envs)
    np.testing.assert_array_equal(x[envs][..., 2], before["x"][envs][..., 2])  # headings kept
    check_outputs(v, "masked")
    mask = np.zeros(B, bool)
    mask[envs] = True
    x = v.reset_device(envs=mask)  # the same selection as a mask
    check_reset(v, x, streams, "masked (bool)", envs)
    np.testing.assert_array_equal(x[others], before["x"][others])
    v.close()


@pytest.mark.parametrize("B,ns,nsheep", [(5, 10, 20), (3, 3, 62)])
def test_headings_are_kept_zeroed_or_zero(B, ns, nsheep):
    n = ns + nsheep
    v = VecShepherding(B, ns, nsheep)
    x = v.reset_device(seed=1)  # a handle with no state: as from the all-zero state
    np.testing.assert_array_equal(x[..., 2], 0.0)
    x0 = _random_state(B, n, 9)
    v.set_state(x0)
    x = v.reset_device()
    np.testing.assert_array_equal(x[..., 2], x0[..., 2])
    assert np.all(x[..., :2] != x0[..., :2])
    np.testing.assert_array_equal(v.obs()[..., 2], x0[..., 2])
    x = v.reset_device(headings="zero")
    np.testing.assert_array_equal(x[..., 2], 0.0)
    check_outputs(v, "zeroed headings")
    v.set_state(x0)
    x = v.reset_device(envs=[0], headings="zero")
    np.testing.assert_array_equal(x[0, :, 2], 0.0)
    np.testing.assert_array_equal(x[1:], x0[1:])
    v.close()
    # a masked reset of a handle with no state: the others are the all-zero state, observed
    v = VecShepherding(B, ns, nsheep)
    x = v.reset_device(seed=3, envs=[1])
    np.testing.assert_array_equal(x[[0, 2]], 0.0)
    assert np.all(x[1, :, :2] != 0.0)
    check_outputs(v, "masked reset without a state")
    v.close()


def test_refusals_leave_the_handle_usable():
    import ctypes
    B = 3
    v = VecShepherding(B)
    h = v.h

    def refused(code, call):
        with pytest.raises(nat.GymFlockError) as e:
            call()
        assert e.value.code == code, str(e.value)

    off = v.goal_offset
    refused(nat.GF_ESTATE, lambda: h.reset_device(v.r_max, off))                    # never seeded or set
    refused(nat.GF_ESTATE, lambda: h.get_rng(0))
    refused(nat.GF_EINVAL, lambda: h.reset_device(v.r_max, off, seed=1, flags=0x10))  # unknown flag
    for bad in (0.0, -1.0, np.inf, np.nan):
        refused(nat.GF_EINVAL, lambda: h.reset_device(bad, off, seed=1))
    refused(nat.GF_EINVAL, lambda: h.reset_device(v.r_max, off, seed=2 ** 32 - 2))  # seed + 3 > 2**32
    refused(nat.GF_EINVAL, lambda: h.reset_device(v.r_max, off, seed=2 ** 40))
    lib = nat.load()
    rc = nat.ShepResetConfig(1.0, (ctypes.c_double * 2)(0.0, 0.0))
    assert lib.shep_reset_device(None, ctypes.byref(rc), 0, None, nat.SHEP_RESET_SEED) == nat.GF_EINVAL
    assert lib.shep_reset_device(h.h, None, 0, None, nat.SHEP_RESET_SEED) == nat.GF_EINVAL
    keys, pos = np.zeros((1, 624), np.uint32), np.array([625], np.int32)
    assert lib.shep_set_rng(h.h, 0, nat.ptr(keys), nat.ptr(pos)) == nat.GF_EINVAL
    assert lib.shep_set_rng(h.h, B, nat.ptr(keys), nat.ptr(pos)) == nat.GF_EINVAL
    # a continued reset of env 1 alone needs only env 1's stream
    h.set_rng(np.random.RandomState(4), env=1)
    refused(nat.GF_ESTATE, lambda: h.reset_device(v.r_max, off, envs=[0, 1]))
    h.reset_device(v.r_max, off, envs=[1])
    refused(nat.GF_ESTATE, lambda: h.get_rng())
    refused(nat.GF_ESTATE, v.controls)  # a reset leaves no controls
    # the largest seed that fits, then the handle works as ever
    x = v.reset_device(seed=2 ** 32 - 3)
    streams = [np.random.RandomState(2 ** 32 - 3 + b) for b in range(B)]
    check_reset(v, x, streams, "largest seed")
    v.step(expert=True)
    np.testing.assert_array_equal(h.episode_steps(), 1)
    check_outputs(v, "after the refusals")
    v.close()


def test_drop_in_env_resets_on_the_device():
    import gym_flock
    ref = gym_flock.make("Shepherding-v0")
    env = gym_flock.make("Shepherding-v0", reset_mode="device")
    assert ref.reset_mode == "reference" and env.reset_mode == "device"
    with pytest.raises(ValueError):
        env.set_reset_mode("host")
    for e in (ref, env):
        e.seed(21)
    obs_r, adj_r = ref.reset()
    obs, adj = env.reset()
    st_r, st = ref.np_random.get_state(), env.np_random.get_state()
    assert st[2] == st_r[2] == 120
    np.testing.assert_array_equal(st[1], st_r[1])
    rs = np.random.RandomState(21)
    length, x, y = numpy_reset(rs, 30, env.r_max, env.goal_offset)
    np.testing.assert_array_equal(ref.x[:, 0], x)  # "reference" mode is untouched: NumPy's bits
    np.testing.assert_array_equal(ref.x[:, 1], y)
    np.testing.assert_array_equal(obs_r[:, :3], ref.x)
    check_positions(env.x, length, x, y, "drop-in")
    np.testing.assert_array_equal(obs[:, :3], env.x)
    np.testing.assert_array_equal(obs[:, 3:], env.agent_identities)
    np.testing.assert_array_equal(adj, sn.observe(env.x, 10)[1])
    assert obs.shape == (30, 4) and adj.shape == (30, 30)
    # headings are carried over a second reset, and np_random stays in step with the reference's
    u = np.random.RandomState(3).uniform(-2, 2, size=(10, 2)).astype(np.float32)
    for e in (ref, env):
        for _ in range(3):
            e.step(u)
    th = env.x[:, 2].copy()
    assert np.all(th != 0.0)
    ref.reset()
    env.reset()
    np.testing.assert_array_equal(env.x[:, 2], th)
    length, x, y = numpy_reset(rs, 30, env.r_max, env.goal_offset)
    check_positions(env.x, length, x, y, "drop-in, second reset")
    np.testing.assert_array_equal(env.np_random.get_state()[1], ref.np_random.get_state()[1])
    assert env.np_random.get_state()[2] == ref.np_random.get_state()[2] == 240
    # a draw by the caller between resets goes up with the next one
    for e in (ref, env):
        e.np_random.uniform(size=7)
    ref.reset()
    env.reset()
    rs.uniform(size=7)
    length, x, y = numpy_reset(rs, 30, env.r_max, env.goal_offset)
    check_positions(env.x, length, x, y, "drop-in, after the caller's draws")
    np.testing.assert_array_equal(ref.x[:, 0], x)
    assert env.np_random.get_state()[2] == ref.np_random.get_state()[2] == rs.get_state()[2]
    env.set_reset_mode("reference")  # back to host draws: NumPy's bits again
    env.reset()
    length, x, y = numpy_reset(rs, 30, env.r_max, env.goal_offset)
    np.testing.assert_array_equal(env.x[:, 0], x)
    np.testing.assert_array_equal(env.x[:, 1], y)
    ref.close()
    env.close()


def test_zz_report_the_largest_position_error_seen():
    print("largest position error %.3e, %.3f of the bound 2e-15 * length + 2**-52 * |x|"
          % (SEEN["pos_abs"], SEEN["pos_frac"]))
