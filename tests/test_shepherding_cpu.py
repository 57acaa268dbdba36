"""Shepherding-v0 without a GPU: the NumPy restatement (tests/shepherding_numpy.py) against
the reference's recorded episodes (tests/golden/shepherding_ep*.npz), the :253 quirk of
the shepherd controller, the package's registration of the env and the shep_* C-ABI."""
import ctypes
import inspect
import os
import sys

import numpy as np
import pytest

from conftest import GOLDEN

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import shepherding_numpy as sn  # noqa: E402


@pytest.fixture(scope="module", params=[0, 1])
def ep(request):
    return np.load(os.path.join(GOLDEN, "shepherding_ep%d.npz" % request.param))


def test_recorded_episodes_are_the_ones_the_issue_names(ep):
    ns, n = int(ep["n_shepherds"]), int(ep["n_shepherds"]) + int(ep["n_sheep"])
    assert (ns, n) == (10, 30)
    assert ep["x"].shape == (61, n, 3) and ep["u"].shape == (60, ns, 2) and ep["controller"].shape == (61, ns, 2)
    assert ep["reward"].shape == (60,) and ep["adj"].shape == (7, n, n)
    assert ep["u"].dtype == (np.float64 if str(ep["policy"]) == "controller" else np.float32)
    if str(ep["policy"]) == "controller":
        np.testing.assert_array_equal(ep["u"], ep["controller"][:60])
    assert 0 < float(ep["free_run_sensitivity"]) < 1e-11


def test_restatement_reproduces_the_recorded_episodes_bit_for_bit(ep):
    """Teacher-forced from every recorded state: next state, reward, adjacency, controller."""
    ns = int(ep["n_shepherds"])
    adj_at = {int(t): k for k, t in enumerate(ep["adj_steps"])}
    gap = np.inf
    for t in range(61):
        x = ep["x"][t]
        out, rows, g = sn.controller(x, ns)
        gap = min(gap, g)
        np.testing.assert_array_equal(out, ep["controller"][t], err_msg="controller, state %d" % t)
        np.testing.assert_array_equal(sn.rows_of(out, x[:ns, 2]), rows)
        obs, adj, rew = sn.observe(x, ns, float(ep["comm_radius"]), float(ep["goal_region_radius"]))
        assert rew == (ep["reward"][t - 1] if t else ep["reward0"])
        np.testing.assert_array_equal(obs[:, :3], x)
        np.testing.assert_array_equal(obs[:, 3], [1.0] * ns + [0.0] * (len(x) - ns))
        if t in adj_at:
            np.testing.assert_array_equal(adj, ep["adj"][adj_at[t]], err_msg="adjacency, state %d" % t)
        if t < 60:
            new, _ = sn.step(x, ep["u"][t], ns, float(ep["dt"]), float(ep["action_scalar"]))
            np.testing.assert_array_equal(new, ep["x"][t + 1], err_msg="state %d" % (t + 1))
        assert sn.pair_gap(x) >= 1e-9 and sn.goal_gap(x, ns) >= 1e-9
    assert gap >= 1e-9  # the recorder's guards hold for the stored episodes


def test_float32_and_float64_actions_multiply_differently():
    """u * 5.0 stays float32 for float32 actions (:89); the restatement follows NumPy."""
    x = np.load(os.path.join(GOLDEN, "shepherding_ep1.npz"))["x"][3]
    u32 = np.full((10, 2), 0.1, np.float32)
    a = sn.step(x, u32, 10)[1][:10]
    b = sn.step(x, u32.astype(np.float64), 10)[1][:10]
    assert np.all(a == (u32 * np.float32(5.0)).astype(np.float64)) and np.all(a != b)


def test_shepherd_branch_needs_an_exactly_zero_component():
    """:253 `s.all() == shepherd.all()` skips a shepherd whenever both states, or neither,
    have a zero component. A generic state never tests a shepherd; one shepherd at theta ==
    0.0 exactly makes the branch reachable. Pinned, not fixed."""
    # shepherd 0 at the origin side looks along +x at shepherd 1; the sheep are behind it
    x = np.array([[-5.0, 0.25, 0.5], [-3.0, 0.25, 0.7], [-9.0, 3.0, 0.3], [-9.0, -3.0, 0.2]])
    x[0, 2] = 1e-300  # generic: no zero anywhere, shepherd 1 dead ahead but never tested
    rows = sn.controller(x, 2)[1]
    assert rows[0] == 2  # the goal (the origin) is within 5 degrees: third row
    x[0, 2] = 0.0        # shepherd 0 now has a zero component, shepherd 1 has none
    out, rows, _ = sn.controller(x, 2)
    assert rows[0] == 1  # shepherd in line of sight: second row
    np.testing.assert_array_equal(out[0], [(0.6098 + 0.5471) / 2, (0.6098 - 0.5471) / 0.6 * 0.3])
    assert rows[1] != 1  # shepherd 1 tests shepherd 0 too (unequal .all()), which is behind it
    x[1, 2] = 0.0        # both have a zero component: skipped again
    assert sn.controller(x, 2)[1][0] == 2
    for k in (0, 1):     # every recorded state after the reset is generic: branch never taken
        f = np.load(os.path.join(GOLDEN, "shepherding_ep%d.npz" % k))
        assert not any(1 in sn.controller(f["x"][t], 10)[1] for t in range(1, 61, 6))


def test_wrap_to_pi_returns_zero_for_an_exactly_zero_angle():
    s = np.array([0.0, 0.0, 0.0])
    assert sn.los_angle(s, np.array([1.0, 0.0]), np.cos, np.sin, np.arctan2) == 0.0
    assert sn.los_angle(s, np.array([-1.0, 0.0]), np.cos, np.sin, np.arctan2) == np.pi


def test_shepherding_id_module_path_and_signature():
    import gym_flock
    from gym_flock.envs import shepherding
    from gym_flock.envs.shepherding.shepherding import ShepherdingEnv
    assert gym_flock.ENV_IDS["Shepherding-v0"] == ("gym_flock.envs.shepherding:ShepherdingEnv", 1000)
    assert shepherding.ShepherdingEnv is ShepherdingEnv
    params = inspect.signature(ShepherdingEnv.__init__).parameters
    assert list(params) == ["self", "device"] and params["device"].default == 0
    env = gym_flock.make("Shepherding-v0")  # no device work before the first reset / step
    assert (env.n_sheep, env.n_shepherds, env.n_agents, env.nx, env.nu) == (20, 10, 30, 3, 2)
    assert (env.dt, env.v_max, env.comm_radius, env.action_scalar) == (0.01, 2.0, 2.0, 5.0)
    assert env.r_max == np.sqrt(30) and env.goal_region_radius == 0.5 * np.sqrt(30)
    np.testing.assert_array_equal(env.goal_offset, [-3 * np.sqrt(30), 0])
    assert env.x.shape == (30, 3) and env.agent_identities.shape == (30, 1) and env.agent_identities.sum() == 10
    assert env.action_space.shape == (10, 2) and env.observation_space.shape == (30, 3)
    assert env.seed(4) == [4] and env.np_random.uniform() == np.random.RandomState(4).uniform()
    with pytest.raises(AssertionError):
        env.step(np.zeros((30, 2)))
    for name in ("seed", "step", "reset", "controller", "render", "close"):
        assert callable(getattr(env, name))
    env.close()


def test_vec_reset_draws_the_recorded_initial_state():
    """The host draw of reset() (lengths first, then angles) is the reference's bit for bit."""
    from gym_flock.init_states import draw_shepherding
    for k in (0, 1):
        f = np.load(os.path.join(GOLDEN, "shepherding_ep%d.npz" % k))
        r_max = np.sqrt(30)
        xy = draw_shepherding(30, r_max, np.array([-r_max * 3, 0]), np.random.RandomState(int(f["seed"])))
        np.testing.assert_array_equal(xy, f["x"][0][:, :2])
        assert np.all(f["x"][0][:, 2] == 0)


def test_every_declared_shep_symbol_is_exported_and_bound():
    from gym_flock import _native as nat
    from test_capi_cpu import declared_symbols  # the one parser of include/gymflock.h
    lib = nat.load()
    syms = [s for s in declared_symbols() if s.startswith("shep_")]
    for s in ("shep_create", "shep_destroy", "shep_set_state", "shep_get_state", "shep_observe", "shep_step",
              "shep_controller", "shep_step_expert", "shep_get_obs", "shep_get_adj", "shep_get_rewards", "shep_sync"):
        assert s in syms
    for s in syms:
        assert hasattr(lib, s), s
        assert s in nat.SIGNATURES, "binding missing for %s" % s
    assert lib.fe_abi_version() == 1


def test_shep_create_validates_arguments_before_touching_the_device():
    from gym_flock import _native as nat
    lib = nat.load()
    h = ctypes.c_void_p()
    good = dict(n_shepherds=10, n_sheep=20, n_envs=1, dt=0.01, comm_radius=2.0, action_scalar=5.0,
                force_weight_shepherd=0.45, force_weight_sheep=0.075, goal_region_radius=2.7, device=0)
    bad = [dict(n_shepherds=0), dict(n_sheep=0), dict(n_shepherds=1000, n_sheep=25), dict(n_envs=0), dict(dt=0.0),
           dict(dt=-0.01), dict(comm_radius=0.0), dict(goal_region_radius=-1.0)]
    for kw in bad:
        cfg = nat.ShepConfig(**dict(good, **kw))
        assert lib.shep_create(ctypes.byref(cfg), ctypes.byref(h)) == nat.GF_EINVAL, kw
        assert lib.fe_last_error() and h.value is None
    cfg = nat.ShepConfig(**good)
    assert lib.shep_create(None, ctypes.byref(h)) == nat.GF_EINVAL
    assert lib.shep_create(ctypes.byref(cfg), None) == nat.GF_EINVAL
    for fn, args in ((lib.shep_step, (None, None, 0)), (lib.shep_observe, (None,)), (lib.shep_set_state, (None, None)),
                     (lib.shep_get_obs, (None, None, 0)), (lib.shep_step_expert, (None, 1, None)),
                     (lib.shep_controller, (None, None)), (lib.shep_sync, (None,))):
        assert fn(*args) == nat.GF_EINVAL


def test_shepherd_handle_without_a_device_fails_loudly():
    """Without a GPU the product raises GF_EHIP; there is no CPU fallback."""
    from gym_flock import _native as nat
    try:
        h = nat.ShepherdHandle(10, 20, 1)
    except nat.GymFlockError as e:
        assert e.code == nat.GF_EHIP
        return
    h.close()
