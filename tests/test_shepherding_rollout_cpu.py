"""Shepherding-v0's device reset and recorded rollouts without a GPU: the C-ABI's new symbols
(header, library, binding), the record shapes, and the multi-episode fixture
(tests/golden/shepherding_episodes.npz) against NumPy's own RandomState."""
import ctypes
import os
import sys

import numpy as np

from conftest import GOLDEN

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import shepherding_numpy as sn  # noqa: E402

NEW = ("shep_set_rng", "shep_get_rng", "shep_reset_device", "shep_expert_rollout", "shep_get_episode_steps")


def test_new_symbols_are_declared_exported_and_bound():
    from gym_flock import _native as nat
    from test_capi_cpu import declared_symbols  # the one parser of include/gymflock.h
    lib = nat.load()
    syms = declared_symbols()
    for s in NEW:
        assert s in syms, "%s is not declared in include/gymflock.h" % s
        assert hasattr(lib, s), "%s is not exported" % s
        assert s in nat.SIGNATURES, "binding missing for %s" % s
    assert len(nat.SIGNATURES["shep_expert_rollout"]) == 7 and len(nat.SIGNATURES["shep_reset_device"]) == 5
    for name in ("set_rng", "get_rng", "reset_device", "expert_rollout", "rollout_shapes", "episode_steps"):
        assert callable(getattr(nat.ShepherdHandle, name)), name
    # the structs' layout is the header's: a double and two doubles; six pointers
    assert ctypes.sizeof(nat.ShepResetConfig) == 24 and ctypes.sizeof(nat.ShepRolloutRecords) == 48
    assert [f[0] for f in nat.ShepRolloutRecords._fields_] == ["obs", "adj", "actions", "rewards", "done", "n_resets"]
    assert (nat.SHEP_RESET_SEED, nat.SHEP_RESET_ZERO_HEADINGS, nat.SHEP_REC_DEVICE, nat.SHEP_REC_F32) == (1, 2, 4, 8)
    with open(os.path.join(os.path.dirname(GOLDEN), os.pardir, "include", "gymflock.h")) as f:
        text = f.read()
    for define in ("SHEP_RESET_SEED          0x1", "SHEP_RESET_ZERO_HEADINGS 0x2", "SHEP_REC_DEVICE 0x4",
                   "SHEP_REC_F32    0x8"):
        assert "#define " + define in text, define


def test_null_handles_are_refused_without_a_device():
    from gym_flock import _native as nat
    lib = nat.load()
    rc = nat.ShepResetConfig(1.0, (ctypes.c_double * 2)(0.0, 0.0))
    assert lib.shep_set_rng(None, -1, None, None) == nat.GF_EINVAL
    assert lib.shep_get_rng(None, -1, None, None) == nat.GF_EINVAL
    assert lib.shep_reset_device(None, ctypes.byref(rc), 0, None, 0) == nat.GF_EINVAL
    assert lib.shep_expert_rollout(None, 1, 1, 0, None, None, 0) == nat.GF_EINVAL
    assert lib.shep_get_episode_steps(None, None) == nat.GF_EINVAL
    assert lib.fe_last_error()


def test_rollout_shapes_arithmetic():
    from gym_flock import _native as nat
    s = nat.shep_rollout_shapes(24, 5, 10, 30, every=4)
    assert s["obs"] == ((6, 5, 30, 4), np.float64) and s["adj"] == ((6, 5, 30, 30), np.float64)
    assert s["actions"] == ((24, 5, 10, 2), np.float64)
    assert s["rewards"] == ((24, 5), np.float64) and s["done"] == ((24, 5), np.uint8)
    assert s["n_resets"] == ((5,), np.int32)
    s = nat.shep_rollout_shapes(7, 2, 3, 65, every=1, f32=True)
    assert s["obs"] == ((7, 2, 65, 4), np.float32) and s["adj"] == ((7, 2, 65, 65), np.float32)
    assert s["actions"] == ((7, 2, 3, 2), np.float32) and s["rewards"][1] == np.float64
    assert sorted(s) == sorted(f[0] for f in nat.ShepRolloutRecords._fields_)


def test_drop_in_env_has_the_reset_mode_switch():
    import pytest
    from gym_flock.envs.shepherding.shepherding import ShepherdingEnv
    env = ShepherdingEnv()
    assert env.reset_mode == "reference"
    env.set_reset_mode("device")
    assert env.reset_mode == "device"
    with pytest.raises(ValueError):
        env.set_reset_mode("synthetic")
    env.close()


def test_the_episode_fixture_is_self_consistent():
    """RandomState(s) with NumPy's own uniform / sqrt / cos / sin reproduces the four reset
    states' positions and the final stream bit for bit; each episode's headings start where
    the last ended; the recorder's guards hold at every state."""
    f = np.load(os.path.join(GOLDEN, "shepherding_episodes.npz"))
    ns, n, L = int(f["n_shepherds"]), int(f["n_shepherds"]) + int(f["n_sheep"]), int(f["episode_length"])
    assert (ns, n, L) == (10, 30, 20)
    assert f["x0"].shape == (4, n, 3) and f["x"].shape == (60, n, 3) and f["u"].shape == (60, ns, 2)
    assert f["reward"].shape == (60,) and f["reward0"].shape == (4,) and f["final_key"].shape == (624,)
    assert 0 < float(f["free_run_sensitivity"]) < 1e-11
    r_max, off = float(f["r_max"]), f["goal_offset"]
    assert r_max == np.sqrt(n) and np.array_equal(off, [-3 * r_max, 0.0])
    rs = np.random.RandomState(int(f["seed"]))
    for k in range(4):
        length = np.sqrt(rs.uniform(0, r_max, size=(n,)))
        angle = np.pi * rs.uniform(0, 2, size=(n,))
        x = length * np.cos(angle)
        y = length * np.sin(angle)
        x += off[0]
        y += off[1]
        np.testing.assert_array_equal(f["x0"][k, :, 0], x)
        np.testing.assert_array_equal(f["x0"][k, :, 1], y)
        assert rs.get_state()[2] == f["pos"][k] == 4 * n * (k + 1)
        want = np.zeros(n) if k == 0 else f["x"][k * L - 1, :, 2]
        np.testing.assert_array_equal(f["x0"][k, :, 2], want)
    assert rs.get_state()[2] == f["final_pos"]
    np.testing.assert_array_equal(rs.get_state()[1], f["final_key"])
    # the restatement walks the recorded run bit for bit, and the guards hold
    gr = float(f["goal_region_radius"])
    for e in range(3):
        x = f["x0"][e]
        assert sn.observe(x, ns, goal_radius=gr)[2] == f["reward0"][e]
        for t in range(L):
            k = e * L + t
            ctrl, _, gap = sn.controller(x, ns)
            assert gap >= 1e-9 and sn.pair_gap(x) >= 1e-9 and sn.goal_gap(x, ns, gr) >= 1e-9
            np.testing.assert_array_equal(ctrl, f["u"][k])
            x = sn.step(x, f["u"][k], ns)[0]
            np.testing.assert_array_equal(x, f["x"][k])
            assert sn.observe(x, ns, goal_radius=gr)[2] == f["reward"][k]
