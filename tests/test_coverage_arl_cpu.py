"""CPU checks of CoverageARL-v0 / CoverageFull-v0: the stated arithmetic of the target pool
and the subgraph sampler (a NumPy restatement, coverage_arl_numpy.py) reproduces the
reference's fixture bit for bit; the new entry points validate their arguments before any
device work; the env ids are registered; the env says where it looked for its map."""
import ctypes
import os
import sys

import numpy as np
import pytest

from conftest import GOLDEN

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import coverage_arl_numpy as an  # noqa: E402

MOTION_RADIUS = 0.5 * 10 * 1.2  # CoverageARLEnv: res = MAP_RES * downsample_rate, radius res * 1.2


@pytest.fixture(scope="module")
def fx():
    return np.load(os.path.join(GOLDEN, "coverage_arl.npz"))


@pytest.fixture(scope="module")
def grid():
    return np.load(os.path.join(GOLDEN, "grid_slice10.npy"))


def _maps(f, key_len, key_idx):
    return np.split(f[key_idx].astype(np.int64), np.cumsum(f[key_len])[:-1])


def test_pool_restatement_matches_the_fixture(fx, grid):
    raw, pool, lo, hi, sub = an.load_graph(grid, MOTION_RADIUS)
    assert raw.shape == (1714, 2) and pool.shape == (1266, 2)
    np.testing.assert_array_equal(raw, fx["pool_raw"])
    np.testing.assert_array_equal(pool, fx["all_targets"])
    np.testing.assert_array_equal(lo, fx["min_xy"])
    np.testing.assert_array_equal(hi, fx["max_xy"])
    np.testing.assert_array_equal(sub, fx["subgraph_size"])


def test_sampler_restatement_matches_every_map_and_try_count(fx):
    pool, lo, hi, sub = fx["all_targets"], fx["min_xy"], fx["max_xy"], fx["subgraph_size"]
    maps, nxt = _maps(fx, "map_len", "map_idx"), _maps(fx, "next_len", "next_idx")
    assert fx["tries"][0] == 13 and fx["tries"][5] == 1 and fx["tries"][38] == 21
    for s in range(40):
        np.random.seed(s)
        idx, tries = an.sample_submap(pool, lo, hi, sub, MOTION_RADIUS)
        assert tries == fx["tries"][s], s
        np.testing.assert_array_equal(idx, maps[s], err_msg="seed %d" % s)
        assert 200 <= len(idx) <= 274
        if s < 10:
            state = np.random.get_state()
            idx2, tries2 = an.sample_submap(pool, lo, hi, sub, MOTION_RADIUS)
            assert tries2 == fx["next_tries"][s], s
            np.testing.assert_array_equal(idx2, nxt[s], err_msg="second map of seed %d" % s)
            np.random.set_state(state)
        assert np.random.uniform() == fx["probe"][s], s


def test_sampler_restatement_is_bounded_by_max_tries(fx):
    pool, lo, hi, sub = fx["all_targets"], fx["min_xy"], fx["max_xy"], fx["subgraph_size"]
    idx, tries = an.sample_submap(pool, lo, hi, sub, MOTION_RADIUS, np.random.RandomState(0), max_tries=2)
    assert idx is None and tries == 2  # seed 0 needs 13


def test_component_tie_goes_to_the_lowest_root():
    # two components of two points each: the first one wins (argmax(bincount)'s first label)
    pts = np.array([[0.0, 0.0], [50.0, 0.0], [5.0, 0.0], [55.0, 0.0], [100.0, 0.0]])
    np.testing.assert_array_equal(an.largest_component(pts, 6.0), [True, False, True, False, False])


def test_new_entry_points_reject_bad_arguments_without_a_device(grid):
    from gym_flock import _native as nat
    lib = nat.load()
    cfg = nat.occupancy_config()
    g = np.ascontiguousarray(grid, dtype=np.uint8)
    n = ctypes.c_int32(0)
    assert lib.cov_load_occupancy(None, ctypes.byref(cfg), nat.ptr(g), g.shape[0], g.shape[1], ctypes.byref(n)) == nat.GF_EINVAL
    assert lib.fe_last_error()
    assert lib.cov_get_pool(None, None, None, None, None) == nat.GF_EINVAL
    assert lib.cov_generate_submaps(None, -1, 0, None, 0, nat.COV_MAP_SEED, None, None, None) == nat.GF_EINVAL
    d = np.zeros((1, 4, 2))
    assert lib.cov_generate_submaps(None, 0, 0, nat.ptr(d), 4, nat.COV_MAP_DRAWS, None, None, None) == nat.GF_EINVAL
    # the configuration struct's layout is the header's
    assert ctypes.sizeof(nat.CovOccupancyConfig) == 56
    assert (cfg.downsample_rate, cfg.perimeter_delta, cfg.check_connected, cfg.num_subgraphs, cfg.min_targets,
            cfg.max_tries) == (10, 2.0, 1, 3.0, 200, 4096)
    assert tuple(cfg.xyz_min) == (-321.0539855957031, -276.5395050048828)


def test_env_ids_hold_the_arl_envs():
    import gym_flock
    for env_id, cls in (("CoverageARL-v0", "CoverageARLEnv"), ("CoverageARL-v1", "CoverageARLEnv"),
                        ("CoverageFull-v0", "CoverageFullEnv")):
        assert gym_flock.ENV_IDS[env_id] == ("gym_flock.envs.spatial:" + cls, 100000)
    from gym_flock.envs import spatial
    assert spatial.CoverageARLEnv.__name__ == "CoverageARLEnv" and issubclass(spatial.CoverageFullEnv, spatial.CoverageARLEnv)


def test_env_without_a_grid_says_where_it_looked(tmp_path, monkeypatch):
    import gym_flock
    monkeypatch.setenv("GYM_FLOCK_MAPS", str(tmp_path))
    with pytest.raises(FileNotFoundError) as e:
        gym_flock.make("CoverageARL-v0")
    assert "grid_slice10.npy" in str(e.value) and str(tmp_path) in str(e.value) and "occupancy=" in str(e.value)
    monkeypatch.delenv("GYM_FLOCK_MAPS")
    with pytest.raises(FileNotFoundError):
        gym_flock.make("CoverageFull-v0")
