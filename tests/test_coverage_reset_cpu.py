"""cov_reset_device without a device: the NumPy restatement of its draws
(tests/coverage_reset_numpy.py) against the reference's three recorded resets
(tests/golden/coverage_arl.npz), the loop form of the scalar np_random.choice(n) against
numpy's RandomState, and what the call refuses before it needs a handle."""
import ctypes
import os
import sys

import numpy as np
import pytest

from conftest import GOLDEN, ROOT

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import coverage_reset_numpy as rn  # noqa: E402

NEARBY_DENSITY = 5  # coverage.py: nearby = n_robots * NEARBY_DENSITY

# episode prefix -> (T, R, region size, rounds)
ENV_SEED = {"g_": 6, "r_": 4, "full_": 12}
RECORDED = {"g_": (215, 4, 21, 4), "r_": (255, 4, 20, 4), "full_": (1266, 10, 52, 12)}


@pytest.fixture(scope="module")
def fx():
    return np.load(os.path.join(GOLDEN, "coverage_arl.npz"))


@pytest.mark.parametrize("pre", sorted(RECORDED))
def test_restatement_reproduces_the_recorded_resets(fx, pre):
    T, R, n_region, rounds = RECORDED[pre]
    env_seed = ENV_SEED[pre]
    if pre + "env_seed" in fx.files:  # the full_ run's seed is the recording script's constant
        assert env_seed == int(fx[pre + "env_seed"])
    assert (int(fx[pre + "n_targets"]), int(fx[pre + "n_robots"])) == (T, R)
    s, q = fx[pre + "motion_senders"] - R, fx[pre + "motion_receivers"] - R
    rs = np.random.RandomState(env_seed)
    d = rn.reset_draws(rs, T, R, 0.5, R * NEARBY_DENSITY, s, q)
    assert d["status"] == 0
    assert (int(d["region"].sum()), d["rounds"]) == (n_region, rounds)
    np.testing.assert_array_equal(d["region"], fx[pre + "start_region"])
    targets = fx[pre + "targets"]
    np.testing.assert_array_equal(fx[pre + "x0"][:R], targets[d["start"]])
    np.testing.assert_array_equal(fx[pre + "x0"][R:], targets)
    visited = d["visited"].copy()
    visited[d["start"]] = 1  # the robots visit their start nodes (coverage.py:359)
    np.testing.assert_array_equal(fx[pre + "visited0"][R:], visited)
    np.testing.assert_array_equal(fx[pre + "visited0"][:R], 1)
    # the motion edges the device writes are these: the radius graph of the targets
    res = 5.0
    s2, q2 = rn.radius_edges(targets, res * 1.2)
    np.testing.assert_array_equal(s2, s)
    np.testing.assert_array_equal(q2, q)


def test_scalar_choice_loop_equals_numpy():
    for n in (1, 2, 5, 200, 237, 1000, 5659):
        for seed in range(40):
            rs = np.random.RandomState(seed)
            rs.random_sample(seed * 17 % 623)  # an arbitrary position (two words per sample)
            _, key, pos = rs.get_state()[:3]
            state = [[int(k) for k in key], int(pos)]
            for _ in range(3):
                assert rn.scalar_choice_loop(state, n) == rs.choice(n), (n, seed)
            _, key2, pos2 = rs.get_state()[:3]
            assert state[1] == int(pos2), (n, seed)
            np.testing.assert_array_equal(np.array(state[0], np.uint32), key2)


def test_region_edges_of_the_restatement():
    # a 12-node line: 0 - 1 - ... - 11
    s = np.r_[np.arange(11), np.arange(1, 12)]
    q = np.r_[np.arange(1, 12), np.arange(11)]
    o = np.lexsort((q, s))
    s, q = s[o], q[o]
    region, rounds, short = rn.grow_region(5, 5, 12, s, q)
    assert (np.nonzero(region)[0].tolist(), rounds, short) == ([3, 4, 5, 6, 7], 2, False)
    region, rounds, short = rn.grow_region(11, 5, 12, s, q)  # the line's end: one side only
    assert (np.nonzero(region)[0].tolist(), rounds, short) == ([7, 8, 9, 10, 11], 4, False)
    region, rounds, short = rn.grow_region(5, 4, 12, s, q)   # overshoot: 3 -> 5 nodes
    assert (int(region.sum()), rounds, short) == (5, 2, False)
    region, rounds, short = rn.grow_region(0, 20, 12, s, q)  # the whole line, then nothing to add
    assert (int(region.sum()), short) == (12, True)
    d = rn.reset_draws(np.random.RandomState(0), 2, 3, 0.5, 2, [0, 1], [1, 0])
    assert d["status"] & rn.REGION_SMALL and d["start"] is None


def test_call_validates_before_it_needs_a_handle():
    from gym_flock import _native as nat
    lib = nat.load()
    rc = nat.CovResetConfig(0.5, 0, 0, 0)
    n = ctypes.c_int32(7)
    assert lib.cov_reset_device(None, ctypes.byref(rc), None, None, None, None, None, ctypes.byref(n)) == nat.GF_EINVAL
    assert lib.fe_last_error()
    assert (nat.COV_RESET_SEED, nat.COV_RESET_NEW_MAPS, nat.COV_RESET_DONE) == (1, 2, 4)
    assert (nat.COV_RESET_REGION_SHORT, nat.COV_RESET_REGION_SMALL) == (rn.REGION_SHORT, rn.REGION_SMALL)
    assert ctypes.sizeof(nat.CovResetConfig) == 24  # double, two int32, uint64
    hdr = open(os.path.join(ROOT, "include", "gymflock.h")).read()
    for name in ("COV_RESET_SEED", "COV_RESET_NEW_MAPS", "COV_RESET_DONE", "COV_RESET_REGION_SHORT",
                 "COV_RESET_REGION_SMALL"):
        assert ("#define %s " % name) in hdr and getattr(nat, name) == int(
            hdr.split("#define %s " % name)[1].split()[0], 16)
    assert "GF_ABI_VERSION 1" in " ".join(hdr.split())
