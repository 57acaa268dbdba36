"""The hidden-node expert rollout without a GPU: the NumPy restatement of the loop
(tests/coverage_explore_rollout_numpy.py) against the reference's recorded greedy ExploreEnv
episode, and cov_explore_expert's argument validation and bindings."""
import os
import sys

import numpy as np

from conftest import GOLDEN

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import coverage_explore_rollout_numpy as xr  # noqa: E402
import coverage_reset_numpy as rn  # noqa: E402


def test_restatement_reproduces_the_recorded_greedy_episode():
    """ExploreEnv-v0's recorded episode (prefix g_): res 5.0, horizon 19, 50 steps at most,
    nearby starts. The env's stream is RandomState(env_seed) after the reset's draws, which are
    checked against the recorded start; then every step's actions (fallback draws included),
    reward, done, discovered set and robot nodes, and the stream's next uniform()."""
    f = np.load(os.path.join(GOLDEN, "coverage_explore.npz"))
    R, T, M = int(f["g_n_robots"]), int(f["g_n_targets"]), int(f["g_max_nodes"])
    targets = f["g_targets"]
    env = xr.ExploreRollout(targets, R, M, motion_radius=5.0 * 1.2, horizon=19, episode_length=50)
    rs = np.random.RandomState(int(f["g_env_seed"]))
    s, q = env.o.motion[0] - R, env.o.motion[1] - R
    d = rn.reset_draws(rs, T, R, 0.5, R * 5, s, q)
    np.testing.assert_array_equal(d["region"], f["g_start_region"])
    np.testing.assert_array_equal(targets[d["start"]], f["g_x0"][:R])
    obs = env.reset(d["start"], d["visited"], rs)
    np.testing.assert_array_equal(env.o.visited, f["g_visited0"])
    np.testing.assert_array_equal(env.disc, f["g_discovered0"])
    np.testing.assert_array_equal(obs["nodes"], f["g_nodes0"])
    np.testing.assert_array_equal(obs["senders"], f["g_senders0"])
    n = len(f["g_reward"])
    out = xr.rollout([env], n)
    np.testing.assert_array_equal(out["actions"][:, 0], f["g_actions"])
    np.testing.assert_array_equal(out["rewards"][:, 0], f["g_reward"])
    np.testing.assert_array_equal(out["done"][:, 0], f["g_done"])
    np.testing.assert_array_equal(out["closest"][:, 0], f["g_closest"])
    np.testing.assert_array_equal(env.disc, f["g_discovered"][-1])
    np.testing.assert_array_equal(env.o.visited, f["g_visited"][-1])
    np.testing.assert_array_equal(env.obs["nodes"], f["g_nodes"][-1])
    np.testing.assert_array_equal(env.obs["senders"], f["g_senders"][-1])
    assert out["needs_random"].sum() == 14 and out["done"][-1, 0] and n < 50  # the episode's 14 draws
    assert rs.uniform() == f["g_probe"]


def test_restatement_records_rows_at_the_stride():
    f = np.load(os.path.join(GOLDEN, "coverage_explore.npz"))
    R, T, M = int(f["g_n_robots"]), int(f["g_n_targets"]), int(f["g_max_nodes"])

    def run(every):
        env = xr.ExploreRollout(f["g_targets"], R, M, motion_radius=6.0, horizon=19, episode_length=50)
        rs = np.random.RandomState(int(f["g_env_seed"]))
        d = rn.reset_draws(rs, T, R, 0.5, R * 5, env.o.motion[0] - R, env.o.motion[1] - R)
        env.reset(d["start"], d["visited"], rs)
        return xr.rollout([env], 6, every)

    a, b = run(1), run(3)
    assert a["flat_obs"].shape == (6, 1, 16 * M + 1) and b["flat_obs"].shape == (2, 1, 16 * M + 1)
    np.testing.assert_array_equal(b["flat_obs"], a["flat_obs"][[2, 5]])
    np.testing.assert_array_equal(a["flat_obs"][:, 0, -1], np.arange(1, 7))  # the step feature


def test_explore_expert_validates_before_touching_the_device():
    from gym_flock import _native as nat
    lib = nat.load()
    assert "cov_explore_expert" in nat.SIGNATURES and "cov_explore_lds_bytes" in nat.SIGNATURES
    assert lib.cov_explore_expert(None, 1, None) == nat.GF_EINVAL
    rec = nat.CovRollout()
    rec.record_every = 1
    assert lib.cov_explore_expert(None, 1, rec) == nat.GF_EINVAL
    assert lib.fe_last_error()
    # the header's struct: five pointers, then two int32
    assert nat.CovRollout.flat_obs.offset == 32 and nat.CovRollout.record_every.offset == 40
    assert nat.CovRollout.flags.offset == 44 and nat.COV_ROLLOUT_DEVICE == 1


def test_rollout_shapes():
    from gym_flock import _native as nat
    sh = nat.cov_rollout_shapes(12, 3, 4, 37, every=3)
    assert sh == {"rewards": ((12, 3), np.float64), "done": ((12, 3), np.uint8),
                  "actions": ((12, 3, 4), np.int32), "needs_random": ((12, 3, 4), np.uint8),
                  "flat_obs": ((4, 3, 16 * 37 + 1), np.float32)}
    assert nat.cov_rollout_shapes(5, 2, 1, 10)["flat_obs"][0] == (5, 2, 161)


def test_lds_bytes_is_host_arithmetic():
    """The LDS a workgroup takes grows with the map (16 bytes per target for the staged
    positions, 4 per node for the claims); the ExploreEnv shape is far below the 64 KB guard,
    and the smallest max_nodes past it is what the GPU test of the guard uses."""
    from gym_flock import _native as nat
    lib = nat.load()
    small = lib.cov_explore_lds_bytes(4, 1000)
    assert 16 * 996 + 4 * 1000 < small < 32 * 1024
    assert lib.cov_explore_lds_bytes(4, 1001) > small
    assert lib.cov_explore_lds_bytes(0, 10) == -1 and lib.cov_explore_lds_bytes(4, 3) == -1
    m = 1000
    while lib.cov_explore_lds_bytes(2, m) <= 64 * 1024:
        m += 1
    assert lib.cov_explore_lds_bytes(2, m - 1) <= 64 * 1024 < lib.cov_explore_lds_bytes(2, m) and 2500 < m < 4000
