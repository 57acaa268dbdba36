"""The recorded expert rollout across episode ends without a GPU: the NumPy restatement of the
loop (tests/coverage_rollout_numpy.py) against the reference's recorded multi-episode runs on
one map (tests/golden/coverage_expert_rollout.npz), and cov_expert_rollout's host arithmetic, bindings
and the refusals that need no device."""
import os
import sys
import types

import numpy as np
import pytest

from conftest import GOLDEN

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import coverage_reset_numpy as rn  # noqa: E402
import coverage_rollout_numpy as cr  # noqa: E402


def _recorded_env(f, pre):
    """The recorded run's env in the restatement, before its first reset."""
    R, M = int(f[pre + "n_robots"]), int(f[pre + "max_nodes"])
    env = cr.CoverageRollout(f[pre + "targets"], R, M, res=float(f[pre + "res"]),
                             episode_length=int(f[pre + "episode_length"]), frac_active=float(f[pre + "frac_active"]),
                             nearby=int(f[pre + "nearby"]))
    np.testing.assert_array_equal(env.o.motion[0], f[pre + "motion_senders"])
    np.testing.assert_array_equal(env.o.motion[1], f[pre + "motion_receivers"])
    return env


@pytest.mark.parametrize("pre", ["a_", "b_"])
def test_restatement_reproduces_the_recorded_episodes(pre):
    """CoverageARLEnv on one kept map (res 5.0, 4 robots, nearby starts of 20 nodes): reset(),
    four greedy episodes, reset() after each. The first reset's draws from RandomState(env_seed)
    are the recorded ones; then one rollout with resets on done reproduces every step's actions,
    reward and done flag, run a's flat rows (the reset rows after the done steps), the four
    in-run resets' regions, starts and visited sets, and the stream after each."""
    f = np.load(os.path.join(GOLDEN, "coverage_expert_rollout.npz"))
    env = _recorded_env(f, pre)
    R, T = env.R, env.T
    assert (T, R, env.M) == ((215, 4, 1000) if pre == "a_" else (255, 4, 1000))
    rs = np.random.RandomState(int(f[pre + "env_seed"]))
    d = rn.reset_draws(rs, T, R, env.frac_active, env.nearby, env.s, env.q)
    np.testing.assert_array_equal(d["region"], f[pre + "region"][0])
    np.testing.assert_array_equal(d["start"], f[pre + "start"][0])
    st = rs.get_state()
    np.testing.assert_array_equal(st[1], f[pre + "rng_key"][0])
    assert st[2] == f[pre + "rng_pos"][0]
    env.reset(d["start"], d["visited"], rs)
    np.testing.assert_array_equal(env.visited(), f[pre + "visited"][0])
    if pre == "a_":
        np.testing.assert_array_equal(env.flat_row(), f["a_row0"])
    n = len(f[pre + "reward"])
    out = cr.rollout([env], n, auto_reset=True)
    np.testing.assert_array_equal(out["actions"][:, 0], f[pre + "actions"])
    np.testing.assert_array_equal(out["rewards"][:, 0], f[pre + "reward"])
    np.testing.assert_array_equal(out["done"][:, 0], f[pre + "done"])
    if pre == "a_":
        np.testing.assert_array_equal(out["flat_obs"][:, 0], f["a_row"])
    per = int(f[pre + "episode_length"]) - 1  # reset()'s own observation counts one step
    assert np.nonzero(out["done"][:, 0])[0].tolist() == [per * k - 1 for k in range(1, 5)]
    assert out["n_resets"][0] == 4 and out["reset_status"][0] == 0 and len(out["resets"][0]) == 4
    for k, r in enumerate(out["resets"][0], start=1):
        np.testing.assert_array_equal(r["region"], f[pre + "region"][k])
        np.testing.assert_array_equal(r["start"], f[pre + "start"][k])
        np.testing.assert_array_equal(r["visited_after"], f[pre + "visited"][k])
        np.testing.assert_array_equal(r["rng_after"][1], f[pre + "rng_key"][k])
        assert r["rng_after"][2] == f[pre + "rng_pos"][k]
        assert 20 <= r["region"].sum() <= 25
    # the stream after the last step (before the trailing reset) and at the end
    last = out["resets"][0][-1]["rng_before"]
    np.testing.assert_array_equal(last[1], f[pre + "rng_key_end"])
    assert last[2] == f[pre + "rng_pos_end"]
    st = env.rng.get_state()
    np.testing.assert_array_equal(st[1], f[pre + "rng_key"][4])
    assert st[2] == f[pre + "rng_pos"][4]
    # a key regeneration falls inside the recorded in-run draws
    assert any(r["regenerated"] for r in out["resets"][0])


def test_restatement_without_resets_steps_on_past_done_and_strides_rows():
    f = np.load(os.path.join(GOLDEN, "coverage_expert_rollout.npz"))

    def run(every, n=15):
        env = _recorded_env(f, "a_")
        rs = np.random.RandomState()
        rs.set_state(("MT19937", f["a_rng_key"][0], int(f["a_rng_pos"][0])))
        env.reset(f["a_start"][0], f["a_visited"][0], rs)
        return cr.rollout([env], n, every)

    a, b = run(1), run(5)
    np.testing.assert_array_equal(a["actions"][:11, 0], f["a_actions"][:11])
    np.testing.assert_array_equal(a["flat_obs"][:10, 0], f["a_row"][:10])
    assert a["done"][:, 0].tolist() == [False] * 10 + [True] + [False] * 4 and "n_resets" not in a
    np.testing.assert_array_equal(a["flat_obs"][:, 0, -1], np.arange(1, 16))  # the step feature counts on
    assert b["flat_obs"].shape == (3, 1, 15 * 1000 + 1)
    np.testing.assert_array_equal(b["flat_obs"], a["flat_obs"][[4, 9, 14]])


def _step_lds(R, M):
    """cov_step_lds_bytes: three robot arrays, claim and seen bits, four counters, the first
    claimers, the visited bits per 64 targets, the direct candidates and their count, the key,
    the fallback robots' bits."""
    return 3 * R * 4 + 2 * ((M + 31) // 32) * 4 + 16 + M * 4 + ((M - R + 63) // 64) * 8 + 33 * 4 + 624 * 4 + \
        ((R + 63) // 64) * 8


def _draw_lds(T):
    """cov_reset_draw_lds_bytes: key, perm, vseq, two bit sets, flags."""
    return 624 * 4 + 8 * T + 16 * ((T + 63) // 64) + T


@pytest.mark.parametrize("R,M", [(4, 1000), (3, 37), (1, 66), (70, 170), (624, 1648)])
def test_lds_bytes_is_host_arithmetic(R, M):
    from gym_flock import _native as nat
    lib = nat.load()
    assert lib.cov_rollout_lds_bytes(R, M, 0) == _step_lds(R, M)
    assert lib.cov_rollout_lds_bytes(R, M, 1) == ((_step_lds(R, M) + 15) & ~15) + _draw_lds(M - R)
    assert lib.cov_rollout_lds_bytes(R, M, 1) <= 64 * 1024  # every shape the greedy lists allow fits


def test_lds_bytes_refuses_nonsense_and_passes_64k_only_beyond_the_lists():
    from gym_flock import _native as nat
    lib = nat.load()
    assert lib.cov_rollout_lds_bytes(0, 10, 1) == -1 and lib.cov_rollout_lds_bytes(4, 3, 0) == -1
    m = 1000
    while lib.cov_rollout_lds_bytes(2, m, 1) <= 64 * 1024:
        m += 1
    assert m - 2 > 1024  # the greedy lists' bound refuses such a handle first


def test_rollout_shapes_for_both_kinds_of_handle():
    from gym_flock import _native as nat
    sh = nat.cov_rollout_shapes(12, 3, 4, 37, every=3, hidden=False)
    assert sh == {"rewards": ((12, 3), np.float64), "done": ((12, 3), np.uint8),
                  "actions": ((12, 3, 4), np.int32), "needs_random": ((12, 3, 4), np.uint8),
                  "flat_obs": ((4, 3, 15 * 37 + 1), np.float32)}
    assert nat.cov_rollout_shapes(12, 3, 4, 37, every=3)["flat_obs"][0] == (4, 3, 16 * 37 + 1)
    for feat, width in ((3, 15), (4, 16)):
        h = types.SimpleNamespace(n_envs=2, n_robots=1, max_nodes=10, n_node_feat=feat)
        assert nat.CoverageHandle.rollout_shapes(h, 5)["flat_obs"][0] == (5, 2, width * 10 + 1)


def test_expert_rollout_validates_before_touching_the_device():
    from gym_flock import _native as nat
    lib = nat.load()
    assert "cov_expert_rollout" in nat.SIGNATURES and "cov_rollout_lds_bytes" in nat.SIGNATURES
    assert lib.cov_expert_rollout(None, 1, None, None) == nat.GF_EINVAL
    rec, ar = nat.CovRollout(), nat.CovAutoReset(0.5, 0, 0, None, None)
    rec.record_every = 1
    assert lib.cov_expert_rollout(None, 1, rec, ar) == nat.GF_EINVAL
    assert lib.fe_last_error()
    # the header's struct: a double, two int32, two pointers
    assert nat.CovAutoReset.nearby.offset == 8 and nat.CovAutoReset.flags.offset == 12
    assert nat.CovAutoReset.n_resets.offset == 16 and nat.CovAutoReset.status.offset == 24
    assert nat.ctypes.sizeof(nat.CovAutoReset) == 32


def test_vec_coverage_refuses_without_a_device_call():
    """VecCoverage.expert_rollout's own refusals come before any library call."""
    from gym_flock.vec import VecCoverage
    v = VecCoverage.__new__(VecCoverage)
    v.hide_nodes = True
    with pytest.raises(RuntimeError, match="hide"):
        v.expert_rollout(2)
    v.hide_nodes, v._dev_streams, v._rngs, v.n_robots = False, False, None, 4
    with pytest.raises(RuntimeError, match="streams"):
        v.expert_rollout(2)
