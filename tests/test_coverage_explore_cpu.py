"""ExploreEnv without a GPU: the NumPy restatement of the hidden-node observation
(tests/coverage_explore_numpy.py) against the reference's recorded episodes
(tests/golden/coverage_explore.npz), and the package's registration of the env."""
import inspect
import os
import sys

import numpy as np
import pytest

from conftest import GOLDEN

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import coverage_explore_numpy as en  # noqa: E402
from oracle import coverage as oc  # noqa: E402


@pytest.fixture(scope="module")
def fx():
    return np.load(os.path.join(GOLDEN, "coverage_explore.npz"))


def _oracle(f, pre):
    """The unhidden env of a recorded episode (oracle.coverage) at its reset."""
    R, M = int(f[pre + "n_robots"]), int(f[pre + "max_nodes"])
    targets = f[pre + "targets"]
    o = oc.CoverageOracle(targets, R, M, motion_radius=5.0 * 1.2)
    start = oc.closest_targets(f[pre + "x0"][:R], targets, R) - R
    obs = o.reset(start, np.nonzero(f[pre + "visited0"] == 0)[0])
    np.testing.assert_array_equal(o.xr, f[pre + "x0"][:R])
    return o, obs


def test_recorded_episodes_are_the_ones_the_issue_names(fx):
    assert (int(fx["g_n_targets"]), len(fx["g_reward"]), fx["g_reward"].sum()) == (215, 49, 62)
    assert (int(fx["r_n_targets"]), len(fx["r_reward"]), fx["r_reward"].sum()) == (255, 49, 20)
    assert fx["g_done"][-1] and fx["r_done"][-1] and not fx["g_done"][:-1].any() and not fx["r_done"][:-1].any()


@pytest.mark.parametrize("pre", ["g_", "r_"])
def test_restatement_reproduces_every_recorded_hidden_observation(fx, pre):
    f = fx
    R, M = int(f[pre + "n_robots"]), int(f[pre + "max_nodes"])
    o, obs = _oracle(f, pre)
    np.testing.assert_array_equal(obs["senders"], f[pre + "stored_senders0"])
    disc = en.initial_discovered(M, R)  # reset() sets it before its observation (:419-421)
    d, nodes, snd = en.hidden_obs(disc, obs["nodes"], obs["senders"], obs["receivers"], o.xr, o.targets)
    assert nodes.dtype == np.float64 and nodes.shape == (M, 4)
    np.testing.assert_array_equal(nodes, f[pre + "nodes0"])
    np.testing.assert_array_equal(snd, f[pre + "senders0"])
    np.testing.assert_array_equal(d, f[pre + "discovered0"])
    np.testing.assert_array_equal(obs["receivers"], f[pre + "receivers0"])
    hidden_edges = frontier = 0
    for t in range(len(f[pre + "reward"])):
        obs, rew, done = o.step(f[pre + "actions"][t])
        np.testing.assert_array_equal(o.xr, f[pre + "xr"][t])
        assert rew == f[pre + "reward"][t]
        d, nodes, snd = en.hidden_obs(d, obs["nodes"], obs["senders"], obs["receivers"], o.xr, o.targets)
        np.testing.assert_array_equal(nodes, f[pre + "nodes"][t], err_msg="nodes, step %d" % t)
        np.testing.assert_array_equal(snd, f[pre + "senders"][t], err_msg="senders, step %d" % t)
        np.testing.assert_array_equal(d, f[pre + "discovered"][t], err_msg="discovered, step %d" % t)
        np.testing.assert_array_equal(obs["receivers"], f[pre + "receivers"][t])
        hidden_edges += int(np.sum(snd != obs["senders"]))
        frontier += int(nodes[:, 3].sum())
    assert hidden_edges > 0 and frontier > 0  # the episodes do hide edges and flag frontier nodes


def test_restatement_reproduces_the_recorded_masked_expert(fx):
    """Every action of the greedy episode that the expert chose itself; the robots it hands to
    np_random.choice are the recording's 14 fallback draws."""
    f, pre = fx, "g_"
    R, M, T = int(f[pre + "n_robots"]), int(f[pre + "max_nodes"]), int(f[pre + "n_targets"])
    o, obs = _oracle(f, pre)
    cost, prev = oc.time_matrix(T, o.motion[0] - R, o.motion[1] - R, horizon=19)
    d = en.hidden_obs(en.initial_discovered(M, R), obs["nodes"], obs["senders"], obs["receivers"], o.xr, o.targets)[0]
    n_rand = 0
    for t in range(len(f[pre + "reward"])):
        cur = o.closest()
        recv = oc.action_receivers(cur, o.nbr, o.cnt, R)
        acts, rand = en.masked_greedy_actions(cost, prev, cur, o.visited[R:], d[R:R + T], recv, R)
        np.testing.assert_array_equal(acts[~rand], f[pre + "actions"][t][~rand], err_msg="step %d" % t)
        n_rand += int(rand.sum())
        obs = o.step(f[pre + "actions"][t])[0]
        d = en.hidden_obs(d, obs["nodes"], obs["senders"], obs["receivers"], o.xr, o.targets)[0]
    assert n_rand == 14


def test_own_node_and_radius_rules_of_the_restatement():
    """A robot does not see the node it stands on (r = 0); r == 22 is seen, the next double is not."""
    xr = np.array([[0.0, 0.0]])
    far = np.nextafter(22.0, np.inf)
    targets = np.array([[0.0, 0.0], [22.0, 0.0], [far, 0.0], [0.0, -22.0]])
    np.testing.assert_array_equal(en.seen_nodes(xr, targets), [False, True, False, True])


def test_explore_ids_and_signature(monkeypatch):
    import gym_flock
    from gym_flock.envs import spatial
    for env_id in ("ExploreEnv-v0", "ExploreEnv-v1"):
        assert gym_flock.ENV_IDS[env_id] == ("gym_flock.envs.spatial:ExploreEnv", 100000)
    assert "ExploreFullEnv-v0" not in gym_flock.ENV_IDS and not hasattr(spatial, "ExploreFullEnv")
    assert issubclass(spatial.ExploreEnv, spatial.CoverageARLEnv)
    params = inspect.signature(spatial.ExploreEnv.__init__).parameters
    assert list(params) == ["self", "occupancy", "device"]  # the reference's takes none beyond self
    assert params["occupancy"].default is None and params["device"].default == 0
    seen = {}
    monkeypatch.setattr(spatial.CoverageARLEnv, "__init__", lambda self, **kw: seen.update(kw))
    spatial.ExploreEnv(occupancy="grid", device=3)
    assert seen == dict(hide_nodes=True, n_node_feat=4, horizon=19, episode_length=50, occupancy="grid", device=3)
