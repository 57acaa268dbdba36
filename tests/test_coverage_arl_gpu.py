"""CoverageARL-v0 / CoverageFull-v0 on the GPU against the reference's fixture
(tests/golden/coverage_arl.npz, made by tests/golden/make_golden_coverage_arl.py from
tests/golden/grid_slice10.npy): the occupancy pool, the batched and the drop-in subgraph
sampler, whole episodes of both envs, and a batched expert episode against the CPU oracle."""
import os
import sys

import numpy as np
import pytest

from conftest import GOLDEN

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import coverage_arl_numpy as an  # noqa: E402

pytestmark = pytest.mark.gpu

OBS_KEYS = ("nodes", "edges", "senders", "receivers", "step")


@pytest.fixture(scope="module")
def fx():
    return np.load(os.path.join(GOLDEN, "coverage_arl.npz"))


@pytest.fixture(scope="module")
def grid():
    return np.load(os.path.join(GOLDEN, "grid_slice10.npy"))


def _maps(f, key_len, key_idx):
    return np.split(f[key_idx].astype(np.int64), np.cumsum(f[key_len])[:-1])


def _arl_handle():
    from gym_flock import _native as nat
    return nat.CoverageHandle(4, 1, 1000, 50, 5.0)


def test_load_occupancy_gives_the_reference_pool(fx, grid):
    from gym_flock import _native as nat
    h = _arl_handle()
    assert h.load_occupancy(grid) == 1266
    pool, lo, hi, sub = h.pool()
    np.testing.assert_array_equal(pool, fx["all_targets"])
    np.testing.assert_array_equal(lo, fx["min_xy"])
    np.testing.assert_array_equal(hi, fx["max_xy"])
    np.testing.assert_array_equal(sub, fx["subgraph_size"])
    # without the component step: from_occupancy's 1714 targets
    assert h.load_occupancy(grid, nat.occupancy_config(check_connected=False)) == 1714
    np.testing.assert_array_equal(h.pool()[0], fx["pool_raw"])
    h.close()


def test_pool_component_tie_goes_to_the_first_component():
    """6 x 5 grid, its middle column occupied, perimeter_delta 1: the kept cells are the two
    columns beside it, two components of 6 points each. argmax(bincount(labels)) takes the
    first label, i.e. the component holding the lowest point (column 1)."""
    from gym_flock import _native as nat
    g = np.zeros((6, 5), bool)
    g[:, 2] = True
    raw, pool, lo, hi, sub = an.load_graph(g, 6.0, perimeter_delta=1.0)
    assert len(raw) == 12 and len(pool) == 6
    np.testing.assert_array_equal(pool, raw[:6])
    h = _arl_handle()
    assert h.load_occupancy(g, nat.occupancy_config(perimeter_delta=1.0)) == 6
    got, glo, ghi, gsub = h.pool()
    np.testing.assert_array_equal(got, pool)
    np.testing.assert_array_equal(glo, lo)
    np.testing.assert_array_equal(ghi, hi)
    np.testing.assert_array_equal(gsub, sub)
    # without the component step every kept cell is in the pool
    assert h.load_occupancy(g, nat.occupancy_config(perimeter_delta=1.0, check_connected=False)) == 12
    np.testing.assert_array_equal(h.pool()[0], raw)
    h.close()


def test_grid_without_an_occupied_cell_is_refused(grid):
    from gym_flock import _native as nat
    h = _arl_handle()
    with pytest.raises(nat.GymFlockError) as e:
        h.load_occupancy(np.zeros((6, 5), bool))
    assert e.value.code == nat.GF_EINVAL
    with pytest.raises(nat.GymFlockError) as e:  # no pool yet
        h.generate_submaps(map_seed=0)
    assert e.value.code == nat.GF_ESTATE
    big = np.zeros((128, 128), bool)  # every third column occupied: ~10,900 candidate cells
    big[:, ::3] = True
    with pytest.raises(nat.GymFlockError) as e:
        h.load_occupancy(big)
    assert e.value.code == nat.GF_EINVAL and "more than the pool holds" in str(e.value)
    assert h.load_occupancy(grid) == 1266  # the handle is still usable
    with pytest.raises(nat.GymFlockError) as e:
        h.generate_submaps(draws=np.zeros((1, 0, 2)))
    assert e.value.code == nat.GF_EINVAL
    h.close()


def test_batched_submaps_match_the_reference_seeds(fx, grid):
    from gym_flock import _native as nat
    from gym_flock.vec import VecCoverage
    B = 8
    pool = fx["all_targets"]
    maps, nxt = _maps(fx, "map_len", "map_idx"), _maps(fx, "next_len", "next_idx")
    v = VecCoverage(B, 4, max_nodes=1000, episode_length=50, res=5.0)
    assert v.load_occupancy(grid) == 1266
    n, st, tries = v.generate_submaps(map_seed=0)
    np.testing.assert_array_equal(tries, fx["tries"][:B])
    np.testing.assert_array_equal(st, 0)
    for b in range(B):
        assert n[b] == len(maps[b])
        np.testing.assert_array_equal(v.targets(b), pool[maps[b]], err_msg="env %d" % b)
    n, st, tries = v.generate_submaps()  # the streams continue
    np.testing.assert_array_equal(tries, fx["next_tries"][:B])
    for b in range(B):
        np.testing.assert_array_equal(v.targets(b), pool[nxt[b]], err_msg="second map of env %d" % b)
    # a bounded retry loop: seed 0 needs 13 tries, seed 5 one
    v.load_occupancy(grid, max_tries=2)
    with pytest.raises(nat.GymFlockError) as e:
        v.generate_submaps(map_seed=0)
    assert e.value.code == nat.GF_EINVAL
    assert e.value.status[0] & nat.COV_MAP_NO_WINDOW and e.value.tries[0] == 2
    assert e.value.status[5] == 0 and e.value.tries[5] == 1 and e.value.n_targets[5] == len(maps[5])
    v.load_occupancy(grid)  # still usable
    n, st, tries = v.generate_submaps(map_seed=0)
    np.testing.assert_array_equal(tries, fx["tries"][:B])
    np.testing.assert_array_equal(v.targets(0), pool[maps[0]])
    v.close()


@pytest.fixture(scope="module")
def arl_env(grid):
    import gym_flock
    env = gym_flock.make("CoverageARL-v0", occupancy=grid)
    yield env
    env.close()


@pytest.mark.parametrize("s", [0, 5, 38])
def test_dropin_generate_targets_follows_the_global_stream(fx, arl_env, s):
    """Seed 5 takes 1 try, seed 0 13 and seed 38 21 (more than the 16 drawn per launch)."""
    maps = _maps(fx, "map_len", "map_idx")
    np.testing.assert_array_equal(arl_env.all_targets, fx["all_targets"])
    np.testing.assert_array_equal(arl_env.subgraph_size, fx["subgraph_size"])
    np.random.seed(s)
    targets, changed = arl_env._generate_targets()
    assert changed
    np.testing.assert_array_equal(targets, fx["all_targets"][maps[s]])
    assert np.random.uniform() == fx["probe"][s]


def _replay(env, obs, f, pre, policies):
    R = int(f[pre + "n_robots"])
    assert env.n_targets == int(f[pre + "n_targets"]) and env.max_nodes == int(f[pre + "max_nodes"])
    np.testing.assert_array_equal(env.x[R:], f[pre + "targets"])
    np.testing.assert_array_equal(np.array(env.start_region), f[pre + "start_region"])
    np.testing.assert_array_equal(env.x, f[pre + "x0"])
    for k in OBS_KEYS:
        np.testing.assert_array_equal(np.asarray(obs[k]).reshape(f[pre + k + "0"].shape), f[pre + k + "0"], err_msg=k)
    for t, policy in enumerate(policies):
        if policy == "greedy":
            a = env.controller(random=False, greedy=True)
            np.testing.assert_array_equal(a.flatten(), f[pre + "actions"][t], err_msg="greedy actions, step %d" % t)
        else:
            a = f[pre + "actions"][t].reshape(-1, 1)
        obs, r, d, _ = env.step(a)
        assert r == f[pre + "reward"][t] and d == f[pre + "done"][t], (t, r, d)
        for k in OBS_KEYS:
            np.testing.assert_array_equal(np.asarray(obs[k]).reshape(f[pre + k][t].shape), f[pre + k][t],
                                          err_msg="%s, step %d" % (k, t))
        np.testing.assert_array_equal(env.closest_targets, f[pre + "closest"][t])
    np.testing.assert_array_equal(env.visited[:, 0], f[pre + "visited"][-1])


@pytest.mark.parametrize("pre,policy", [("g_", "greedy"), ("r_", "random")])
def test_arl_episode_replays_the_reference(fx, grid, pre, policy):
    from gym_flock.envs.spatial import CoverageARLEnv
    map_seed, env_seed = int(fx[pre + "map_seed"]), int(fx[pre + "env_seed"])
    np.random.seed(map_seed)
    env = CoverageARLEnv(occupancy=grid)
    env.seed(env_seed)
    np.random.seed(map_seed)
    obs = env.reset()
    _replay(env, obs, fx, pre, [policy] * 50)
    if pre == "r_":  # update_state (coverage_arl.py:42-44) on this episode's final env
        env.update_state(fx["us_state"])
        np.testing.assert_array_equal(env.x[:env.n_robots], fx["us_x"])
        np.testing.assert_array_equal(env.x[env.closest_targets], fx["us_x"])
    env.close()


def test_coverage_full_run_replays_the_reference(fx, grid):
    import gym_flock
    np.random.seed(11)
    env = gym_flock.make("CoverageFull-v0", occupancy=grid)
    assert (env.n_targets, env.max_nodes, env.n_motion_edges) == (1266, 1276, 3552)
    env.seed(12)
    obs = env.reset()
    assert obs["nodes"].shape == (1276, 3) and obs["edges"].shape == (5104, 1)
    _replay(env, obs, fx, "full_", ["random"] * 12 + ["greedy"] * 8)
    env.close()


@pytest.mark.parametrize("greedy", [False, True])
def test_driver_loop_runs_to_done(arl_env, greedy):
    """The reference driver's episode loop (test.py:43-74) with its random and greedy policies."""
    np.random.seed(3)
    arl_env.seed(4)
    arl_env.reset()
    done, steps, total = False, 0, 0.0
    while not done:
        action = arl_env.controller(random=False, greedy=True) if greedy else arl_env.controller(random=True)
        obs, reward, done, _ = arl_env.step(action)
        total += reward
        steps += 1
        assert steps <= 50
    assert total == arl_env.episode_reward and (total > 0 or not greedy)


def test_batched_expert_episode_matches_the_oracle(fx, grid, monkeypatch):
    """VecCoverage.reset(seed, new_maps=True, map_seed=0) on the occupancy pool, then 50
    fused greedy steps at B=4: every env replayed on the CPU oracle from the fixture's
    maps (the oracle's edge scale and episode length set to CoverageARL-v0's)."""
    from gym_flock.vec import VecCoverage
    from oracle import coverage as oc
    monkeypatch.setattr(oc, "RES", 5.0)
    monkeypatch.setattr(oc, "EPISODE_LENGTH", 50)
    B, R, M = 4, 4, 1000
    pool, maps = fx["all_targets"], _maps(fx, "map_len", "map_idx")
    v = VecCoverage(B, R, max_nodes=M, episode_length=50, res=5.0)
    v.load_occupancy(grid)
    start, visited = v.reset(seed=11, new_maps=True, map_seed=0)
    orcs, mats, rngs = [], [], []
    for b in range(B):
        tg = pool[maps[b]]
        T = len(tg)
        assert v.n_targets[b] == T
        np.testing.assert_array_equal(v.targets(b), tg)
        rs = np.random.RandomState(11 + b)
        st = rs.choice(np.arange(T), size=(R,), replace=False)
        drop = rs.choice(np.arange(T) + R, size=(int(T * 0.5),), replace=False)
        np.testing.assert_array_equal(start[b], st)
        o = oc.CoverageOracle(tg, R, M, motion_radius=5.0 * 1.2)
        ref = o.reset(st, drop)
        got = v.obs(b)
        for key in ("nodes", "edges", "senders", "receivers"):
            np.testing.assert_array_equal(got[key].reshape(ref[key].shape), ref[key], err_msg="reset b=%d %s" % (b, key))
        orcs.append(o)
        mats.append(oc.time_matrix(T, o.motion[0] - R, o.motion[1] - R, horizon=10))
        rngs.append(rs)
    for t in range(50):
        v.step(greedy=True)
        r, d = v.rewards()
        for b in range(B):
            o = orcs[b]
            cur = o.closest()
            recv = oc.action_receivers(cur, o.nbr, o.cnt, R)
            a, rnd = oc.greedy_actions(mats[b][0], mats[b][1], cur, o.visited[R:], recv, R)
            for i in np.nonzero(rnd)[0]:
                a[i] = rngs[b].choice(4)
            ref, rr, dd = o.step(a)
            assert r[b] == rr and d[b] == dd, (t, b)
            got = v.obs(b)
            for key in ("nodes", "edges", "senders", "receivers"):
                np.testing.assert_array_equal(got[key].reshape(ref[key].shape), ref[key], err_msg="t=%d b=%d %s" % (t, b, key))
    v.close()
