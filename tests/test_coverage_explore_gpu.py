"""ExploreEnv-v0 / -v1 and cov_set_hidden on the GPU: the hidden-node observation of tiny
handles against the NumPy restatement (tests/coverage_explore_numpy.py) applied to the
handle's own unhidden observation, and the drop-in env against the reference's recorded
episodes (tests/golden/coverage_explore.npz). Every comparison is exact: all values are
flags, indices or counts."""
import os
import sys

import numpy as np
import pytest

from conftest import GOLDEN

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import coverage_explore_numpy as en  # noqa: E402
from oracle import coverage as oc  # noqa: E402

pytestmark = pytest.mark.gpu

OBS_KEYS = ("nodes", "edges", "senders", "receivers", "step")


@pytest.fixture(scope="module")
def nat():
    from gym_flock import _native
    return _native


@pytest.fixture(scope="module")
def grid():
    return np.load(os.path.join(GOLDEN, "grid_slice10.npy"))


def _line(n=12, spacing=5.0):
    return np.stack([np.arange(n) * spacing, np.zeros(n)], axis=1)


def _line_handle(nat, max_nodes, start=1, n=12):
    """One env, res 5.0 (motion radius 6.0), n targets 5.0 apart on a line, one robot on
    target `start`, every target unvisited."""
    h = nat.CoverageHandle(1, 1, max_nodes, 50, 5.0)
    h.set_hidden(True)
    h.set_targets(_line(n), env=0)
    h.reset(np.array([[start]], np.int32), np.zeros((1, max_nodes - 1), np.uint8))
    return h


def _check_env(h, b, disc, targets, msg=""):
    """Env b's hidden observation equals the restatement applied to its unhidden one and to
    the discovered set `disc` from before this observation. Returns the set after it."""
    o = h.obs(b)
    xr, _ = h.robots(b)
    d, nodes, snd = en.hidden_obs(disc, o["nodes"], o["senders"], o["receivers"], xr, targets)
    got = h.hidden_obs(b)
    assert got["nodes"].dtype == np.float64 and got["nodes"].shape == (h.max_nodes, 4)
    np.testing.assert_array_equal(got["nodes"], nodes, err_msg="nodes " + msg)
    np.testing.assert_array_equal(got["senders"], snd, err_msg="senders " + msg)
    np.testing.assert_array_equal(h.discovered(b), d, err_msg="discovered " + msg)
    for k in ("edges", "receivers", "step"):  # never hidden
        np.testing.assert_array_equal(got[k], o[k], err_msg=k + " " + msg)
    return d


def _walk_line(h, max_nodes, start=1, n=12):
    R, targets = 1, _line(n)
    d = _check_env(h, 0, en.initial_discovered(max_nodes, R), targets, "reset")
    for t in range(6):  # a node of degree 2 offers (left, right, itself, itself)
        h.step(np.array([[1]]))
        assert h.robots(0)[1][0] == R + start + 1 + t
        d = _check_env(h, 0, d, targets, "step %d" % t)
    return d


def test_line_graph_own_node_frontier_and_four_hops(nat):
    M = 16
    h = _line_handle(nat, M)
    d = h.discovered(0)
    # robot, target 0 (5.0 away), NOT its own target 1 (r = 0), targets 2..5 (up to 20.0), not 6 (25.0)
    np.testing.assert_array_equal(d, [1, 1, 0, 1, 1, 1, 1] + [0] * 9)
    o = h.hidden_obs(0)
    # the robot's row: robot flag, and the frontier flag from the two padding loops to its
    # undiscovered node among its action targets
    np.testing.assert_array_equal(o["nodes"][0], [1, 0, 0, 1])
    np.testing.assert_array_equal(o["nodes"][2], [0, 0, 0, 0])  # its own node: masked
    np.testing.assert_array_equal(o["nodes"][1], [0, 1, 1, 1])  # target 0: next to the undiscovered node
    np.testing.assert_array_equal(o["nodes"][6], [0, 1, 1, 1])  # target 5: the frontier towards target 6
    d = _walk_line(h, M)
    np.testing.assert_array_equal(d, [1] * 13 + [0] * 3)  # from target 7 everything has been seen
    h.close()


def test_wrapped_minus_one_lands_on_a_real_node(nat):
    """n_agents == max_nodes: the unused slots' -1 indexes the last target."""
    M = 13
    h = _line_handle(nat, M)
    o = h.obs(0)
    assert (o["senders"] == -1).any() and h.n_motion()[0] + 8 < 4 * M
    d = _walk_line(h, M)
    assert d[M - 1] == 1  # target 11 was discovered: the unused slots now index a discovered node
    assert (h.hidden_obs(0)["senders"][h.n_motion()[0]:4 * M - 8] == -1).all()
    h.close()


@pytest.mark.parametrize("max_nodes", [400, 1100])
def test_long_line_discovers_targets_past_the_first_item(nat, max_nodes):
    """300 targets, the robot around target 280: the nodes that change belong to a thread's
    second round of the pass's loops, and with max_nodes = 1100 the loops take five rounds."""
    h = _line_handle(nat, max_nodes, start=278, n=300)
    d = _walk_line(h, max_nodes, start=278, n=300)
    assert d[1 + 274:1 + 289].all() and not d[1 + 289:].any() and not d[1:1 + 274].any()  # targets 274..288
    h.close()


def test_radius_boundary(nat):
    far = np.nextafter(22.0, np.inf)
    targets = np.array([[0.0, 0.0],        # robot 0 stands here: r = 0, not seen
                        [22.0, 0.0],       # r == 22.0: seen
                        [0.0, far],        # one ulp farther: not seen
                        [1000.0, 0.0],     # robot 1 stands here
                        [13.2, 17.6],      # 22 up to rounding: whatever sqrt(dx*dx + dy*dy) says
                        [1000.0 - 22.0, 0.0],   # r == 22.0 from robot 1
                        [-1000.0, 0.0], [-1000.0, 500.0]])  # the reset's starts, out of everyone's sight
    R, M = 2, 12
    h = nat.CoverageHandle(R, 1, M, 75, 5.5)
    h.set_hidden(True)
    h.set_targets(targets, env=0)
    h.reset(np.array([[6, 7]], np.int32), np.zeros((1, M - R), np.uint8))
    d = _check_env(h, 0, en.initial_discovered(M, R), targets, "reset")
    np.testing.assert_array_equal(d, [1, 1] + [0] * 10)  # nothing in sight, own nodes unseen
    h.set_robot_positions(0, targets[[0, 3]])
    np.testing.assert_array_equal(h.discovered(0), d)  # placing robots discovers nothing by itself
    h.step(np.zeros((1, R)))  # isolated nodes: every action stays
    np.testing.assert_array_equal(h.robots(0)[1], [R + 0, R + 3])
    d = _check_env(h, 0, d, targets, "placed")
    exp = en.seen_nodes(targets[[0, 3]], targets)
    assert list(exp[[0, 1, 2, 3, 5]]) == [False, True, False, False, True]
    np.testing.assert_array_equal(d[R:R + len(targets)], exp)
    h.close()


# ------------------------------------------------------------------ the batch of three maps
def _maps():
    s = 5.5
    gx, gy = np.meshgrid(np.arange(4) * s, np.arange(5) * s, indexing="ij")
    grid_map = np.stack([gx.ravel(), gy.ravel()], axis=1)  # 20: target ix * 5 + iy
    n_ring, n_chord = 26, 8
    r = s / (2.0 * np.sin(np.pi / n_ring))
    ang = 2.0 * np.pi * np.arange(n_ring) / n_ring
    ring = np.stack([r * np.cos(ang), r * np.sin(ang)], axis=1)
    chord = np.stack([np.linspace(r, -r, n_chord + 2)[1:-1], np.zeros(n_chord)], axis=1)
    ring_map = np.vstack([ring, chord])  # 34 = max_nodes - n_robots
    bx, by = np.meshgrid(np.arange(3) * s, np.arange(3) * s, indexing="ij")
    blob = np.stack([bx.ravel(), by.ravel()], axis=1)
    bridge = np.stack([2 * s + (1 + np.arange(9)) * s, np.full(9, s)], axis=1)
    blobs_map = np.vstack([blob, bridge, blob + np.array([12 * s, 0.0])])  # 27
    maps = [grid_map, ring_map, blobs_map]
    assert [len(m) for m in maps] == [20, 34, 27]
    for m in maps:
        snd = oc.radius_graph(m, s * 1.2)[0]
        assert np.bincount(snd).max() <= 4 and np.bincount(snd, minlength=len(m)).min() >= 1
    return maps


B, R, M = 3, 3, 37


def _batch(nat):
    maps = _maps()
    h = nat.CoverageHandle(R, B, M, 75, 5.5)
    h.set_hidden(True)
    for b, m in enumerate(maps):
        h.set_targets(m, env=b)
    return h, maps


@pytest.mark.parametrize("streams", [0, 2])
def test_batch_follows_the_restatement(nat, streams):
    """Uniform device starts (own-node hiding is common), then 10 random steps; with
    streams=2 the steps run as two half-batch launches and the hidden pass behind both."""
    h, maps = _batch(nat)
    h.set_streams(streams)
    h.reset_seeded(11, 0.5)
    d = [_check_env(h, b, en.initial_discovered(M, R), maps[b], "reset env %d" % b) for b in range(B)]
    own_hidden = sum(int(d[b][h.robots(b)[1]].min() == 0) for b in range(B))
    assert own_hidden > 0  # some robot stands on a node nobody has seen
    rs = np.random.RandomState(5)
    robot_frontier = 0
    for t in range(10):
        a = rs.randint(0, 4, size=(B, R))
        if streams == 2:  # resident actions after a sync: the step splits
            h.set_actions(a)
            h.sync()
            h.step(resident=True)
        else:
            h.step(a)
        for b in range(B):
            d[b] = _check_env(h, b, d[b], maps[b], "step %d env %d" % (t, b))
            robot_frontier += int(h.hidden_obs(b)["nodes"][:R, 3].sum())
    assert robot_frontier > 0
    h.close()


def test_discovered_across_resets_and_graph_builds(nat):
    M1 = 16
    h = _line_handle(nat, M1)
    targets = _line()
    prev = h.discovered(0)
    for t in range(6):
        h.step(np.array([[1]]))
        cur = h.discovered(0)
        assert (cur >= prev).all()  # never loses a node within an episode
        prev = cur
    assert prev[12] == 1  # target 11, seen from target 7
    # a second reset starts again from the robots only (then sees from the new start)
    h.reset(np.array([[1]], np.int32), np.zeros((1, M1 - 1), np.uint8))
    np.testing.assert_array_equal(h.discovered(0), [1, 1, 0, 1, 1, 1, 1] + [0] * 9)
    _check_env(h, 0, en.initial_discovered(M1, 1), targets, "second reset")
    # robots placed elsewhere: the set is left alone until the next observation
    before = h.discovered(0)
    h.set_robot_positions(0, targets[[9]])
    np.testing.assert_array_equal(h.discovered(0), before)
    # a new graph: robots only
    h.set_targets(targets + 1.0, env=0)
    np.testing.assert_array_equal(h.discovered(0), en.initial_discovered(M1, 1))
    h.close()


def _oracle_tables(m, horizon=10):
    s, q, _ = oc.radius_graph(m, 5.5 * 1.2)
    nbr, cnt = oc.neighbour_table(len(m), s, q)
    cost, prev = oc.time_matrix(len(m), s, q, horizon=horizon)
    return nbr, cnt, cost, prev


def _stepped_batch(nat):
    """The batch after an explicit reset and 3 steps, then env 0's robots placed so that
    target 0 (unvisited, discovered, one hop from robot 0) is the expert's nearest candidate.
    Env 2's robots start in one blob and its only unvisited targets lie at the bridge's far
    end, within the horizon but out of sight."""
    h, maps = _batch(nat)
    start = np.array([[13, 18, 19], [3, 12, 20], [0, 1, 3]], np.int32)
    visited = np.zeros((B, M - R), np.uint8)
    visited[:, 5::3] = 1
    visited[2] = 1
    visited[2, [15, 16, 17]] = 0
    h.reset(start, visited)
    rs = np.random.RandomState(9)
    for _ in range(3):
        h.step(rs.randint(0, 4, size=(B, R)))
    # border nodes of the 4 x 5 grid (degree <= 3): action 3 is a padding loop, they stay
    h.set_robot_positions(0, maps[0][[1, 19, 15]])
    a = rs.randint(0, 4, size=(B, R))
    a[0] = 3
    h.step(a)
    np.testing.assert_array_equal(h.robots(0)[1], np.array([1, 19, 15]) + R)
    return h, maps


def test_masked_greedy_and_refused_fused_forms(nat):
    h, maps = _stepped_batch(nat)
    acts, rnd = h.controller_greedy()
    differs = 0
    for b in range(B):
        T = len(maps[b])
        nbr, cnt, cost, prev = _oracle_tables(maps[b])
        cur = h.robots(b)[1].astype(np.int64)
        recv = oc.action_receivers(cur, nbr, cnt, R)
        vis, disc = h.visited(b)[:T], h.discovered(b)[R:R + T]
        e_a, e_r = en.masked_greedy_actions(cost, prev, cur, vis, disc, recv, R)
        np.testing.assert_array_equal(acts[b], e_a, err_msg="env %d" % b)
        np.testing.assert_array_equal(rnd[b], e_r, err_msg="env %d" % b)
        p_a, p_r = oc.greedy_actions(cost, prev, cur, vis, recv, R)  # without the discovered mask
        differs += int(np.any(p_r != e_r) or np.any(p_a != e_a))
        if b == 0:  # the column-0 quirk decides: target 0 would be robot 0's first nearest candidate
            assert vis[0] == 0 and disc[0] == 1 and cost[cur[0] - R, 0] == 1 and vis.any()
            plain = np.where((vis == 1) | (disc == 0), oc.MAX_COST, cost[cur[0] - R])
            assert np.argmin(plain) == 0 and not e_r[0]
            assert prev[0, cur[0] - R] + R != recv[0][e_a[0]]  # the expert did not head for target 0
    assert differs > 0 and rnd[2].all()  # env 2: every unvisited target is undiscovered, the expert gives up
    # the fused forms read the visited flags inside the step: refused, with the route named
    a = np.zeros((B, R), np.int32)
    lib = h.lib
    for rc in (lib.cov_step(h.h, None, nat.COV_ACTIONS_GREEDY),
               lib.cov_step(h.h, None, nat.COV_ACTIONS_GREEDY | nat.COV_GREEDY_RNG),
               lib.cov_step_expert(h.h, 1, None, None),
               lib.cov_step_host(h.h, a.ctypes.data, None, None, None, None, None, None, None, None, None, None, 0),
               lib.cov_step_host(h.h, a.ctypes.data, None, None, None, None, None, None, None, None, None, None,
                                 nat.COV_NEXT_GREEDY)):
        assert rc == nat.GF_EINVAL
        assert b"cov_controller_greedy" in lib.fe_last_error()
    h.close()


def test_wire_formats_carry_the_hidden_observation(nat):
    from gym_flock.envs.spatial import CoverageEnv
    h, maps = _batch(nat)
    # env 0: robots on (0, 0), (16.5, 22) and (11, 22) of the grid, where action 3 is a padding
    # loop: nobody ever sees target 0 (23.3 and 24.6 away), so graph 0 has hidden motion edges
    h.reset(np.array([[0, 19, 14], [3, 12, 20], [0, 1, 3]], np.int32), np.zeros((B, M - R), np.uint8))
    rs = np.random.RandomState(2)
    for _ in range(3):
        a = rs.randint(0, 4, size=(B, R))
        a[0] = 3
        h.step(a)
    obs = [h.hidden_obs(b) for b in range(B)]
    assert h.discovered(0)[R] == 0 and (obs[0]["senders"][:h.n_motion()[0]] == -1).sum() == 4
    rows = np.stack([oc.flatten_obs(o) for o in obs])
    assert rows.shape == (B, 16 * M + 1) and rows.dtype == np.float64
    flat = h.flat_obs()
    assert flat.dtype == np.float64
    np.testing.assert_array_equal(flat, rows)
    flat32 = h.flat_obs(f32=True)
    assert flat32.dtype == np.float32
    np.testing.assert_array_equal(flat32, rows.astype(np.float32))

    class _Space:
        shape = (16 * M + 1,)

    names = ("n_node", "nodes", "n_edge", "edges", "senders", "receivers", "globs")
    exp = dict(zip(names, CoverageEnv.unpack_obs(flat32, _Space, dim_nodes=4)[1:]))
    got = h.graphs_tuple()
    assert got["nodes"].shape == (B * M, 4)
    for k in names:
        np.testing.assert_array_equal(got[k], np.asarray(exp[k]).reshape(got[k].shape), err_msg=k)
    assert got["n_edge"][0] < h.n_motion()[0] + 8 * R and (got["n_edge"][1:] == 4 * M).all()
    # mask_all: every graph drops the slots whose hidden sender is -1
    keep = [o["senders"] != -1 for o in obs]
    got = h.graphs_tuple(mask_all=True)
    np.testing.assert_array_equal(got["n_edge"], [k.sum() for k in keep])
    np.testing.assert_array_equal(got["edges"], np.concatenate([o["edges"][k] for o, k in zip(obs, keep)]))
    np.testing.assert_array_equal(got["senders"], np.concatenate([o["senders"][k] + b * M for b, (o, k) in enumerate(zip(obs, keep))]))
    np.testing.assert_array_equal(got["receivers"], np.concatenate([o["receivers"][k] + b * M for b, (o, k) in enumerate(zip(obs, keep))]))
    np.testing.assert_array_equal(got["nodes"], np.concatenate([o["nodes"] for o in obs]).astype(np.float32))
    h.close()


# ------------------------------------------------------------------------ the drop-in env
@pytest.fixture(scope="module")
def fx():
    return np.load(os.path.join(GOLDEN, "coverage_explore.npz"))


def _assert_obs(obs, f, pre, suffix, t, env):
    rec = (lambda k: f[pre + k + "0"]) if t is None else (lambda k: f[pre + k][t])
    assert obs["nodes"].dtype == np.float64 and obs["nodes"].shape == (env.max_nodes, 4)
    for k in OBS_KEYS:
        np.testing.assert_array_equal(np.asarray(obs[k]).reshape(rec(k).shape), rec(k), err_msg="%s, %s" % (k, suffix))
    assert env.discovered_nodes.shape == (env.max_nodes, 1) and env.discovered_nodes.dtype == np.float64
    np.testing.assert_array_equal(env.discovered_nodes[:, 0], rec("discovered"), err_msg="discovered, " + suffix)


@pytest.mark.parametrize("pre,policy", [("g_", "greedy"), ("r_", "random")])
def test_explore_episode_replays_the_reference(fx, grid, pre, policy):
    import gym_flock
    f = fx
    map_seed, env_seed = int(f[pre + "map_seed"]), int(f[pre + "env_seed"])
    np.random.seed(map_seed)
    env = gym_flock.make("ExploreEnv-v0", occupancy=grid)
    assert env.hide_nodes and env.n_node_feat == 4 and env.horizon == 19 and env.episode_length == 50
    assert env.observation_space.spaces["nodes"].shape == (env.max_nodes, 4)
    env.seed(env_seed)
    np.random.seed(map_seed)
    obs = env.reset()
    R = int(f[pre + "n_robots"])
    assert env.n_targets == int(f[pre + "n_targets"]) and env.max_nodes == int(f[pre + "max_nodes"])
    np.testing.assert_array_equal(env.x, f[pre + "x0"])
    _assert_obs(obs, f, pre, "reset", None, env)
    n = len(f[pre + "reward"])
    for t in range(n):
        if policy == "greedy":
            a = env.controller(random=False, greedy=True)
            np.testing.assert_array_equal(a.flatten(), f[pre + "actions"][t], err_msg="greedy actions, step %d" % t)
        else:
            a = f[pre + "actions"][t].reshape(-1, 1)
        obs, r, d, _ = env.step(a)
        assert r == f[pre + "reward"][t] and d == f[pre + "done"][t], (t, r, d)
        _assert_obs(obs, f, pre, "step %d" % t, t, env)
        np.testing.assert_array_equal(env.closest_targets, f[pre + "closest"][t])
    assert d and n < 50
    np.testing.assert_array_equal(env.visited[:, 0], f[pre + "visited"][-1])
    if policy == "greedy":
        assert env.np_random.uniform() == f[pre + "probe"]
    env.close()


def test_other_hide_nodes_combinations_keep_raising(grid):
    from gym_flock.envs.spatial import CoverageARLEnv
    for kw in (dict(hide_nodes=True), dict(n_node_feat=4), dict(hide_nodes=True, n_node_feat=5)):
        with pytest.raises(NotImplementedError):
            CoverageARLEnv(occupancy=grid, **kw)


def test_vec_coverage_hidden(nat):
    from gym_flock.vec import VecCoverage
    v = VecCoverage(B, R, max_nodes=M, hide_nodes=True)
    maps = _maps()
    for b, m in enumerate(maps):
        v.set_targets(m, env=b)
    v.reset(seed=3)
    d = [_check_env(v.h, b, en.initial_discovered(M, R), maps[b]) for b in range(B)]
    v.step(greedy=True)  # controller_greedy, the fallback draws on the host, a resident step
    for b in range(B):
        _check_env(v.h, b, d[b], maps[b])
        o = v.obs(b)
        assert o["nodes"].shape == (M, 4)
        np.testing.assert_array_equal(o["senders"], v.h.hidden_obs(b)["senders"])
    assert v.flat_obs().shape == (B, 16 * M + 1)
    with pytest.raises(nat.GymFlockError):
        v.expert_steps(2)
    v.close()


def test_hiding_off_is_unchanged(nat, grid):
    """A handle without set_hidden and CoverageARLEnv() at its defaults give the observations
    they gave before: the first recorded step of coverage_arl.npz."""
    from gym_flock.envs.spatial import CoverageARLEnv
    f = np.load(os.path.join(GOLDEN, "coverage_arl.npz"))
    pre = "r_"
    map_seed, env_seed = int(f[pre + "map_seed"]), int(f[pre + "env_seed"])
    np.random.seed(map_seed)
    env = CoverageARLEnv(occupancy=grid)
    env.seed(env_seed)
    np.random.seed(map_seed)
    obs = env.reset()
    for k in OBS_KEYS:
        np.testing.assert_array_equal(np.asarray(obs[k]).reshape(f[pre + k + "0"].shape), f[pre + k + "0"], err_msg=k)
    obs, r, d, _ = env.step(f[pre + "actions"][0].reshape(-1, 1))
    assert obs["nodes"].dtype == np.float32 and obs["nodes"].shape == (env.max_nodes, 3)
    for k in OBS_KEYS:
        np.testing.assert_array_equal(np.asarray(obs[k]).reshape(f[pre + k][0].shape), f[pre + k][0], err_msg=k)
    assert r == f[pre + "reward"][0] and d == f[pre + "done"][0]
    h = env._h
    assert h.n_node_feat == 3 and h.flat_obs().shape == (1, 15 * env.max_nodes + 1)
    assert h.lib.cov_get_hidden_obs(h.h, 0, None, None, None) == nat.GF_ESTATE
    with pytest.raises(AttributeError):
        env.discovered_nodes
    env.close()
