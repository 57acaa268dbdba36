"""Coverage maps of up to 8,192 targets on the GPU: the time matrix's narrower tiles and the
schedule's global scratch at the smallest maps where they can go wrong, the occupancy pool,
the motion graph and the seeded reset at and around their former limits, and the reference's
ExploreFullEnv configuration (5,659 targets, 100 robots, hidden nodes) against its recorded
steps (tests/golden/coverage_explore_full.npz). Every comparison is exact: all values are
hop counts, indices, flags or coordinates copied from the inputs. Needs an MI355X."""
import os
import sys
import time

import numpy as np
import pytest

from conftest import GOLDEN
from oracle import coverage as oc

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import coverage_arl_numpy as an  # noqa: E402
from coverage_large_inputs import line, walled_grid, walled_reference  # noqa: E402

pytestmark = pytest.mark.gpu

nat = pytest.importorskip("gym_flock._native")

PLANS = [(S, g) for S in (8, 16, 32) for g in (0, 1)]


@pytest.fixture(scope="module")
def grid():
    return np.load(os.path.join(GOLDEN, "grid_slice10.npy"))


@pytest.fixture(scope="module")
def small_maps():
    """(targets, graph_cost, graph_previous) at horizon 10 of the two recorded maps
    (T = 394, 613) and of the 300-target path (the oracle's), computed once."""
    out = []
    for name in ("coverage_r6_greedy.npz", "coverage_r20_greedy.npz"):
        f = np.load(os.path.join(GOLDEN, name))
        assert len(f["targets"]) == int(f["n_targets"])
        out.append((f["targets"], f["graph_cost"], f["graph_previous"]))
    assert [len(m[0]) for m in out] == [394, 613]
    out.append((line(),) + _oracle(line(), 10))
    return out


def _oracle(targets, horizon):
    s, q, _ = oc.radius_graph(targets, 5.5 * 1.2)
    return oc.time_matrix(len(targets), s, q, horizon=horizon)


def _check_plans(h, envs, expected):
    """Every plan's matrices equal `expected` (per env: cost, prev) and the default plan's."""
    base = [h.time_matrix(b, len(expected[b][0])) for b in envs]
    for b in envs:
        np.testing.assert_array_equal(base[b][0], expected[b][0], err_msg="cost, env %d, default plan" % b)
        np.testing.assert_array_equal(base[b][1], expected[b][1], err_msg="prev, env %d, default plan" % b)
    for S, g in PLANS + [(64, 1), (0, 0)]:
        h.set_tm_plan(S, bool(g))
        for b in envs:
            cost, prev = h.time_matrix(b, len(expected[b][0]))
            np.testing.assert_array_equal(cost, base[b][0], err_msg="cost, env %d, plan (%d, %d)" % (b, S, g))
            np.testing.assert_array_equal(prev, base[b][1], err_msg="prev, env %d, plan (%d, %d)" % (b, S, g))


# --------------------------------------------------------------- 1. narrow tiles at small T
@pytest.mark.parametrize("which", [0, 1])
def test_narrow_tiles_give_the_recorded_matrices(small_maps, which):
    """T = 394 and 613: no multiple of 8, so every S has a partial last chunk."""
    targets, cost, prev = small_maps[which]
    T = len(targets)
    h = nat.CoverageHandle(6, 1, T + 6, horizon=10)
    h.set_targets(targets, env=0)
    _check_plans(h, [0], [(cost, prev)])
    h.close()


def test_narrow_tiles_rerun_with_two_byte_entries():
    """The 300-target path, unbounded horizon: hop counts reach 299, so the one-byte pass
    gives up and the two-byte rerun runs at each S (its own, narrower where the plan's tile
    would not fit)."""
    targets = line()
    T = len(targets)
    cost, prev = _oracle(targets, -1)
    assert cost.max() == 299 and cost[0, 299] == 299
    h = nat.CoverageHandle(8, 1, T + 10, horizon=-1)
    h.set_targets(targets, env=0)
    _check_plans(h, [0], [(cost, prev)])
    h.close()


@pytest.mark.parametrize("horizon", [10, -1])
def test_narrow_tiles_in_a_batch_of_unequal_maps(small_maps, horizon):
    """Three envs of 394, 613 and 300 targets in one launch: the grid is sized for 613, the
    smaller envs' last chunks are partial and their later chunks return at once. Horizon 10
    against the recorded matrices and the oracle; unbounded (the path alone overflows the
    one-byte entries and is rerun) against the handle's own S = 64 result and the path's
    oracle."""
    maps = [m[0] for m in small_maps]
    Tm = max(len(m) for m in maps)
    h = nat.CoverageHandle(6, 3, Tm + 6, horizon=horizon)
    for b, m in enumerate(maps):
        h.set_targets(m, env=b)
    if horizon == 10:
        _check_plans(h, [0, 1, 2], [(m[1], m[2]) for m in small_maps])
    else:
        base = [h.time_matrix(b, len(maps[b])) for b in range(3)]
        lc, lp = _oracle(maps[2], -1)
        np.testing.assert_array_equal(base[2][0], lc)
        np.testing.assert_array_equal(base[2][1], lp)
        _check_plans(h, [0, 1, 2], base)
    h.close()


def test_tm_plan_refusals():
    h = nat.CoverageHandle(4, 1, 2604, horizon=10)  # 2,600 targets: (2600 + 1) * 64 bytes > 160 KB
    lib = h.lib
    for S in (7, -8, 1, 128):
        assert lib.cov_set_tm_plan(h.h, S, 0) == nat.GF_EINVAL
    assert lib.cov_set_tm_plan(h.h, 32, 2) == nat.GF_EINVAL
    assert lib.cov_set_tm_plan(h.h, 64, 0) == nat.GF_EINVAL
    assert b"160 KB" in lib.fe_last_error()
    h.set_tm_plan(32)
    h.close()
    h = nat.CoverageHandle(4, 1, 2563, horizon=10)  # 2,559 targets: the widest tile still fits
    h.set_tm_plan(64)
    h.close()


# ------------------------------------------------------------------- 2. pool boundaries
def _arl_handle(n_envs=1, max_nodes=1000):
    return nat.CoverageHandle(4, n_envs, max_nodes, 50, 5.0)


@pytest.mark.parametrize("block", [(17, 241), (64, 128)])
def test_pools_past_the_former_cap_load(block):
    raw, pool, lo, hi, sub = walled_reference(*block)
    h = _arl_handle()
    cfg = nat.occupancy_config(perimeter_delta=max(block) + 2)
    assert h.load_occupancy(walled_grid(*block), cfg) == len(pool) == block[0] * block[1]
    got, glo, ghi, gsub = h.pool()
    np.testing.assert_array_equal(got, pool)
    np.testing.assert_array_equal(glo, lo)
    np.testing.assert_array_equal(ghi, hi)
    np.testing.assert_array_equal(gsub, sub)
    h.close()


def test_pool_one_past_the_cap_is_refused(grid):
    h = _arl_handle()
    with pytest.raises(nat.GymFlockError) as e:
        h.load_occupancy(walled_grid(3, 2731), nat.occupancy_config(perimeter_delta=2733))
    assert e.value.code == nat.GF_EINVAL and "more than the pool holds" in str(e.value)
    assert "8193" in str(e.value) and "8192" in str(e.value)
    assert h.load_occupancy(grid) == 1266  # the handle is still usable
    h.close()


def test_submaps_of_the_largest_pool():
    block = (64, 128)
    raw, pool, lo, hi, sub = walled_reference(*block)
    B = 4
    h = _arl_handle(B, 1500)
    assert h.load_occupancy(walled_grid(*block), nat.occupancy_config(perimeter_delta=max(block) + 2)) == 8192
    n, st, tries = h.generate_submaps(map_seed=0)
    np.testing.assert_array_equal(st, 0)
    for b in range(B):
        np.random.seed(b)
        idx, k = an.sample_submap(pool, lo, hi, sub, 6.0)
        assert tries[b] == k and n[b] == len(idx) and 200 <= len(idx) <= 1496
        np.testing.assert_array_equal(h.targets(b, n[b]), pool[idx], err_msg="env %d" % b)
    h.close()


# ------------------------------------------------------- 3. motion graph above 4,096 targets
@pytest.mark.parametrize("block", [(17, 241), (64, 128)], ids=["lds-4097", "scan-8192"])
def test_motion_graph_above_the_former_limit(block):
    """4,097 targets take the kernel form with the targets and a cell grid in LDS (98 KB),
    8,192 the form in which every node scans every target."""
    pool = walled_reference(*block)[1]
    T, R = len(pool), 4
    h = nat.CoverageHandle(R, 1, T + R, 50, 5.0)
    h.set_targets(pool, env=0)
    s, q, _ = oc.radius_graph(pool, 5.0 * 1.2)
    assert np.bincount(s).max() == 4
    assert h.n_motion()[0] == len(s)
    snd, rcv = h.motion_edges(0)
    np.testing.assert_array_equal(snd, s + R)
    np.testing.assert_array_equal(rcv, q + R)
    h.close()


# ----------------------------------------------------- 4. seeded reset past the old guard
def test_seeded_reset_with_7100_targets():
    """max_nodes - n_robots = 7,100: past the former guard's 65,536 bytes (it counted 5 bytes
    per target where the kernel uses 9: 66,396 here) and inside the kernel's raised LDS."""
    pool = walled_reference(64, 128)[1]
    T, R, B, seed = 7100, 4, 2, 9
    h = nat.CoverageHandle(R, B, T + R, 50, 5.0)
    h.set_targets(pool[:T])
    start, visited = h.reset_seeded(seed, 0.5)
    for b in range(B):
        rs = np.random.RandomState(seed + b)
        np.testing.assert_array_equal(start[b], rs.choice(np.arange(T), size=(R,), replace=False))
        unv = rs.choice(np.arange(T) + R, size=(int(T * 0.5),), replace=False)
        exp = np.ones(T, np.uint8)
        exp[unv - R] = 0
        np.testing.assert_array_equal(visited[b], exp)
        np.testing.assert_array_equal(h.robots(b)[1], start[b] + R)
    h.close()


# ------------------------------------------------------------- 5. the full configuration
FULL_KW = dict(hide_nodes=True, n_node_feat=4, n_robots=100, episode_length=50, pad_nodes=False, max_nodes=1500,
               nearby_starts=True, num_subgraphs=1, check_connected=True, downsample_rate=10, perimeter_delta=12.0,
               horizon=19)


def _bits(a):
    return np.packbits(np.asarray(a).astype(np.uint8).ravel())


def test_explore_full_configuration_replays_the_reference(grid):
    from gym_flock.envs.spatial import CoverageARLEnv
    f = np.load(os.path.join(GOLDEN, "coverage_explore_full.npz"))
    np.random.seed(int(f["map_seed"]))
    env = CoverageARLEnv(occupancy=grid, **FULL_KW)
    env.seed(int(f["env_seed"]))
    np.random.seed(int(f["map_seed"]))
    obs = env.reset()
    R, T, M = 100, 5659, 5759
    assert env.n_targets == T == int(f["n_targets"]) and env.max_nodes == M == int(f["max_nodes"])
    np.testing.assert_array_equal(env.x[R:, :2], f["targets"])
    np.testing.assert_array_equal(env.x, f["x0"])
    np.testing.assert_array_equal(_bits(env.visited[:, 0]), f["visited0"])
    np.testing.assert_array_equal(_bits(np.array(env.start_region, bool)), f["start_region"])
    np.testing.assert_array_equal(np.asarray(obs["edges"]).reshape(-1), f["edges0"].reshape(-1))
    np.testing.assert_array_equal(np.asarray(obs["receivers"]), f["receivers0"])
    np.testing.assert_array_equal(np.asarray(obs["step"]).reshape(-1), f["step0"].reshape(-1))
    stored = f["stored_senders0"]

    def check_obs(o, rec, msg):
        assert o["nodes"].dtype == np.float64 and o["nodes"].shape == (M, 4)
        assert set(np.unique(o["nodes"])) <= {0.0, 1.0}
        np.testing.assert_array_equal(_bits(o["nodes"]), rec("nodes"), err_msg="nodes, " + msg)
        snd = np.asarray(o["senders"])
        kept = snd != -1
        np.testing.assert_array_equal(_bits(kept), rec("kept"), err_msg="kept senders, " + msg)
        nm = env._h.n_motion()[0]  # the motion edges' senders never change; the tail follows the robots
        np.testing.assert_array_equal(snd[:nm][kept[:nm]], stored[:nm][kept[:nm]], err_msg="senders, " + msg)
        np.testing.assert_array_equal(_bits(env.discovered_nodes[:, 0]), rec("discovered"), err_msg="discovered, " + msg)

    assert env._h.n_motion()[0] == 20910
    check_obs(obs, lambda k: f[k + "0"], "reset")
    for t in range(len(f["reward"])):
        t0 = time.perf_counter()
        a = env.controller(random=False, greedy=True)
        if t == 0:
            print("first greedy call (time matrix of 5,659 targets included): %.3f s" % (time.perf_counter() - t0))
        np.testing.assert_array_equal(a.flatten(), f["actions"][t], err_msg="greedy actions, step %d" % t)
        obs, r, d, _ = env.step(a)
        assert r == f["reward"][t] and d == f["done"][t], (t, r, d)
        check_obs(obs, lambda k: f[k][t], "step %d" % t)
        np.testing.assert_array_equal(np.asarray(obs["step"]).reshape(-1), f["step"][t].reshape(-1))
        np.testing.assert_array_equal(_bits(env.visited[:, 0]), f["visited"][t])
        np.testing.assert_array_equal(env.closest_targets, f["closest"][t])
        np.testing.assert_array_equal(env.x[:R, :2], f["xr"][t])
    assert env.np_random.uniform() == f["probe"]
    # the time matrix against the digest: every source's finite entries, and 8 whole rows
    cost, prev = env._h.time_matrix(0, T)
    fin = cost < oc.MAX_COST
    assert cost.max() == oc.MAX_COST and cost[fin].max() == int(f["tm_max_finite"]) == 205
    np.testing.assert_array_equal(fin.sum(axis=1), f["tm_count"])
    np.testing.assert_array_equal(np.where(fin, cost, 0).sum(axis=1, dtype=np.int64), f["tm_sum"])
    rows = f["tm_rows"]
    np.testing.assert_array_equal(cost[rows], f["tm_cost_rows"])
    np.testing.assert_array_equal(prev[rows], f["tm_prev_rows"])
    env.close()
