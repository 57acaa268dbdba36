"""cov_reset_device on the GPU: reset() of chosen envs from their continued np_random
streams, with the reference's nearby_starts region, against numpy's RandomState
(tests/coverage_reset_numpy.py), twin handles, the CPU oracle and the reference's recorded
resets (tests/golden/coverage_arl.npz, coverage_explore.npz). All comparisons are exact."""
import os
import sys

import numpy as np
import pytest

from conftest import GOLDEN

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import coverage_explore_numpy as en  # noqa: E402
import coverage_reset_numpy as rn  # noqa: E402
from oracle import coverage as oc  # noqa: E402

pytestmark = pytest.mark.gpu

OBS_KEYS = ("nodes", "edges", "senders", "receivers", "step")
S = 5.5  # Coverage-v0's res: motion radius 6.6


@pytest.fixture(scope="module")
def nat():
    from gym_flock import _native
    return _native


@pytest.fixture(scope="module")
def arl():
    return np.load(os.path.join(GOLDEN, "coverage_arl.npz"))


@pytest.fixture(scope="module")
def grid():
    return np.load(os.path.join(GOLDEN, "grid_slice10.npy"))


def _grid_map(n, width=4, s=S):
    """The first n points of a `width`-wide grid of spacing s (degree <= 4)."""
    k = np.arange(n)
    return np.stack([(k % width) * s, (k // width) * s], axis=1).astype(np.float64)


def _line(n=12, s=S):
    return np.stack([np.arange(n) * s, np.zeros(n)], axis=1)


def _edges(m, s=S):
    snd, rcv, _ = oc.radius_graph(m, s * 1.2)
    return snd, rcv


def _at(seed, k):
    """RandomState(seed) after k one-word draws: position k (k >= 1; 0 draws: 624)."""
    rs = np.random.RandomState(seed)
    if k:
        rs.choice(4, size=k)
        assert rs.get_state()[2] == k
    return rs


def _rng_of(h, b):
    keys, pos = h.get_rng()
    rs = np.random.RandomState()
    rs.set_state(("MT19937", keys[b], int(pos[b])))
    return rs


def _assert_stream(h, b, rs, msg=""):
    keys, pos = h.get_rng()
    st = rs.get_state()
    assert int(pos[b]) == st[2], (msg, b, int(pos[b]), st[2])
    np.testing.assert_array_equal(keys[b], st[1], err_msg="key of env %d %s" % (b, msg))


def _snapshot(h, b, hidden=False):
    x, nodes = h.robots(b)
    r, d = h.rewards()
    a, nr = h.actions()
    keys, pos = h.get_rng()
    s = {"x": x, "cur": nodes, "visited": h.visited(b), "reward": r[b], "done": d[b], "actions": a[b],
         "key": keys[b].copy(), "pos": int(pos[b])}
    for k, v in h.obs(b).items():
        s["obs_" + k] = v
    if hidden:
        for k, v in h.hidden_obs(b).items():
            s["hid_" + k] = v
        s["discovered"] = h.discovered(b)
    return s


def _assert_same(a, b, msg):
    assert a.keys() == b.keys()
    for k in a:
        np.testing.assert_array_equal(a[k], b[k], err_msg="%s: %s" % (msg, k))


def _assert_reset_state(h, b, m, R, M, start, visited, msg, s=S):
    """Env b equals the CPU oracle's reset on map m from (start, visited)."""
    o = oc.CoverageOracle(m, R, M, motion_radius=s * 1.2)
    ref = o.reset(start, np.nonzero(visited[:len(m)] == 0)[0] + R)
    got = h.obs(b)
    for k in OBS_KEYS:
        np.testing.assert_array_equal(got[k].reshape(ref[k].shape), ref[k], err_msg="%s %s" % (msg, k))
    np.testing.assert_array_equal(h.robots(b)[0], m[start], err_msg=msg)
    np.testing.assert_array_equal(h.visited(b)[:len(m)], o.visited[R:], err_msg=msg)
    return o


# ------------------------------------------------------------------ 1. continued streams
def test_continued_streams_all_envs_uniform_starts(nat):
    R, M = 3, 40
    maps = [_grid_map(n) for n in (20, 33, 37, 12, 28)]
    B = len(maps)
    pos = [620, 623, 624, 0, 17]  # 624: every word consumed; 0: a fresh RandomState (also 624)
    rss = [_at(100 + b, pos[b]) for b in range(B)]
    h, twin = nat.CoverageHandle(R, B, M), nat.CoverageHandle(R, B, M)
    for b, m in enumerate(maps):
        h.set_targets(m, env=b)
        twin.set_targets(m, env=b)
    with pytest.raises(nat.GymFlockError) as e:  # no streams on the device yet
        h.reset_device(None, 0.5, 0)
    assert e.value.code == nat.GF_ESTATE
    h.set_rng(rss)
    n, start, visited, region, status = h.reset_device(None, 0.5, 0)
    assert n == B and (status == 0).all()
    exp_start = np.zeros((B, R), np.int32)
    exp_vis = np.ones((B, M - R), np.uint8)
    for b, m in enumerate(maps):
        T = len(m)
        rs = rss[b]
        exp_start[b] = rs.choice(np.arange(T), size=(R,), replace=False)
        drop = rs.choice(np.arange(T) + R, size=(int(T * 0.5),), replace=False)
        exp_vis[b, drop - R] = 0
        _assert_stream(h, b, rs, "after the reset")
        np.testing.assert_array_equal(region[b], np.arange(M - R) < T)
    np.testing.assert_array_equal(start, exp_start)
    np.testing.assert_array_equal(visited, exp_vis)
    twin.reset(exp_start, exp_vis)
    for b in range(B):
        for k, v in twin.obs(b).items():
            np.testing.assert_array_equal(h.obs(b)[k], v, err_msg="env %d %s" % (b, k))
        np.testing.assert_array_equal(h.robots(b)[0], twin.robots(b)[0])
        np.testing.assert_array_equal(h.visited(b), twin.visited(b))
    np.testing.assert_array_equal(h.rewards()[0], twin.rewards()[0])
    np.testing.assert_array_equal(h.rewards()[1], twin.rewards()[1])
    # a second episode continues each stream again (the reference's second reset())
    n, start2, visited2, _, _ = h.reset_device(None, 0.5, 0)
    for b, m in enumerate(maps):
        T = len(m)
        np.testing.assert_array_equal(start2[b], rss[b].choice(np.arange(T), size=(R,), replace=False))
        drop = rss[b].choice(np.arange(T) + R, size=(int(T * 0.5),), replace=False)
        v = np.ones(M - R, np.uint8)
        v[drop - R] = 0
        np.testing.assert_array_equal(visited2[b], v)
        _assert_stream(h, b, rss[b], "after the second reset")
    # COV_RESET_SEED and nearby = 0 are cov_reset_seeded's draws
    n, s3, v3, _, _ = h.reset_device(None, 0.5, 0, seed=11)
    s4, v4 = twin.reset_seeded(11, 0.5)
    np.testing.assert_array_equal(s3, s4)
    np.testing.assert_array_equal(v3, v4)
    np.testing.assert_array_equal(h.get_rng()[0], twin.get_rng()[0])
    np.testing.assert_array_equal(h.get_rng()[1], twin.get_rng()[1])
    # what the call refuses
    for kw in ({"frac_active": 1.5}, {"frac_active": -0.1}, {"nearby": -1}, {"seed": 2 ** 32 - 2}):
        with pytest.raises(nat.GymFlockError) as e:
            h.reset_device(None, **kw)
        assert e.value.code == nat.GF_EINVAL, kw
    import ctypes
    rc = nat.CovResetConfig(0.5, 0, 0x8, 0)
    assert h.lib.cov_reset_device(h.h, ctypes.byref(rc), None, None, None, None, None, None) == nat.GF_EINVAL
    h.close()
    twin.close()


# ------------------------------------------------------------------------ 2. masked reset
def test_masked_reset_leaves_the_other_envs_alone(nat):
    R, M, B, NEARBY = 3, 40, 6, 6
    maps = [_grid_map(n) for n in (20, 33, 37, 16, 28, 24)]
    h = nat.CoverageHandle(R, B, M)
    for b, m in enumerate(maps):
        h.set_targets(m, env=b)
    s0, v0 = h.reset_seeded(40, 0.5)
    orcs = []
    for b, m in enumerate(maps):
        orcs.append(_assert_reset_state(h, b, m, R, M, s0[b], v0[b], "seeded reset env %d" % b))
    act = np.random.RandomState(3)
    for _ in range(7):
        a = act.randint(0, 4, size=(B, R))
        h.step(a)
        for b in range(B):
            orcs[b].step(a[b])
    # selected streams at the key's end: the regeneration falls inside the scalar draw (env 1:
    # every word consumed), inside the region's permutation (env 4) or the second one (env 5)
    rss = [_rng_of(h, b) for b in range(B)]
    rss[1], rss[4], rss[5] = _at(201, 624), _at(204, 623), _at(205, 610)
    h.set_rng(rss)
    before = [_snapshot(h, b) for b in range(B)]
    mask = np.array([0, 1, 0, 0, 1, 1], bool)
    n, start, visited, region, status = h.reset_device(mask, 0.5, NEARBY)
    assert n == 3
    after = [_snapshot(h, b) for b in range(B)]
    for b in range(B):
        if not mask[b]:
            _assert_same(before[b], after[b], "unselected env %d" % b)
            assert not start[b].any() and not visited[b].any() and not region[b].any() and status[b] == 0
            continue
        m, T = maps[b], len(maps[b])
        d = rn.reset_draws(rss[b], T, R, 0.5, NEARBY, *_edges(m))
        assert d["status"] == status[b] == 0
        np.testing.assert_array_equal(region[b, :T], d["region"], err_msg="region env %d" % b)
        assert not region[b, T:].any()
        np.testing.assert_array_equal(start[b], d["start"], err_msg="start env %d" % b)
        np.testing.assert_array_equal(visited[b, :T], d["visited"], err_msg="visited env %d" % b)
        assert visited[b, T:].all()
        _assert_stream(h, b, rss[b], "selected")
        orcs[b] = _assert_reset_state(h, b, m, R, M, start[b], visited[b], "masked reset env %d" % b)
        np.testing.assert_array_equal(after[b]["actions"], before[b]["actions"])  # resident actions stay
    for t in range(3):
        a = act.randint(0, 4, size=(B, R))
        h.step(a)
        r, dn = h.rewards()
        for b in range(B):
            ref, rr, dd = orcs[b].step(a[b])
            assert r[b] == rr and dn[b] == dd, (t, b)
            got = h.obs(b)
            for k in OBS_KEYS:
                np.testing.assert_array_equal(got[k].reshape(ref[k].shape), ref[k], err_msg="t=%d b=%d %s" % (t, b, k))
    h.close()


# ------------------------------------------------------------------------ 3. region edges
def _seed_with(T, want, lo=0):
    """The first seed >= lo whose RandomState draws choice(T) in `want`."""
    s = lo
    while int(np.random.RandomState(s).choice(T)) not in want:
        s += 1
    return s


def test_region_on_a_line_overshoot_end_short_and_small(nat):
    R, M = 3, 20
    line = _line()
    pair_map = np.vstack([line[:10], np.array([[500.0, 0.0], [500.0 + S, 0.0]])])  # 10-line + an isolated pair
    B = 4
    h = nat.CoverageHandle(R, B, M)
    for b in range(3):
        h.set_targets(line, env=b)
    h.set_targets(pair_map, env=3)
    seeds = [_seed_with(12, (11,)), _seed_with(12, (0,)), _seed_with(12, (5, 6)), _seed_with(12, range(2, 8), 50)]

    def run(nearby, expect_fail=None):
        rss = [np.random.RandomState(s) for s in seeds]
        h.set_rng(rss)
        try:
            n, start, visited, region, status = h.reset_device(None, 0.5, nearby)
            assert expect_fail is None
        except nat.GymFlockError as e:
            assert expect_fail is not None and e.code == nat.GF_EINVAL and ("env %d" % expect_fail) in str(e), str(e)
            n, start, visited, region, status = e.n_reset, e.start, e.visited, e.region, e.status
        out = []
        for b in range(B):
            m = pair_map if b == 3 else line
            d = rn.reset_draws(rss[b], len(m), R, 0.5, nearby, *_edges(m))
            assert status[b] == d["status"], (nearby, b, status[b], d["status"])
            np.testing.assert_array_equal(region[b, :len(m)], d["region"], err_msg="nearby %d env %d" % (nearby, b))
            _assert_stream(h, b, rss[b], "nearby %d" % nearby)
            if d["start"] is not None:
                np.testing.assert_array_equal(start[b], d["start"])
                np.testing.assert_array_equal(visited[b, :len(m)], d["visited"])
                _assert_reset_state(h, b, m, R, M, start[b], visited[b], "nearby %d env %d" % (nearby, b))
            out.append(d)
        return n, out

    n, d = run(5)
    assert n == B
    assert np.nonzero(d[0]["region"])[0].tolist() == [7, 8, 9, 10, 11] and d[0]["rounds"] == 4  # i at the line's end
    assert np.nonzero(d[1]["region"])[0].tolist() == [0, 1, 2, 3, 4]
    assert d[2]["rounds"] == 2 and d[2]["region"].sum() == 5
    n, d = run(4)  # 1 -> 3 -> 5 nodes: the set overshoots nearby
    assert n == B and d[2]["region"].sum() == 5 and d[0]["region"].sum() == 4
    n, d = run(20)  # more than the line holds: the whole component, REGION_SHORT, and the call returns
    assert n == B
    for b in range(3):
        assert d[b]["status"] == nat.COV_RESET_REGION_SHORT and d[b]["region"].all()
    assert d[3]["status"] == nat.COV_RESET_REGION_SHORT and d[3]["region"].sum() == 10
    # the isolated pair: a region of 2 nodes for 3 robots. The env keeps its state; the others are reset
    seeds[3] = _seed_with(12, (10, 11))
    seeds[0] = seeds[1] = seeds[2]  # interior draws: regions of 3 nodes
    before = _snapshot(h, 3)
    n, d = run(2, expect_fail=3)
    assert n == 3 and d[3]["status"] == nat.COV_RESET_REGION_SMALL and d[3]["region"].sum() == 2
    after = _snapshot(h, 3)
    for k in before:
        if k not in ("key", "pos"):  # its stream has advanced by the scalar draw
            np.testing.assert_array_equal(before[k], after[k], err_msg=k)
    h.close()


@pytest.mark.parametrize("T", [33, 64, 65])
def test_region_at_the_bit_word_edges(nat, T):
    R = 3
    M = T + R
    m = _grid_map(T)
    B = 3
    h = nat.CoverageHandle(R, B, M)
    h.set_targets(m)
    # i in the last word's first bits, in the last bit of a full word, anywhere
    seeds = [_seed_with(T, (T - 1,)), _seed_with(T, (31, 32, 63, 64)), 7]
    rss = [np.random.RandomState(s) for s in seeds]
    h.set_rng(rss)
    n, start, visited, region, status = h.reset_device(None, 0.5, 5 * R)
    assert n == B
    for b in range(B):
        d = rn.reset_draws(rss[b], T, R, 0.5, 5 * R, *_edges(m))
        assert status[b] == d["status"] == 0 and d["region"].sum() >= 5 * R
        np.testing.assert_array_equal(region[b], d["region"])
        np.testing.assert_array_equal(start[b], d["start"])
        np.testing.assert_array_equal(visited[b], d["visited"])
        _assert_stream(h, b, rss[b])
        _assert_reset_state(h, b, m, R, M, start[b], visited[b], "T %d env %d" % (T, b))
    h.close()


# ----------------------------------------------------------------- 4. the recorded maps
@pytest.mark.parametrize("pre,env_seed", [("g_", 6), ("r_", 4), ("full_", 12)])
def test_recorded_resets(nat, arl, pre, env_seed):
    f = arl
    R, T, M = int(f[pre + "n_robots"]), int(f[pre + "n_targets"]), int(f[pre + "max_nodes"])
    h = nat.CoverageHandle(R, 1, M, 50, 5.0)
    h.set_targets(f[pre + "targets"], env=0)
    rs = np.random.RandomState(env_seed)
    h.set_rng([rs])
    n, start, visited, region, status = h.reset_device(None, 0.5, 5 * R)
    assert n == 1 and status[0] == 0
    np.testing.assert_array_equal(region[0, :T].astype(bool), f[pre + "start_region"])
    x, _ = h.robots(0)
    np.testing.assert_array_equal(x, f[pre + "x0"][:R])
    np.testing.assert_array_equal(h.visited(0)[:T], f[pre + "visited0"][R:])
    o = h.obs(0)
    for k in ("nodes", "edges", "senders", "receivers"):
        np.testing.assert_array_equal(o[k].reshape(f[pre + k + "0"].shape), f[pre + k + "0"], err_msg=k)
    d = rn.reset_draws(rs, T, R, 0.5, 5 * R, f[pre + "motion_senders"] - R, f[pre + "motion_receivers"] - R)
    np.testing.assert_array_equal(start[0], d["start"])
    _assert_stream(h, 0, rs)
    h.close()


# -------------------------------------------------------------------- 5. COV_RESET_DONE
def test_reset_of_the_done_envs(nat):
    R, M, B = 3, 40, 4
    maps = [_grid_map(n) for n in (20, 24, 28, 32)]
    h = nat.CoverageHandle(R, B, M, episode_length=5)
    for b, m in enumerate(maps):
        h.set_targets(m, env=b)
    h.set_rng([np.random.RandomState(60 + b) for b in range(B)])
    with pytest.raises(nat.GymFlockError) as e:  # no state, no done flags
        h.reset_device(None, 0.5, 0, done=True)
    assert e.value.code == nat.GF_ESTATE
    start = np.tile(np.arange(R, dtype=np.int32), (B, 1))
    visited = np.zeros((B, M - R), np.uint8)
    visited[0] = visited[2] = 1  # nothing left to visit: envs 0 and 2 finish early
    h.reset(start, visited)
    h.step(np.zeros((B, R), np.int32))
    np.testing.assert_array_equal(h.rewards()[1], [True, False, True, False])
    before = [_snapshot(h, b) for b in range(B)]
    n, s1, v1, _, _ = h.reset_device(None, 0.5, 6, done=True)
    assert n == 2
    np.testing.assert_array_equal(h.rewards()[1], [False] * B)
    for b in (1, 3):
        _assert_same(before[b], _snapshot(h, b), "env %d was not done" % b)
        assert not s1[b].any() and not v1[b].any()
    for b in (0, 2):
        rs = np.random.RandomState(60 + b)
        d = rn.reset_draws(rs, len(maps[b]), R, 0.5, 6, *_edges(maps[b]))
        np.testing.assert_array_equal(s1[b], d["start"])
        _assert_reset_state(h, b, maps[b], R, M, s1[b], v1[b], "done env %d" % b)
        _assert_stream(h, b, rs)
    before = [_snapshot(h, b) for b in range(B)]
    n, _, _, _, _ = h.reset_device(None, 0.5, 6, done=True)  # nothing is done: a no-op
    assert n == 0
    for b in range(B):
        _assert_same(before[b], _snapshot(h, b), "no-op env %d" % b)
    for _ in range(3):  # envs 1 and 3 reach episode_length = 5; envs 0 and 2 are at 4
        h.step(np.zeros((B, R), np.int32))
    np.testing.assert_array_equal(h.rewards()[1], [False, True, False, True])
    n, _, _, _, _ = h.reset_device(None, 0.5, 6, done=True)
    assert n == 2 and not h.rewards()[1].any()
    assert [int(h.obs(b)["step"][0, 0]) for b in range(B)] == [3, 0, 3, 0]
    h.close()


# ------------------------------------------------------------- 6. COV_RESET_NEW_MAPS
def test_new_maps_for_a_subset_generated(nat):
    """Coverage-v0's city maps (cov_generate_maps' kernels) through an arbitrary env list."""
    B, R, M = 4, 6, 1000
    h, twin = nat.CoverageHandle(R, B, M), nat.CoverageHandle(R, B, M)
    with pytest.raises(nat.GymFlockError) as e:  # no map streams yet
        h.reset_device(None, 0.5, 0, seed=1, new_maps=True)
    assert e.value.code == nat.GF_ESTATE
    n0, _, _ = h.generate_maps(map_seed=0)
    twin.generate_maps(map_seed=0)
    n1, _, _ = twin.generate_maps()  # every stream's second map
    first = [h.targets(b, n0[b]) for b in range(B)]
    h.reset_seeded(5, 0.5)
    mask = np.array([1, 0, 0, 1], bool)
    n, start, visited, _, _ = h.reset_device(mask, 0.5, 5 * R, new_maps=True)
    assert n == 2
    nt = h.n_targets()
    for b in range(B):
        if mask[b]:
            assert nt[b] == n1[b]
            np.testing.assert_array_equal(h.targets(b, nt[b]), twin.targets(b, n1[b]), err_msg="new map env %d" % b)
        else:
            assert nt[b] == n0[b]
            np.testing.assert_array_equal(h.targets(b, nt[b]), first[b], err_msg="kept map env %d" % b)
    assert not h.rewards()[1].any() and (start[mask] < nt[mask, None]).all()
    h.close()
    twin.close()


def test_new_maps_for_a_subset_sampled(nat, arl, grid, monkeypatch):
    """CoverageARL's sampler (cov_generate_submaps' kernel) through an arbitrary env list,
    and the greedy expert after it: the selected envs' time matrices are rebuilt, the others'
    actions are unchanged."""
    monkeypatch.setattr(oc, "RES", 5.0)
    B, R, M = 4, 4, 1000
    h, twin = nat.CoverageHandle(R, B, M, 50, 5.0), nat.CoverageHandle(R, B, M, 50, 5.0)
    h.load_occupancy(grid)
    twin.load_occupancy(grid)
    n0, _, _ = h.generate_submaps(map_seed=0)
    twin.generate_submaps(map_seed=0)
    n1, _, _ = twin.generate_submaps()
    first = [h.targets(b, n0[b]) for b in range(B)]
    second = [twin.targets(b, n1[b]) for b in range(B)]
    h.reset_seeded(9, 0.5)
    a0, rnd0 = h.controller_greedy()
    before = [_snapshot(h, b) for b in range(B)]
    mask = np.array([0, 1, 1, 0], bool)
    n, start, visited, region, status = h.reset_device(mask, 0.5, 5 * R, new_maps=True)
    assert n == 2 and (status == 0).all()
    a1, rnd1 = h.controller_greedy()
    nt = h.n_targets()
    for b in range(B):
        if not mask[b]:
            np.testing.assert_array_equal(h.targets(b, nt[b]), first[b])
            _assert_same(before[b], _snapshot(h, b), "unselected env %d" % b)
            np.testing.assert_array_equal(a1[b], a0[b])
            np.testing.assert_array_equal(rnd1[b], rnd0[b])
            continue
        m = second[b]
        assert nt[b] == n1[b]
        np.testing.assert_array_equal(h.targets(b, nt[b]), m)
        T = len(m)
        o = _assert_reset_state(h, b, m, R, M, start[b], visited[b], "new map env %d" % b, s=5.0)
        assert region[b, :T].sum() >= 5 * R and len(set(start[b].tolist())) == R
        assert region[b, start[b]].all()
        cost, prev = oc.time_matrix(T, o.motion[0] - R, o.motion[1] - R, horizon=10)
        cur = o.closest()
        recv = oc.action_receivers(cur, o.nbr, o.cnt, R)
        a, rnd = oc.greedy_actions(cost, prev, cur, o.visited[R:], recv, R)
        np.testing.assert_array_equal(rnd1[b], rnd)
        np.testing.assert_array_equal(a1[b][~rnd], np.asarray(a)[~rnd])
    # the map streams: the selected ones advanced by one map, the others where they were
    n2, _, _ = h.generate_submaps()
    n3, _, _ = twin.generate_submaps()
    for b in range(B):
        exp = twin.targets(b, n3[b]) if mask[b] else second[b]
        np.testing.assert_array_equal(h.targets(b, n2[b]), exp, err_msg="next map of env %d" % b)
    h.close()
    twin.close()


# ------------------------------------------------------------------- 7. a hidden handle
def test_hidden_handle_resets_discovered_for_the_selected_envs(nat):
    import test_coverage_explore_gpu as xg
    h, maps = xg._batch(nat)
    B, R, M = xg.B, xg.R, xg.M
    h.reset_seeded(11, 0.5)
    act = np.random.RandomState(5)
    for _ in range(4):
        h.step(act.randint(0, 4, size=(B, R)))
    before = [_snapshot(h, b, hidden=True) for b in range(B)]
    assert all(s["discovered"][R:].sum() > 0 for s in before)
    mask = np.array([1, 0, 1], bool)
    rss = [_rng_of(h, b) for b in range(B)]
    n, start, visited, region, status = h.reset_device(mask, 0.5, 2 * R)
    assert n == 2
    _assert_same(before[1], _snapshot(h, 1, hidden=True), "unselected hidden env")
    for b in (0, 2):
        d = rn.reset_draws(rss[b], len(maps[b]), R, 0.5, 2 * R, *_edges(maps[b]))
        np.testing.assert_array_equal(start[b], d["start"])
        np.testing.assert_array_equal(region[b, :len(maps[b])], d["region"])
        _assert_reset_state(h, b, maps[b], R, M, start[b], visited[b], "hidden env %d" % b)
        xg._check_env(h, b, en.initial_discovered(M, R), maps[b], "reset_device env %d" % b)
    a = act.randint(0, 4, size=(B, R))
    disc = [h.discovered(b) for b in range(B)]
    h.step(a)
    for b in range(B):
        xg._check_env(h, b, disc[b], maps[b], "step after reset_device env %d" % b)
    h.close()


# -------------------------------------------------------------------- 8. the drop-in env
def test_explore_env_device_reset_replays_the_reference(grid):
    import gym_flock
    import test_coverage_explore_gpu as xg
    f = np.load(os.path.join(GOLDEN, "coverage_explore.npz"))
    pre = "g_"
    map_seed, env_seed = int(f[pre + "map_seed"]), int(f[pre + "env_seed"])
    np.random.seed(map_seed)
    env = gym_flock.make("ExploreEnv-v0", occupancy=grid, reset_mode="device")
    env.seed(env_seed)
    held = env.np_random  # callers holding the RandomState see it continue
    np.random.seed(map_seed)
    obs = env.reset()
    assert env.np_random is held
    assert env.n_targets == int(f[pre + "n_targets"])
    np.testing.assert_array_equal(np.array(env.start_region), f[pre + "start_region"])
    np.testing.assert_array_equal(env.x, f[pre + "x0"])
    xg._assert_obs(obs, f, pre, "reset", None, env)
    n = len(f[pre + "reward"])
    for t in range(n):
        a = env.controller(random=False, greedy=True)
        np.testing.assert_array_equal(a.flatten(), f[pre + "actions"][t], err_msg="greedy actions, step %d" % t)
        obs, r, d, _ = env.step(a)
        assert r == f[pre + "reward"][t] and d == f[pre + "done"][t], (t, r, d)
        xg._assert_obs(obs, f, pre, "step %d" % t, t, env)
        np.testing.assert_array_equal(env.closest_targets, f[pre + "closest"][t])
    assert d
    np.testing.assert_array_equal(env.visited[:, 0], f[pre + "visited"][-1])
    assert env.np_random.uniform() == f[pre + "probe"]
    env.close()


def test_arl_env_device_reset_gives_the_recorded_reset(arl, grid):
    from gym_flock.envs.spatial import CoverageARLEnv
    f, pre = arl, "g_"
    map_seed, env_seed = int(f[pre + "map_seed"]), int(f[pre + "env_seed"])
    np.random.seed(map_seed)
    env = CoverageARLEnv(occupancy=grid, reset_mode="device")
    ref = CoverageARLEnv(occupancy=grid)  # the default mode on the same seeds
    env.seed(env_seed)
    np.random.seed(map_seed)
    obs = env.reset()
    R = int(f[pre + "n_robots"])
    np.testing.assert_array_equal(env.x[R:], f[pre + "targets"])
    np.testing.assert_array_equal(np.array(env.start_region), f[pre + "start_region"])
    np.testing.assert_array_equal(env.x, f[pre + "x0"])
    np.testing.assert_array_equal(env.visited[:, 0], f[pre + "visited0"])
    for k in OBS_KEYS:
        np.testing.assert_array_equal(np.asarray(obs[k]).reshape(f[pre + k + "0"].shape), f[pre + k + "0"], err_msg=k)
    ref.seed(env_seed)
    np.random.seed(map_seed)
    ref.reset()
    assert env.np_random.get_state()[2] == ref.np_random.get_state()[2]
    np.testing.assert_array_equal(env.np_random.get_state()[1], ref.np_random.get_state()[1])
    env.close()
    ref.close()


# --------------------------------------------------------------------- VecCoverage
def test_vec_coverage_reset_envs(nat):
    from gym_flock.vec import VecCoverage
    R, M, B = 3, 40, 5
    maps = [_grid_map(n) for n in (20, 33, 37, 16, 28)]
    v = VecCoverage(B, R, max_nodes=M, nearby_starts=True)
    for b, m in enumerate(maps):
        v.set_targets(m, env=b)
    v.reset(seed=3)
    for _ in range(2):
        v.step(np.ones((B, R), np.int32))
    rss = [v.np_random(b) for b in range(B)]
    before = [v.obs(b) for b in range(B)]
    n, start, visited, status = v.reset_envs([1, 3])
    assert n == 2 and (status == 0).all()
    for b in range(B):
        if b in (1, 3):
            d = rn.reset_draws(rss[b], len(maps[b]), R, 0.5, 5 * R, *_edges(maps[b]))
            np.testing.assert_array_equal(start[b], d["start"])
            np.testing.assert_array_equal(visited[b, :len(maps[b])], d["visited"])
            assert v.np_random(b).get_state()[2] == rss[b].get_state()[2]
        else:
            for k in OBS_KEYS:
                np.testing.assert_array_equal(v.obs(b)[k], before[b][k])
    m = np.zeros(B, bool)
    m[4] = True
    n, start, _, _ = v.reset_envs(m, nearby=0, seed=50)
    exp = np.random.RandomState(54).choice(np.arange(28), size=(R,), replace=False)
    assert n == 1
    np.testing.assert_array_equal(start[4], exp)
    n, _, _, _ = v.reset_envs("done")
    assert n == int(v.rewards()[1].sum()) == 0
    v.close()
