"""cov_explore_expert on the GPU: whole expert rollouts of envs that hide nodes in one launch,
against the NumPy restatement of the loop (tests/coverage_explore_rollout_numpy.py), against a
twin handle stepped through the host-paced route (cov_controller_greedy, the fallback draws
on the host, cov_set_actions, the resident step with its hidden pass), and against the
reference's recorded ExploreEnv episode. Every comparison is exact: the values are flags,
indices, counts, stream words, or float32 features that both sides compute the same way."""
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import GOLDEN

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import coverage_explore_numpy as en  # noqa: E402
import coverage_explore_rollout_numpy as xr  # noqa: E402

pytestmark = pytest.mark.gpu

RECORDS = ("rewards", "done", "actions", "needs_random", "flat_obs")


@pytest.fixture(scope="module")
def nat():
    from gym_flock import _native
    return _native


# ------------------------------------------------------------------ the batch of three maps
def _maps():
    """A 4 x 5 grid, a ring with a chord, two blobs joined by a bridge (the maps of
    test_coverage_explore_gpu.py): 20, 34 and 27 targets, every degree in 1..4."""
    s = 5.5
    gx, gy = np.meshgrid(np.arange(4) * s, np.arange(5) * s, indexing="ij")
    grid_map = np.stack([gx.ravel(), gy.ravel()], axis=1)
    n_ring, n_chord = 26, 8
    r = s / (2.0 * np.sin(np.pi / n_ring))
    ang = 2.0 * np.pi * np.arange(n_ring) / n_ring
    ring = np.stack([r * np.cos(ang), r * np.sin(ang)], axis=1)
    chord = np.stack([np.linspace(r, -r, n_chord + 2)[1:-1], np.zeros(n_chord)], axis=1)
    ring_map = np.vstack([ring, chord])
    bx, by = np.meshgrid(np.arange(3) * s, np.arange(3) * s, indexing="ij")
    blob = np.stack([bx.ravel(), by.ravel()], axis=1)
    bridge = np.stack([2 * s + (1 + np.arange(9)) * s, np.full(9, s)], axis=1)
    blobs_map = np.vstack([blob, bridge, blob + np.array([12 * s, 0.0])])
    maps = [grid_map, ring_map, blobs_map]
    assert [len(m) for m in maps] == [20, 34, 27]
    return maps


B, R, M = 3, 3, 37
N = 12


def _rng_at(seed, pos=None):
    rs = np.random.RandomState(seed)
    if pos is not None:
        st = rs.get_state()
        rs.set_state((st[0], st[1], pos))
    return rs


def _handle(nat, kind, streams=0, pos=None):
    """The batch on a new handle and its restatement, at the same state.
    kind "seeded": reset_seeded(11, 0.5), the streams continuing from the reset's draws.
    kind "placed": an explicit start with env 2's robots in one blob and its only unvisited
    targets at the bridge's far end, out of sight (the expert gives up for every robot, every
    step), env 0's robots then placed on other nodes (its first step recomputes their nodes),
    and the streams RandomState(40 + b), at position `pos` when given."""
    maps = _maps()
    h = nat.CoverageHandle(R, B, M, 75, 5.5)
    h.set_hidden(True)
    for b, m in enumerate(maps):
        h.set_targets(m, env=b)
    h.set_streams(streams)
    envs = [xr.ExploreRollout(m, R, M) for m in maps]
    if kind == "seeded":
        start, visited = h.reset_seeded(11, 0.5)
        keys, p = h.get_rng()
        rngs = []
        for b in range(B):
            rs = np.random.RandomState()
            rs.set_state(("MT19937", keys[b], int(p[b])))
            rngs.append(rs)
    else:
        start = np.array([[13, 18, 19], [3, 12, 20], [0, 1, 3]], np.int32)
        visited = np.zeros((B, M - R), np.uint8)
        visited[:, 5::3] = 1
        visited[2] = 1
        visited[2, [15, 16, 17]] = 0
        h.reset(start, visited)
        rngs = [_rng_at(40 + b, pos) for b in range(B)]
        h.set_rng(rngs)
        rngs = [_rng_at(40 + b, pos) for b in range(B)]  # the restatement's own copies
        h.set_robot_positions(0, maps[0][[1, 19, 15]])
    for b, e in enumerate(envs):
        e.reset(start[b], visited[b], rngs[b])
    if kind == "placed":
        envs[0].o.xr[:] = maps[0][[1, 19, 15]]
    return h, envs


_REF = {}


def _restated(nat, kind, pos=None, n=N):
    """The restatement's records of n steps from a start, computed once per module."""
    key = (kind, pos, n)
    if key not in _REF:
        h, envs = _handle(nat, kind, 0, pos)
        h.close()
        out = xr.rollout(envs, n)
        out["rng"] = [e.rng.get_state() for e in envs]
        out["disc"] = [e.disc.copy() for e in envs]
        out["visited"] = [e.visited() for e in envs]
        _REF[key] = out
    return _REF[key]


def _assert_records(got, ref, msg=""):
    for k in ("rewards", "actions", "flat_obs"):
        np.testing.assert_array_equal(got[k], ref[k], err_msg=k + msg)
    for k in ("done", "needs_random"):
        np.testing.assert_array_equal(got[k].astype(bool), ref[k], err_msg=k + msg)


def _twin_steps(twin, n):
    """n expert steps through the host-paced route; the streams move to the host. Returns the
    records and the host streams."""
    keys, pos = twin.get_rng()
    rngs = []
    for b in range(B):
        rs = np.random.RandomState()
        rs.set_state(("MT19937", keys[b], int(pos[b])))
        rngs.append(rs)
    sh = twin.rollout_shapes(n)
    out = {k: np.zeros(*sh[k]) for k in RECORDS}
    for t in range(n):
        a, rnd = twin.controller_greedy()
        for b in np.nonzero(rnd.any(axis=1))[0]:
            k = np.nonzero(rnd[b])[0]
            a[b, k] = rngs[b].choice(4, size=len(k))
        twin.set_actions(a)
        twin.sync()
        twin.step(resident=True)
        out["actions"][t], out["needs_random"][t] = a, rnd
        out["rewards"][t], out["done"][t] = twin.rewards()
        out["flat_obs"][t] = twin.flat_obs(f32=True)
    return out, rngs


def _state(h):
    """Every getter of the handle, as one dict of arrays."""
    s = {"flat32": h.flat_obs(f32=True), "flat64": h.flat_obs(), "rewards": h.rewards()[0], "done": h.rewards()[1],
         "actions": h.actions()[0], "needs_random": h.actions()[1]}
    for k, v in h.graphs_tuple().items():
        s["gt_" + k] = np.asarray(v)
    for b in range(B):
        for k, v in h.obs(b).items():
            s["obs%d_%s" % (b, k)] = v
        for k, v in h.hidden_obs(b).items():
            s["hid%d_%s" % (b, k)] = v
        s["disc%d" % b], s["vis%d" % b] = h.discovered(b), h.visited(b)
        s["xr%d" % b], s["cur%d" % b] = h.robots(b)
    return s


def _assert_same_state(a, b, msg=""):
    sa, sb = _state(a), _state(b)
    assert sa.keys() == sb.keys()
    for k in sa:
        np.testing.assert_array_equal(sa[k], sb[k], err_msg=k + msg)


@pytest.mark.parametrize("streams", [0, 2])
@pytest.mark.parametrize("kind", ["seeded", "placed"])
def test_batch_against_the_restatement_and_the_host_paced_twin(nat, kind, streams):
    """12 fused steps, recorded at every step, against (a) the restatement and (b) a twin
    handle stepped 12 times through the host-paced route: every step's rewards, done, actions,
    needs_random and flat row, then every getter, the streams, and what later calls make of
    the state.

    The "seeded" start is reset_seeded(11, 0.5). On it env 2's expert gives up for every robot
    at step 11, but in the restatement no pick of its 12 steps (nor of 40) differs from the
    unmasked greedy's: on maps this small every nearest unvisited target is already in sight.
    So that the mask demonstrably matters, the same checks also run from the "placed" start,
    where env 2 draws for every robot at every step while the unmasked expert would head for
    the far blob, and where env 0's robots were placed externally before the call."""
    ref = _restated(nat, kind)
    assert ref["needs_random"][:, 2].all(axis=1).any()  # env 2 drew for every robot at some step
    if kind == "placed":
        assert ref["differs"].any() and ref["needs_random"][:, 2].all()
    h, _ = _handle(nat, kind, streams)
    twin, _ = _handle(nat, kind, streams)
    got = h.explore_expert(N, RECORDS, every=1)
    _assert_records(got, ref, " vs the restatement")
    exp, rngs = _twin_steps(twin, N)
    _assert_records(got, exp, " vs the twin")
    keys, pos = h.get_rng()
    for b in range(B):
        for st in (rngs[b].get_state(), ref["rng"][b]):
            np.testing.assert_array_equal(keys[b], st[1])
            assert int(pos[b]) == st[2]
        np.testing.assert_array_equal(h.discovered(b), ref["disc"][b])
        np.testing.assert_array_equal(h.visited(b)[:len(ref["visited"][b])], ref["visited"][b])
    _assert_same_state(h, twin, " after the rollout")
    # later calls: the masked controller, a plain step, a device reset of two envs
    for x in (h, twin):
        x.set_rng(rngs)
    a1, r1 = h.controller_greedy()
    a2, r2 = twin.controller_greedy()
    np.testing.assert_array_equal(a1, a2)
    np.testing.assert_array_equal(r1, r2)
    a = np.random.RandomState(3).randint(0, 4, size=(B, R))
    for x in (h, twin):
        x.step(a)
    _assert_same_state(h, twin, " after a plain step")
    mask = np.array([1, 0, 1], np.uint8)
    o1, o2 = h.reset_device(mask, 0.5), twin.reset_device(mask, 0.5)
    for u, v in zip(o1, o2):
        np.testing.assert_array_equal(u, v)
    _assert_same_state(h, twin, " after reset_device")
    h.close()
    twin.close()


def test_chunks_and_stride(nat):
    ref = _restated(nat, "placed")
    h1, _ = _handle(nat, "placed")
    full = h1.explore_expert(N, RECORDS, every=1)
    _assert_records(full, ref)
    # three chunks of 4
    h2, _ = _handle(nat, "placed")
    parts = [h2.explore_expert(4, RECORDS) for _ in range(3)]
    for k in RECORDS:
        np.testing.assert_array_equal(np.concatenate([p[k] for p in parts]), full[k], err_msg=k)
    _assert_same_state(h1, h2, " (three chunks)")
    # every third row, nothing else fetched; then nothing recorded at all
    h3, _ = _handle(nat, "placed")
    strided = h3.explore_expert(N, ("flat_obs",), every=3)
    assert set(strided) == {"flat_obs"} and strided["flat_obs"].shape == (4, B, 16 * M + 1)
    np.testing.assert_array_equal(strided["flat_obs"], full["flat_obs"][[2, 5, 8, 11]])
    _assert_same_state(h1, h3, " (every=3)")
    h4, _ = _handle(nat, "placed")
    assert h4.explore_expert(N, fetch=False) is None
    _assert_same_state(h1, h4, " (unrecorded)")
    for x in (h1, h2, h3, h4):
        x.close()


_TORCH_CHILD = """
import sys
import numpy as np
import torch
assert torch.cuda.is_available()
sys.path[:0] = [{root!r}, {pkg!r}, {tests!r}]
import test_coverage_explore_rollout_gpu as T
from gym_flock import _native as nat
h1, _ = T._handle(nat, "placed")
host = h1.explore_expert(T.N, T.RECORDS, every=3)
h2, _ = T._handle(nat, "placed")
tdt = {{np.float64: torch.float64, np.uint8: torch.uint8, np.int32: torch.int32, np.float32: torch.float32}}
dev = {{k: torch.full(s, 77, dtype=tdt[d], device="cuda") for k, (s, d) in h2.rollout_shapes(T.N, 3).items()}}
torch.cuda.synchronize()
assert h2.explore_expert(T.N, every=3, device_ptrs={{k: v.data_ptr() for k, v in dev.items()}}) is None
h2.sync()
for k in T.RECORDS:
    np.testing.assert_array_equal(dev[k].cpu().numpy(), host[k], err_msg=k)
T._assert_same_state(h1, h2, " (device destinations)")
assert host["flat_obs"].shape == (4, T.B, 16 * T.M + 1) and host["actions"].shape == (T.N, T.B, T.R)
print("ok")
"""


def test_device_destinations_equal_host_destinations():
    """Records written straight into torch tensors (data_ptr(), COV_ROLLOUT_DEVICE) equal the
    host records, and the handle ends in the same state. torch is imported before gym_flock
     in a child process: this one stays torch-free."""
    here = os.path.dirname(os.path.abspath(__file__))
    root = os.path.dirname(here)
    code = _TORCH_CHILD.format(root=root, pkg=os.path.join(root, "gym-flock_amd"), tests=here)
    p = subprocess.run([sys.executable, "-c", code], capture_output=True, timeout=240)
    assert p.returncode == 0, p.stderr.decode()[-3000:]
    assert p.stdout.decode().strip().endswith("ok")


def test_list_pick_direct_pick_and_the_switch(nat):
    """One env on a 10 x 10 lattice, two robots from opposite corners, nothing visited: the
    targets the expert may head for (T minus the masked ones) number 32 at the first step (the
    direct pick from the candidate list), grow past 32 as the robots discover the lattice (the
    greedy lists) and fall to 32 and below again as they visit it."""
    s, n = 5.5, 44
    gx, gy = np.meshgrid(np.arange(10) * s, np.arange(10) * s, indexing="ij")
    lat = np.stack([gx.ravel(), gy.ravel()], axis=1)
    Rl, Ml = 2, 102
    env = xr.ExploreRollout(lat, Rl, Ml)
    start, visited = np.array([[0, 99]], np.int32), np.zeros((1, Ml - Rl), np.uint8)
    env.reset(start[0], visited[0], _rng_at(5))
    ref = xr.rollout([env], n)
    left = ref["left"][:, 0]
    assert left[0] <= 32 and left.max() > 32 and left[-1] <= 32 and (np.diff((left > 32).astype(int)) != 0).sum() == 2
    h = nat.CoverageHandle(Rl, 1, Ml, 75, 5.5)
    h.set_hidden(True)
    h.set_targets(lat, env=0)
    h.reset(start, visited)
    h.set_rng([_rng_at(5)])
    got = h.explore_expert(n, RECORDS)
    _assert_records(got, ref)
    np.testing.assert_array_equal(h.discovered(0), env.disc)
    np.testing.assert_array_equal(h.visited(0), env.visited())
    h.close()


def test_more_robots_than_threads(nat):
    """260 robots on a 20 x 20 lattice: more robots than the workgroup has threads, so the
    step takes its looped robot passes and the workgroup-wide claim rounds, robots block each
    other, and from the third step on hundreds of robots draw per step (the key is regenerated
    inside the rollout)."""
    s, n = 5.5, 6
    gx, gy = np.meshgrid(np.arange(20) * s, np.arange(20) * s, indexing="ij")
    lat = np.stack([gx.ravel(), gy.ravel()], axis=1)
    Rl, Ml = 260, 920  # 1,520 motion edges and 8 * 260 action edges fit the 4 * 920 slots
    rs = np.random.RandomState(1)
    start = rs.choice(400, Rl, replace=False).astype(np.int32)[None]
    visited = np.ones((1, Ml - Rl), np.uint8)
    visited[0, rs.choice(400, 150, replace=False)] = 0
    env = xr.ExploreRollout(lat, Rl, Ml)
    env.reset(start[0], visited[0], _rng_at(2))
    ref = xr.rollout([env], n)
    assert ref["needs_random"][-1].all() and 0 < ref["needs_random"][2].sum() < Rl
    h = nat.CoverageHandle(Rl, 1, Ml, 75, 5.5)
    h.set_hidden(True)
    h.set_targets(lat, env=0)
    h.reset(start, visited)
    h.set_rng([_rng_at(2)])
    got = h.explore_expert(n, RECORDS)
    _assert_records(got, ref)
    keys, pos = h.get_rng()
    st = env.rng.get_state()
    np.testing.assert_array_equal(keys[0], st[1])
    assert int(pos[0]) == st[2]
    np.testing.assert_array_equal(h.discovered(0), env.disc)
    np.testing.assert_array_equal(h.visited(0)[:400], env.visited())
    np.testing.assert_array_equal(h.robots(0)[1], env.o.closest())
    h.close()


def _line(n, spacing=5.0):
    return np.stack([np.arange(n) * spacing, np.zeros(n)], axis=1)


def _check_env(h, b, disc, targets, msg=""):
    """Env b's hidden observation equals the restatement applied to its unhidden one and to
    the discovered set `disc` from before this observation. Returns the set after it."""
    o = h.obs(b)
    pos, _ = h.robots(b)
    d, nodes, snd = en.hidden_obs(disc, o["nodes"], o["senders"], o["receivers"], pos, targets)
    got = h.hidden_obs(b)
    np.testing.assert_array_equal(got["nodes"], nodes, err_msg="nodes " + msg)
    np.testing.assert_array_equal(got["senders"], snd, err_msg="senders " + msg)
    np.testing.assert_array_equal(h.discovered(b), d, err_msg="discovered " + msg)
    for k in ("edges", "receivers", "step"):
        np.testing.assert_array_equal(got[k], o[k], err_msg=k + " " + msg)
    return d


@pytest.mark.parametrize("max_nodes", [33, 65, 66])
def test_bit_word_edges_on_a_line(nat, max_nodes):
    """One robot on a line that fills the handle (T = max_nodes - 1): the last node's bit ends
    on or just past a 32- or 64-bit word of the discovered, mask and claim bits. Everything
    left of the robot is visited, so the expert walks right, towards the last target, which
    comes into sight on the way. After each fused step the hidden observation follows from the
    step before (the expectations of the line walks in test_coverage_explore_gpu.py)."""
    T, start = max_nodes - 1, max_nodes - 1 - 8
    targets = _line(T)
    h = nat.CoverageHandle(1, 1, max_nodes, 50, 5.0)
    h.set_hidden(True)
    h.set_targets(targets, env=0)
    visited = np.zeros((1, T), np.uint8)
    visited[0, :start] = 1
    h.reset(np.array([[start]], np.int32), visited)
    h.set_rng([_rng_at(0)])
    d = _check_env(h, 0, en.initial_discovered(max_nodes, 1), targets, "reset")
    assert d[1 + T - 1] == 0  # the last target is not in sight yet
    for t in range(6):
        out = h.explore_expert(1, ("actions", "needs_random", "rewards"))
        assert out["actions"][0, 0, 0] == 1 and not out["needs_random"].any() and out["rewards"][0, 0] == 1
        assert h.robots(0)[1][0] == 1 + start + 1 + t
        d = _check_env(h, 0, d, targets, "step %d" % t)
    assert d[1 + start - 4:].all() and h.visited(0)[start:start + 7].all() and not h.visited(0)[start + 7:].any()
    h.close()


def test_key_regeneration_inside_a_rollout(nat):
    """Every stream at position 620: env 2 draws three words per step, so its second step
    takes words 623, 624 and 625, the last two from the regenerated key; env 0 draws two words
    at the first step and three from step 8 on."""
    ref = _restated(nat, "placed", pos=620)
    assert ref["needs_random"][:2, 2].all() and ref["rng"][2][2] == (620 + 3 * N) % 624
    h, _ = _handle(nat, "placed", pos=620)
    got = h.explore_expert(N, RECORDS)
    _assert_records(got, ref)
    keys, pos = h.get_rng()
    for b in range(B):
        np.testing.assert_array_equal(keys[b], ref["rng"][b][1])
        assert int(pos[b]) == ref["rng"][b][2]
    assert not np.array_equal(keys[2], _rng_at(42).get_state()[1])  # the key was regenerated
    h.close()


def test_the_reference_episode_in_one_launch():
    import gym_flock
    f = np.load(os.path.join(GOLDEN, "coverage_explore.npz"))
    grid = np.load(os.path.join(GOLDEN, "grid_slice10.npy"))
    pre = "g_"
    map_seed, env_seed = int(f[pre + "map_seed"]), int(f[pre + "env_seed"])
    np.random.seed(map_seed)
    env = gym_flock.make("ExploreEnv-v0", occupancy=grid)
    env.seed(env_seed)
    np.random.seed(map_seed)
    env.reset()
    Rr, T = int(f[pre + "n_robots"]), int(f[pre + "n_targets"])
    np.testing.assert_array_equal(env.x, f[pre + "x0"])
    h = env._h
    h.set_rng([env.np_random])
    n = len(f[pre + "reward"])
    out = h.explore_expert(n, ("rewards", "done", "actions", "needs_random"))
    np.testing.assert_array_equal(out["actions"][:, 0], f[pre + "actions"])
    np.testing.assert_array_equal(out["rewards"][:, 0], f[pre + "reward"])
    np.testing.assert_array_equal(out["done"][:, 0].astype(bool), f[pre + "done"])
    assert out["needs_random"].sum() == 14
    np.testing.assert_array_equal(h.discovered(0), f[pre + "discovered"][-1])
    np.testing.assert_array_equal(h.visited(0)[:T], f[pre + "visited"][-1][Rr:])
    np.testing.assert_array_equal(h.robots(0)[1], f[pre + "closest"][-1])
    obs = h.hidden_obs(0)
    for k in ("nodes", "edges", "senders", "receivers", "step"):
        rec = f[pre + k][-1]
        np.testing.assert_array_equal(np.asarray(obs[k]).reshape(rec.shape), rec, err_msg=k)
    keys, pos = h.get_rng()
    rs = np.random.RandomState()
    rs.set_state(("MT19937", keys[0], int(pos[0])))
    assert rs.uniform() == f[pre + "probe"]
    env.close()


def _small(nat, max_nodes, n_robots=1, hidden=True, rng=True):
    """A reset handle on a 12-target line (res 5.0)."""
    h = nat.CoverageHandle(n_robots, 1, max_nodes, 50, 5.0)
    if hidden:
        h.set_hidden(True)
    h.set_targets(_line(12), env=0)
    h.reset(np.arange(1, 1 + n_robots, dtype=np.int32)[None], np.zeros((1, max_nodes - n_robots), np.uint8))
    if rng:
        h.set_rng([_rng_at(0)])
    return h


def test_refusals_launch_nothing(nat):
    def refused(h, code, n_steps=1, every=1, flags=0, word=None):
        before = h.flat_obs(f32=True)
        rec = nat.CovRollout()
        rec.record_every, rec.flags = every, flags
        assert h.lib.cov_explore_expert(h.h, n_steps, rec) == code
        if word:
            assert word in h.lib.fe_last_error()
        np.testing.assert_array_equal(h.flat_obs(f32=True), before)
        h.close()

    refused(_small(nat, 16, hidden=False), nat.GF_ESTATE, word=b"hide")
    refused(_small(nat, 16, rng=False), nat.GF_ESTATE, word=b"streams")
    refused(_small(nat, 16), nat.GF_EINVAL, n_steps=0)
    refused(_small(nat, 16), nat.GF_EINVAL, n_steps=12, every=5)
    refused(_small(nat, 16), nat.GF_EINVAL, n_steps=12, every=0)
    refused(_small(nat, 16), nat.GF_EINVAL, flags=2)
    refused(_small(nat, 1026), nat.GF_EINVAL, word=b"1024")
    # the LDS guard: the smallest max_nodes whose layout passes 64 KB, from the function that
    # the guard and the launcher share
    lib = nat.load()
    m = 1026
    while lib.cov_explore_lds_bytes(2, m) <= 64 * 1024:
        m += 1
    refused(_small(nat, m, n_robots=2), nat.GF_EINVAL, word=b"LDS")
    # not set up at all: no reset yet
    h = nat.CoverageHandle(1, 1, 16, 50, 5.0)
    h.set_hidden(True)
    h.set_targets(_line(12), env=0)
    assert h.lib.cov_explore_expert(h.h, 1, None) == nat.GF_ESTATE
    h.close()
    # and the call that is not refused, on the same small handle
    h = _small(nat, 16)
    out = h.explore_expert(2, ("rewards",))
    assert out["rewards"].shape == (2, 1)
    h.close()


def test_vec_coverage_routes_the_hidden_expert_through_the_fused_call(nat):
    """VecCoverage.step(greedy=True) on a hidden batch with device streams is the fused call
    with n_steps = 1, bit-identical to the host-paced route (a twin whose predicate is
    switched off); explore_expert_steps records and raises where it cannot run."""
    from gym_flock.vec import VecCoverage
    vs = []
    for _ in range(3):
        v = VecCoverage(B, R, max_nodes=M, hide_nodes=True)
        for b, m in enumerate(_maps()):
            v.set_targets(m, env=b)
        v.reset(seed=3)
        vs.append(v)
    fused, host, roll = vs
    assert fused._explore_fused() and not fused._device_draws()
    host._explore_fused = lambda: False
    for _ in range(6):
        fused.step(greedy=True)
        host.step(greedy=True)
    _assert_same_state(fused.h, host.h, " step(greedy=True)")
    out = roll.explore_expert_steps(6, record=("rewards", "done", "actions"))
    assert out["done"].dtype == bool and out["actions"].shape == (6, B, R)
    _assert_same_state(fused.h, roll.h, " explore_expert_steps")
    kf, pf = fused.h.get_rng()
    for b in range(B):
        st = host.np_random(b).get_state()
        np.testing.assert_array_equal(kf[b], st[1])
        assert int(pf[b]) == st[2]
    del host._explore_fused
    host._host_rngs()  # the streams move to the host (as a host-drawn fallback moves them)
    assert not host._explore_fused()
    with pytest.raises(RuntimeError, match="streams"):
        host.explore_expert_steps(2)
    plain = VecCoverage(1, 1, max_nodes=16)
    with pytest.raises(RuntimeError, match="hide"):
        plain.explore_expert_steps(2)
    for v in vs + [plain]:
        v.close()
