"""The variant step (flock_step_kernel<..., VAR=true>, load_state_variant, the obstacle
and clip branches of step_epilogue, fe_set_variant / fe_set_dt and the variant block of
base_args / env_range) against oracle.flocking_variants: every switch alone, the
registered combinations with constants float32 cannot represent, prefixes at and past
their edges, a batched rollout with a new per-env dt every step and a closed loop, the
split and de-phased launch forms, and Flocking-v0's observation. Needs an MI355X.

Tolerances are those of tests/test_flock_gpu.py: state, adjacency and kNN indices
bit-exact, network exactly float32(1/deg) on set bits, state_values rtol 1e-5 atol 1e-9,
controller rtol 1e-9 atol 1e-12, reward rtol 1e-12. Where a case holds NaN by
construction the NaN masks must be equal and the tolerance applies to the other entries."""
import os

import numpy as np
import pytest

from conftest import GOLDEN
from oracle import flocking as fo
from oracle import flocking_variants as fv

pytestmark = pytest.mark.gpu

nat = pytest.importorskip("gym_flock._native")
from gym_flock.envs import flocking as envs  # noqa: E402
from gym_flock.vec import VARIANTS, VecFlockingRelative  # noqa: E402

WORST = {}  # quantity -> largest |ours - ref| / (atol + rtol |ref|) seen (1 = at the tolerance)


@pytest.fixture(scope="module", autouse=True)
def _report_worst():
    yield
    print("\nvariant matrix, largest error / tolerance:", {k: float("%.3g" % v) for k, v in sorted(WORST.items())})


def close(name, ours, ref, rtol, atol):
    """Equal NaN masks; rtol / atol on the other entries (infinities must be equal)."""
    ours, ref = np.asarray(ours, np.float64), np.asarray(ref, np.float64)
    np.testing.assert_array_equal(np.isnan(ours), np.isnan(ref), err_msg=name + " NaN mask")
    ok = np.isfinite(ref) & np.isfinite(ours)
    if ok.any():
        ratio = np.abs(ours[ok] - ref[ok]) / (atol + rtol * np.abs(ref[ok]))
        WORST[name] = max(WORST.get(name, 0.0), float(ratio.max()))
    ok = ~np.isnan(ref)
    np.testing.assert_allclose(ours[ok], ref[ok], rtol=rtol, atol=atol, err_msg=name)


def same_bits(ours, ref, what="state"):
    """Bit-exact float64 (the sign of zero included); NaN where the reference has NaN."""
    ours, ref = np.ascontiguousarray(ours, np.float64), np.ascontiguousarray(ref, np.float64)
    np.testing.assert_array_equal(np.isnan(ours), np.isnan(ref), err_msg=what + " NaN mask")
    ok = ~np.isnan(ref)
    np.testing.assert_array_equal(ours.view(np.uint64)[ok], ref.view(np.uint64)[ok], err_msg=what)


def oracle_step(x, u, dt, var, action_scalar=10.0):
    """One step of a variant given as fe_variant fields (None: only the per-env dt)."""
    var = var or {}
    with np.errstate(all="ignore"):
        return fv.integrate(x, u, dt, var.get("u_scale", action_scalar), var.get("n_frozen", 0),
                            var.get("u_clip") or None, var.get("x_scale"))


def check_env(v, b, x1, var, ctrl=True, ctrl_centralized=True):
    """Every output of env b of the last step against the oracle on the oracle's state x1."""
    var = var or {}
    nz, cc = var.get("n_vel_zero", 0), var.get("ctrl_clip") or None
    same_bits(v.h.get_state(b), x1)
    with np.errstate(all="ignore"):
        sv, net, adj, deg = fv.helpers(x1, n_vel_zero=nz)
        rew = fo.reward(x1)
        want_c = fv.controller(x1, centralized=ctrl_centralized, n_vel_zero=nz, clip=cc) if ctrl else None
        sv32 = sv.astype(np.float32)
    got = v.network(b)
    np.testing.assert_array_equal(got > 0, adj)
    np.testing.assert_array_equal(got, net.astype(np.float32))  # float32(1/deg) on set bits, else 0
    got = v.state_values(b)
    np.testing.assert_array_equal(np.isnan(got), np.isnan(sv32))
    close("state_values", got, np.where(np.isnan(sv32), np.nan, sv), 1e-5, 1e-9)
    close("reward", v.rewards()[b], rew, 1e-12, 0.0)
    if ctrl:
        close("controller", v.controls(b), want_c, 1e-9, 1e-12)


def check_decentralized(v, xs, var):
    var = var or {}
    dec = v.controller(centralized=False)
    for b, x1 in enumerate(xs):
        with np.errstate(all="ignore"):
            want = fv.controller(x1, centralized=False, n_vel_zero=var.get("n_vel_zero", 0),
                                 clip=var.get("ctrl_clip") or None)
        close("controller", dec[b], want, 1e-9, 1e-12)


def states(B, n, seed0):
    return np.stack([fo.synthetic_state(n, seed0 + b) for b in range(B)])


def actions(rs, B, n, f64, scale=1.0):
    u = rs.uniform(-scale, scale, size=(B, n, 2))
    return u if f64 else u.astype(np.float32)


# ------------------------------------------------------------------ a. one switch at a time
SINGLE = {
    "u_scale_1": dict(u_scale=1.0),
    "u_scale_0.3": dict(u_scale=0.3),
    "n_frozen_5": dict(n_frozen=5),
    "n_vel_zero_5": dict(n_vel_zero=5),
    "u_clip_0.1": dict(u_clip=0.1),
    "x_scale_0.7": dict(x_scale=0.7),
    "x_scale_-2": dict(x_scale=-2.0),
    "ctrl_clip_0.1": dict(ctrl_clip=0.1),
    "dt_only": None,  # no fe_variant at all: u_scale falls back to action_scalar, x_scale to 1
}


@pytest.mark.parametrize("n", [97, 513])
@pytest.mark.parametrize("case", sorted(SINGLE))
def test_single_switch_vs_oracle(case, n):
    """One fe_variant field set and every other left at its default (set_variant's
    u_scale default is action_scalar), or no fe_variant and a per-env dt; N = 97 has one
    LDS tile and a ragged last adjacency word, N = 513 a second tile of one agent."""
    B = 3
    var = SINGLE[case]
    for f64 in (False, True):
        v = VecFlockingRelative(B, n, variant=var)
        x0 = states(B, n, 1100 + n)
        v.reset(x=x0)
        rs = np.random.RandomState(n + 2 * len(case) + f64)
        u = actions(rs, B, n, f64)
        dt = rs.normal(0.12, 0.018, size=B) if var is None else None
        v.step(u, controller=True, dt=dt)
        xs = [oracle_step(x0[b], u[b], 0.01 if dt is None else dt[b], var) for b in range(B)]
        for b in range(B):
            check_env(v, b, xs[b], var)
        check_decentralized(v, xs, var)
        v.close()


# ------------------------------------------- b. registered combinations, inexact constants
INEXACT = dict(u_clip=0.1, ctrl_clip=0.1, u_scale=0.3, x_scale=0.7)


def special_values(t):
    c = t(0.1)
    return [c, np.nextafter(c, t(1)), np.nextafter(c, t(0)), -c, -np.nextafter(c, t(1)), -np.nextafter(c, t(0)),
            t(-0.0), t(np.inf), t(-np.inf), t(np.nan)]


def special_actions(rs, B, n, f64):
    """Random actions around the clip, with the clip constant of the action dtype, its two
    neighbours, their negatives and -0.0 in fixed slots of env 0 (agent 8 + k component 0,
    agent 24 + k component 1), +-inf in the same slots of env 1 and NaN in those of env 2.
    Env 0 stays finite under every preset, so its centralised controller (a sum over all
    agents) is compared by value; env 1 is too under "stochastic", whose clip makes +-inf
    +-0.1, while under "leader" and "obstacle" its velocities are +-inf and the centralised
    controller is NaN everywhere, like env 2's: those are compared by NaN mask, and by
    value in the decentralised form."""
    t = np.float64 if f64 else np.float32
    u = actions(rs, B, n, f64, scale=0.25)
    sp = special_values(t)
    for k, val in enumerate(sp):
        b = 0 if k < 7 else (1 if k < 9 else 2)
        u[b, 8 + k, 0] = val
        u[b, 24 + k, 1] = val
    return u


@pytest.mark.parametrize("f64", [False, True], ids=["f32", "f64"])
@pytest.mark.parametrize("n", [97, 513])
@pytest.mark.parametrize("name", ["leader", "obstacle", "stochastic"])
def test_presets_with_inexact_constants(name, n, f64):
    """np.clip(u32, -0.1, 0.1) clips at float32(0.1) and u32 * float32(0.3) rounds once in
    float32; float64 actions take the double constants. 0.7 as x_scale makes the scaling
    round both ways."""
    B = 3
    var = {k: INEXACT.get(k, val) for k, val in VARIANTS[name].items()}
    assert set(var) == set(VARIANTS[name]) and var != VARIANTS[name]
    v = VecFlockingRelative(B, n, variant=var)
    x0 = states(B, n, 1300 + n)
    v.reset(x=x0)
    rs = np.random.RandomState(n + len(name))
    u = special_actions(rs, B, n, f64)
    dt = rs.normal(0.12, 0.018, size=B)
    v.step(u, controller=True, dt=dt)
    xs = [oracle_step(x0[b], u[b], dt[b], var) for b in range(B)]
    if "u_clip" in var:  # the clipped +-inf are +-0.1: finite states; NaN stays NaN
        assert np.isfinite(xs[1]).all()
    assert np.isnan(xs[2][[17, 33]]).any(axis=1).all() and np.isfinite(xs[0]).all()
    for b in range(B):
        check_env(v, b, xs[b], var)
    check_decentralized(v, xs, var)
    v.close()


# ------------------------------------------------------------------------ c. prefix edges
def _prefix_cases():
    n = 130
    cases = []
    for k in (1, n - 1, n, n + 5):
        cases.append(("frozen_%d" % k, n, dict(n_frozen=k, u_scale=1.0, ctrl_clip=0.1), (60, 70)))
        cases.append(("velzero_%d" % k, n, dict(n_vel_zero=k, ctrl_clip=0.1), (60, 70)))
    # both prefixes end inside the second 512-agent tile
    cases.append(("both_600", 1030, dict(n_frozen=600, n_vel_zero=600, u_scale=1.0, ctrl_clip=0.1), (700, 900)))
    return cases


@pytest.mark.parametrize("case", _prefix_cases(), ids=lambda c: c[0])
def test_prefix_edges_vs_oracle(case):
    """Frozen and zero-velocity prefixes of 1, N-1, N and more than N agents (the
    epilogue's min(n_vel_zero, N)), and prefixes that end in the second tile. Two agents
    with the same state and the same action, neither frozen alone, stay coincident: the
    clipped controller's gradient term is 0/0 for them, as in the reference."""
    _, n, var, (p, q) = case
    B = 3
    for f64 in (False, True):
        v = VecFlockingRelative(B, n, variant=var)
        x0 = states(B, n, 1500 + n)
        x0[:, q] = x0[:, p]
        v.reset(x=x0)
        rs = np.random.RandomState(n + var.get("n_frozen", 0) + 3 * var.get("n_vel_zero", 0) + f64)
        u = actions(rs, B, n, f64)
        u[:, q] = u[:, p]
        v.step(u, controller=True)
        xs = [oracle_step(x0[b], u[b], 0.01, var) for b in range(B)]
        for b in range(B):
            same_bits(xs[b][q], xs[b][p], "coincident pair")
            k = var.get("n_frozen", 0)
            if k:  # the frozen prefix keeps its velocity, the first free agent does not
                same_bits(xs[b][:min(k, n), 2:], x0[b][:min(k, n), 2:], "frozen velocities")
                assert k >= n or (xs[b][k, 2:] != x0[b][k, 2:]).all()
            check_env(v, b, xs[b], var)
            assert np.isnan(v.controls(b)[[p, q]]).all()
        check_decentralized(v, xs, var)
        cen = v.controller(centralized=True)
        for b in range(B):
            with np.errstate(all="ignore"):
                want = fv.controller(xs[b], n_vel_zero=var.get("n_vel_zero", 0), clip=0.1)
            close("controller", cen[b], want, 1e-9, 1e-12)
        v.close()


# ------------------------------------------- the centralised controller on non-finite states
@pytest.mark.parametrize("n", [130, 600])
@pytest.mark.parametrize("handle", ["plain", "obstacle"])
def test_centralized_controller_nonfinite_positions(handle, n):
    """The reference zeroes a pair's gradient only where r2 > comm_radius, so a pair whose
    r2 is NaN keeps a NaN gradient in the centralised sum over all j. Velocities stay
    finite here, so nothing but that gradient can make a row NaN. Env 0: one agent with a
    NaN coordinate makes every row NaN. Env 1: two agents at +inf in x make each other's
    rows NaN (inf - inf) and no one else's; one at -inf in x and one at +inf in y have
    infinite, not NaN, r2 to everyone, so their rows and all finite rows are compared by
    value. Env 2 is finite. N = 130 is one LDS tile, N = 600 two, with the agents in both."""
    B = 3
    var = VARIANTS["obstacle"] if handle == "obstacle" else None
    p, q, r, s = 7, n - 30, 40, n - 5
    x = states(B, n, 2300 + n)
    x[0, q, 1] = np.nan
    x[1, p, 0] = np.inf
    x[1, q, 0] = np.inf
    x[1, r, 0] = -np.inf
    x[1, s, 1] = np.inf
    v = VecFlockingRelative(B, n, variant=var)
    v.reset(x=x)
    nz = (var or {}).get("n_vel_zero", 0)
    for centralized in (True, False):
        got = v.controller(centralized=centralized)
        for b in range(B):
            with np.errstate(all="ignore"):
                want = fv.controller(x[b], centralized=centralized, n_vel_zero=nz)
            if centralized:  # what the case is about, stated without the oracle
                nan_rows = np.isnan(want).all(axis=1)
                expect = {0: np.arange(n), 1: np.array([p, q]), 2: np.array([], int)}[b]
                np.testing.assert_array_equal(np.flatnonzero(nan_rows), expect)
                assert not np.isnan(want[~nan_rows]).any()
            close("controller", got[b], want, 1e-9, 1e-12)
    v.close()


# ------------------------------------------------------------------- d. batched rollout
def test_stochastic_rollout_per_step_dt_and_closed_loop():
    """12 steps of B = 5 stochastic envs, a new per-env dt at every step: six with host
    actions of alternating dtype, six closed loop (FE_U_EXPERT), where the oracle
    integrates the device's own clipped controls of the step before (themselves within
    the controller tolerance of the oracle's), so the state stays comparable bit for bit.
    Then clear_variant() with the last per-env dt still set steps like FlockingRelative at
    that dt, the variant set again keeps the dt, and set_dt(None) returns to the config dt."""
    B, n = 5, 100
    var = VARIANTS["stochastic"]
    v = VecFlockingRelative(B, n, variant="stochastic")
    x = states(B, n, 1700)
    v.reset(x=x)
    rs = np.random.RandomState(1701)
    ctrl = None
    for t in range(12):
        dt = rs.normal(0.12, 0.018, size=B)
        if t < 6:
            u = actions(rs, B, n, f64=bool(t % 2))
            v.step(u, controller=True, dt=dt)
        else:
            u = ctrl  # float64, already within +-ctrl_clip
            v.step(expert=True, controller=True, dt=dt)
        x = np.stack([oracle_step(x[b], u[b], dt[b], var) for b in range(B)])
        for b in range(B):
            check_env(v, b, x[b], var)
        ctrl = v.controls()
        assert np.abs(ctrl).max() <= 0.5
    # the last step's per-env dt is still set: it must survive clear_variant() (no set_dt
    # from here on, the steps pass no dt)
    v.h.clear_variant()
    for f64 in (False, True):
        u = actions(rs, B, n, f64)
        v.step(u, controller=True)
        x = np.stack([fo.integrate(x[b], u[b], dt=dt[b]) for b in range(B)])
        for b in range(B):
            check_env(v, b, x[b], None)
    # and the variant set again keeps it, until set_dt(None) returns to the config dt
    v.h.set_variant(**var)
    for per_env in (True, False):
        if not per_env:
            v.h.set_dt(None)
        u = actions(rs, B, n, f64=False)
        v.step(u, controller=True)
        x = np.stack([oracle_step(x[b], u[b], dt[b] if per_env else 0.01, var) for b in range(B)])
        for b in range(B):
            check_env(v, b, x[b], var)
    v.close()


# --------------------------------------------------------------------- e. split launches
@pytest.mark.parametrize("B", [3, 5, 8])
def test_split_launches_use_each_envs_dt(B):
    """With two streams a step that follows another step (or reset's compute_helpers) with
    no other call in between goes out as two half-batch launches, the first of them as
    three (the first half's first quarter alone); each launch must read its own envs' dt
    (env_range's dt_env + b0). The per-env dt is set once; k = 1..4 back-to-back steps
    are each checked against the oracle at every env's own dt, and one stream must give
    the same bits."""
    n = 97
    var = VARIANTS["obstacle"]
    x0 = states(B, n, 1900 + B)
    rs = np.random.RandomState(1901 + B)
    us = [actions(rs, B, n, f64=bool(i % 2)) for i in range(4)]
    dt = 0.004 * (1 + np.arange(B)) + 0.001 * rs.uniform(size=B)  # distinct per env
    outs = []
    for streams in (2, 1):
        v = VecFlockingRelative(B, n, variant="obstacle")
        v.h.set_streams(streams)
        v.h.set_dt(dt)
        got = []
        for k in range(1, 5):
            v.reset(x=x0)
            for i in range(k):
                v.step(us[i], controller=True)
            xs = x0
            for i in range(k):
                xs = [oracle_step(xs[b], us[i][b], dt[b], var) for b in range(B)]
            for b in range(B):
                check_env(v, b, xs[b], var)
            got += [v.get_state(), v.state_values(), v.network(), v.rewards(), v.controls()]
        outs.append(got)
        v.close()
    for a, b in zip(*outs):
        np.testing.assert_array_equal(a, b)


# ------------------------------------------------------- f. Flocking-v0 on a variant handle
@pytest.mark.parametrize("n", [100, 300])
@pytest.mark.parametrize("mode", ["obstacle", "dt_only"])
def test_flocking_v0_observation_on_variant_handle(mode, n):
    """knn=True on a handle with a variant or a per-env dt: the step writes the adjacency
    bits and the kNN kernel ranks from them (the fused selection is not built for
    variants). Indices bit-exact, obs the float32 of the float64 differences."""
    B = 3
    var = VARIANTS["obstacle"] if mode == "obstacle" else None
    v = VecFlockingRelative(B, n, n_neighbors=7, variant=var)
    x = states(B, n, 2100 + n)
    v.reset(x=x)
    rs = np.random.RandomState(2101 + n)
    dts = rs.normal(0.12, 0.018, size=(3, B))
    for t in range(3):
        u = actions(rs, B, n, f64=bool(t % 2))
        dt = dts[t] if var is None else None
        v.step(u, knn=True, dt=dt)
        x = np.stack([oracle_step(x[b], u[b], 0.01 if dt is None else dt[b], var) for b in range(B)])
        for b in range(B):
            same_bits(v.h.get_state(b), x[b])
            idx, obs = v.knn(b)
            ridx, robs = fo.knn_observation(x[b])
            np.testing.assert_array_equal(idx, ridx)
            np.testing.assert_array_equal(obs, robs.astype(np.float32))
            check_env(v, b, x[b], var, ctrl=False)
    v.close()


# ----------------------------------------------------------- the reference's own episode
class Cfg:
    def __init__(self, n):
        self.n = n

    def getfloat(self, k):
        return {"comm_radius": 0.9, "v_max": 5.0, "dt": 0.01}[k]

    def getint(self, k):
        return self.n


def test_stochastic_inexact_episode_matches_reference():
    """The reference's FlockingStochasticEnv with max_accel = 0.1 and scale = 0.3 set on
    the instance (tests/golden/variant_stochastic_inexact.npz), replayed by the drop-in
    env with the same two attributes set."""
    f = np.load(os.path.join(GOLDEN, "variant_stochastic_inexact.npz"))
    n = int(f["n_agents"])
    np.random.seed(int(f["seed"]))
    env = envs.FlockingStochasticEnv()
    env.params_from_cfg(Cfg(n))
    env.max_accel = 0.1
    env.scale = 0.3
    sv0, _ = env.reset()
    np.testing.assert_array_equal(env.x, f["x0"])
    close("state_values", sv0, f["sv0"], 1e-5, 1e-9)
    for t in range(len(f["x"])):
        u = f["u"][t].astype(np.float32) if f["u_is_f32"][t] else f["u"][t]
        (sv, net), r, done, info = env.step(u)
        assert done is False and info == {}
        assert env.dt == f["dt"][t]
        same_bits(env.x, f["x"][t])
        close("state_values", sv, f["sv"][t], 1e-5, 1e-9)
        adj = np.unpackbits(f["adj_bits"][t], axis=1, count=n).astype(bool)
        np.testing.assert_array_equal(net > 0, adj)
        deg = np.maximum(f["deg"][t], 1).astype(np.float64)
        np.testing.assert_array_equal(net, np.where(adj, (1.0 / deg).astype(np.float32)[:, None], 0))
        close("reward", r, f["reward"][t], 1e-12, 0.0)
        close("controller", env.controller(), f["ctrl"][t], 1e-9, 1e-12)
        close("controller", env.controller(centralized=False), f["ctrl_dec"][t], 1e-9, 1e-12)
    env.close()
