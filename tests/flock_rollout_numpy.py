"""NumPy restatement of the closed-loop expert rollout (fe_step_expert /
VecFlockingRelative.expert_steps), written from oracle.flocking's integrate, helpers,
controller and reward, and the checks the CPU and GPU tests of the rollout share.

TEST INFRASTRUCTURE ONLY (not collected: no test_ prefix)."""
import numpy as np

from oracle import flocking as fo

RECORDS = ("x", "state_values", "adj_bits", "degree", "controls", "rewards")

# the project's tolerances (tests/test_flock_gpu.py): state, bits and degree are bit-exact
SV_RTOL, SV_ATOL = 1e-5, 1e-9
CTRL_RTOL, CTRL_ATOL = 1e-9, 1e-12
REWARD_RTOL = 1e-12


def pack_bits(adj):
    """(N,N) bool -> (N, ceil(N/64)) uint64 in fe_get_network_packed's layout: bit j % 64 of
    word j // 64 of row i is adj[i, j]."""
    n = adj.shape[0]
    wn = (n + 63) // 64
    out = np.zeros((n, wn), np.uint64)
    for j in range(n):
        out[:, j // 64] |= adj[:, j].astype(np.uint64) << np.uint64(j % 64)
    return out


def unpack_bits(bits, n):
    """The inverse of pack_bits: (N, Wn) uint64 -> (N,N) bool."""
    j = np.arange(n)
    return ((bits[:, j // 64] >> (j % 64).astype(np.uint64)) & np.uint64(1)).astype(bool)


def rollout(x0, n_steps, every=1, comm_radius=0.9, dt=0.01, action_scalar=10.0, centralized=True, u0=None):
    """n_steps of u = controller(x); x = step(x, u) for ONE env (x0 (N,4)), recording like
    fe_rollout: x, state_values (float64 here), adj_bits, degree, controls of every
    `every`-th step (controls: the controller of the recorded state) and every step's
    reward. u0: the first action (default controller(x0))."""
    assert every >= 1 and n_steps % every == 0
    x = np.array(x0, np.float64)
    with np.errstate(all="ignore"):
        u = fo.controller(x, comm_radius, action_scalar, centralized) if u0 is None else np.asarray(u0, np.float64)
    rec = {k: [] for k in RECORDS}
    for t in range(n_steps):
        with np.errstate(all="ignore"):
            x = fo.integrate(x, u, dt, action_scalar)
            geom = fo.pair_geometry(x)
            sv, _, adj, deg = fo.helpers(x, comm_radius, True, geom)
            u = fo.controller(x, comm_radius, action_scalar, centralized, geom)
            rec["rewards"].append(fo.reward(x))
        if (t + 1) % every == 0:
            rec["x"].append(x)
            rec["state_values"].append(sv)
            rec["adj_bits"].append(pack_bits(adj))
            rec["degree"].append(deg.astype(np.int32))
            rec["controls"].append(u)
    return {k: np.stack(v) for k, v in rec.items()}


def same_bits(ours, ref, what):
    """Bit-exact float64, the sign of zero included; NaN wherever the reference has NaN."""
    ours, ref = np.ascontiguousarray(ours, np.float64), np.ascontiguousarray(ref, np.float64)
    np.testing.assert_array_equal(np.isnan(ours), np.isnan(ref), err_msg=what + " NaN mask")
    ok = ~np.isnan(ref)
    np.testing.assert_array_equal(ours.view(np.uint64)[ok], ref.view(np.uint64)[ok], err_msg=what)


def close(ours, ref, rtol, atol, what):
    """Equal NaN masks; rtol / atol elsewhere (infinities must be equal)."""
    ours, ref = np.asarray(ours, np.float64), np.asarray(ref, np.float64)
    np.testing.assert_array_equal(np.isnan(ours), np.isnan(ref), err_msg=what + " NaN mask")
    ok = ~np.isnan(ref)
    np.testing.assert_allclose(ours[ok], ref[ok], rtol=rtol, atol=atol, err_msg=what)


def check_recording(rec, x0, u0, comm_radius=0.9, dt=0.01, action_scalar=10.0, centralized=True):
    """The project's parity protocol on an every=1 recording of a batch (arrays (T,B,N,.)),
    the oracle consuming the recording's own actions: for every step t and env b,
    integrate(x[t-1], controls[t-1]) is x[t] bit for bit (t = 0: x0, u0, the state and
    controls before the call), adjacency bits and degree of x[t] are exact, and
    state_values[t], controls[t], rewards[t] are within the project's tolerances."""
    T, B = rec["x"].shape[:2]
    for t in range(T):
        for b in range(B):
            xp = x0[b] if t == 0 else rec["x"][t - 1, b]
            up = u0[b] if t == 0 else rec["controls"][t - 1, b]
            what = "step %d env %d " % (t, b)
            with np.errstate(all="ignore"):
                x1 = fo.integrate(xp, up, dt, action_scalar)
                geom = fo.pair_geometry(x1)
                sv, _, adj, deg = fo.helpers(x1, comm_radius, True, geom)
                want_u = fo.controller(x1, comm_radius, action_scalar, centralized, geom)
                want_r = fo.reward(x1)
            same_bits(rec["x"][t, b], x1, what + "state")
            np.testing.assert_array_equal(rec["adj_bits"][t, b], pack_bits(adj), err_msg=what + "adjacency bits")
            np.testing.assert_array_equal(rec["degree"][t, b], deg, err_msg=what + "degree")
            close(rec["state_values"][t, b], sv, SV_RTOL, SV_ATOL, what + "state_values")
            close(rec["controls"][t, b], want_u, CTRL_RTOL, CTRL_ATOL, what + "controls")
            close(rec["rewards"][t, b], want_r, REWARD_RTOL, 0.0, what + "reward")


def free_run_sensitivity(f, n_steps=20, patterns=20, seed=0):
    """How far the reference's own closed loop moves when every action is off by the
    controller tolerance: the oracle's free run from the golden episode's x0 with each
    action moved by +-(CTRL_ATOL + CTRL_RTOL |u|), `patterns` random sign patterns, the
    worst deviation of any state entry of the first n_steps from the golden states."""
    rs = np.random.RandomState(seed)
    worst = 0.0
    for _ in range(patterns):
        x = np.array(f["x0"], np.float64)
        for t in range(n_steps):
            u = fo.controller(x)
            sign = rs.choice([-1.0, 1.0], size=u.shape)
            x = fo.integrate(x, u + sign * (CTRL_ATOL + CTRL_RTOL * np.abs(u)))
            worst = max(worst, float(np.abs(x - f["x"][t]).max()))
    return worst
