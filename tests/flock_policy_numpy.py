"""NumPy restatement of the DAgger rollout (fe_step_policy / VecFlockingRelative.policy_steps):
the float32 sequential network, the delayed-aggregation recursion, a free-running rollout
built on oracle.flocking, and the per-step checks the CPU and GPU tests share.

TEST INFRASTRUCTURE ONLY (not collected: no test_ prefix)."""
import numpy as np

from oracle import flocking as fo

import flock_rollout_numpy as frn

RECORDS = frn.RECORDS + ("agg", "policy", "applied", "used_expert")
F32_TINY = np.float32(2.0 ** -126)  # the smallest normal float32
EPS32, EPS64_SUM, DENORM = 2.0 ** -23, 2.0 ** -44, 2.0 ** -149


def make_policy(widths, seed, scale=0.3):
    """Seeded weights and biases, uniform in +-scale, float32, torch.nn.Linear's layout."""
    rs = np.random.RandomState(seed)
    ws = [rs.uniform(-scale, scale, size=(widths[l + 1], widths[l])).astype(np.float32) for l in range(len(widths) - 1)]
    bs = [rs.uniform(-scale, scale, size=(widths[l + 1],)).astype(np.float32) for l in range(len(widths) - 1)]
    return ws, bs


def _assert_normal(v, a=None, b=None, what=""):
    """No subnormal value; with the factors a, b: no product of two non-zeros that
    underflowed to zero either. The device's flush mode then cannot matter."""
    av = np.abs(v)
    assert not ((av > 0) & (av < F32_TINY)).any(), "subnormal " + what
    if a is not None:
        assert not ((v == 0) & (a != 0) & (b != 0)).any(), "underflow " + what


def flat(z):
    """(..., n_taps, 6) -> (..., 6 * n_taps): the network's input order."""
    z = np.asarray(z, np.float32)
    return z.reshape(z.shape[:-2] + (z.shape[-2] * 6,))


def mlp(z, weights, biases, clip=0.0, check_normal=True):
    """The shared network on rows of inputs z (..., 6 * n_taps) (flat(): index 6k + f), float32,
    in the library's order: every output starts from its bias and adds w[o, i] * x[i] for i
    ascending, each product and each sum rounded to float32 once; ReLU (x > 0 ? x : 0) after
    every layer but the last; clip > 0 (as float32) clips the outputs. Returns (..., width[-1])
    float32. check_normal: assert that no product or partial sum is subnormal."""
    z = np.asarray(z, np.float32)
    n_in = weights[0].shape[1]
    assert z.shape[-1] == n_in, (z.shape, n_in)
    lead = z.shape[:-1]
    x = z.reshape(-1, n_in)
    for l, (w, b) in enumerate(zip(weights, biases)):
        w, b = np.asarray(w, np.float32), np.asarray(b, np.float32)
        acc = np.broadcast_to(b, (x.shape[0], w.shape[0])).copy()
        for i in range(w.shape[1]):
            wi, xi = w[None, :, i], x[:, i, None]
            prod = wi * xi
            acc = acc + prod
            assert prod.dtype == np.float32 and acc.dtype == np.float32
            if check_normal:
                _assert_normal(prod, np.broadcast_to(wi, prod.shape), np.broadcast_to(xi, prod.shape),
                               "product, layer %d input %d" % (l, i))
                _assert_normal(acc, what="partial sum, layer %d input %d" % (l, i))
        x = np.where(acc > 0, acc, np.float32(0)) if l < len(weights) - 1 else acc
    if clip > 0:
        c = np.float32(clip)
        x = np.where(x < -c, -c, np.where(x > c, c, x))
    return x.astype(np.float32).reshape(lead + (x.shape[-1],))


def mlp_f64(z, weights, biases):
    """The same network as float64 matrix products (ReLU, no clip): (M, 2)."""
    x = np.asarray(z, np.float64).reshape(-1, weights[0].shape[1])
    for l, (w, b) in enumerate(zip(weights, biases)):
        x = x @ np.asarray(w, np.float64).T + np.asarray(b, np.float64)
        if l < len(weights) - 1:
            x = np.maximum(x, 0.0)
    return x


def next_taps(z_prev, sv, adj, deg, mean_pooling=True):
    """z of a state from the previous state's z_prev (N,K,6) float32, the state's float32
    state_values sv (N,6), adjacency (N,N) bool and degree: tap 0 is sv, tap k >= 1 is
    float32((sum over adjacent j of double(z_prev[j, k-1])) / d), d = max(deg, 1) with mean
    pooling, else 1. Returns (z (N,K,6) float32, bound (N,K,6)): the bound of a float64 sum
    of the same terms taken in another order, the division, and one float32 rounding on
    either side: 2^-23 |z| + 2^-44 sum|terms| / d + 2^-149 (0 for tap 0)."""
    z_prev = np.asarray(z_prev, np.float32)
    n, k_taps = z_prev.shape[:2]
    z = np.zeros((n, k_taps, 6), np.float32)
    bound = np.zeros((n, k_taps, 6))
    z[:, 0] = np.asarray(sv, np.float32)
    a = np.asarray(adj, np.float64)
    d = (np.maximum(np.asarray(deg), 1) if mean_pooling else np.ones(n)).astype(np.float64)[:, None]
    for k in range(1, k_taps):
        terms = z_prev[:, k - 1].astype(np.float64)
        with np.errstate(all="ignore"):
            s = (a @ terms) / d
            z[:, k] = s.astype(np.float32)
            bound[:, k] = EPS32 * np.abs(s) + EPS64_SUM * (a @ np.abs(terms)) / d + DENORM
    return z, bound


def initial_agg(sv, n_taps):
    """An episode's first aggregation: ([state_values, 0 ...])."""
    sv = np.asarray(sv, np.float32)
    z = np.zeros(sv.shape[:-1] + (n_taps, 6), np.float32)
    z[..., 0, :] = sv
    return z


def rollout(x0, n_steps, weights, biases, n_taps, used_expert, clip=0.0, z0=None, comm_radius=0.9, dt=0.01,
            action_scalar=10.0, centralized=True, mean_pooling=True, check_normal=True):
    """The DAgger loop for ONE env, free-running, recording every step like fe_policy_rollout
    (state_values as float32 of the oracle's). used_expert: (n_steps) bools. z0: the first
    state's aggregation (default: an episode's start)."""
    x = np.array(x0, np.float64)
    with np.errstate(all="ignore"):
        sv, _, adj, deg = fo.helpers(x, comm_radius, True)
        u = fo.controller(x, comm_radius, action_scalar, centralized)
    z = initial_agg(sv, n_taps) if z0 is None else np.asarray(z0, np.float32)
    pol = mlp(flat(z), weights, biases, clip, check_normal)
    rec = {k: [] for k in RECORDS}
    for t in range(n_steps):
        ue = bool(used_expert[t])
        applied = u if ue else pol.astype(np.float64)
        with np.errstate(all="ignore"):
            x = fo.integrate(x, applied, dt, action_scalar)
            geom = fo.pair_geometry(x)
            sv, _, adj, deg = fo.helpers(x, comm_radius, True, geom)
            u = fo.controller(x, comm_radius, action_scalar, centralized, geom)
            rw = fo.reward(x)
        sv = sv.astype(np.float32)
        z, _ = next_taps(z, sv, adj, deg, mean_pooling)
        pol = mlp(flat(z), weights, biases, clip, check_normal)
        for name, v in (("x", x), ("state_values", sv), ("adj_bits", frn.pack_bits(adj)), ("degree", deg.astype(np.int32)),
                        ("controls", u), ("rewards", rw), ("agg", z), ("policy", pol), ("applied", applied),
                        ("used_expert", np.uint8(ue))):
            rec[name].append(v)
    return {k: np.stack(v) for k, v in rec.items()}


def rollout_batch(x0, n_steps, weights, biases, n_taps, used_expert, **kw):
    """rollout() of every env of x0 (B,N,4), used_expert (n_steps,B): arrays (T,B,...)."""
    recs = [rollout(x0[b], n_steps, weights, biases, n_taps, used_expert[:, b], **kw) for b in range(x0.shape[0])]
    return {k: np.stack([r[k] for r in recs], axis=1) for k in RECORDS}


def same_f32(ours, ref, what):
    ours, ref = np.ascontiguousarray(ours, np.float32), np.ascontiguousarray(ref, np.float32)
    np.testing.assert_array_equal(ours.view(np.uint32), ref.view(np.uint32), err_msg=what)


def check_recording(rec, x0, u0, z0, weights, biases, clip=0.0, comm_radius=0.9, dt=0.01, action_scalar=10.0,
                    centralized=True, mean_pooling=True, check_normal=True):
    """The parity protocol on an every=1 recording of a batch (arrays (T,B,...)), the oracle
    consuming the recording's own actions. x0, u0, z0: state (B,N,4), controller output
    (B,N,2) and aggregation (B,N,K,6) before the call. For every step t and env b:
      applied[t] == where(used_expert[t], controls[t-1], double(policy[t-1])) bit for bit
        (t = 0: u0 and the network on z0);
      x[t] == integrate(x[t-1], applied[t]) bit for bit;
      adjacency bits and degree of x[t] exact; state_values, controls, rewards within the
        project's tolerances (flock_rollout_numpy);
      agg[t][:, 0] == state_values[t] bit for bit; agg[t][:, k >= 1] within next_taps' bound of
        the recursion on the recorded agg[t-1] and the recorded bits;
      policy[t] == the network on the recorded agg[t], bit for bit."""
    T, B = rec["x"].shape[:2]
    n = rec["x"].shape[2]
    assert rec["applied"].shape[0] == T and rec["agg"].shape[0] == T, "check_recording needs every=1"
    for t in range(T):
        for b in range(B):
            what = "step %d env %d " % (t, b)
            xp = x0[b] if t == 0 else rec["x"][t - 1, b]
            up = u0[b] if t == 0 else rec["controls"][t - 1, b]
            zp = z0[b] if t == 0 else rec["agg"][t - 1, b]
            pp = mlp(flat(zp), weights, biases, clip, check_normal) if t == 0 else rec["policy"][t - 1, b]
            ue = rec["used_expert"][t, b]
            assert ue in (0, 1), what + "used_expert"
            want_applied = np.asarray(up, np.float64) if ue else np.asarray(pp, np.float32).astype(np.float64)
            frn.same_bits(rec["applied"][t, b], want_applied, what + "applied")
            with np.errstate(all="ignore"):
                x1 = fo.integrate(xp, rec["applied"][t, b], dt, action_scalar)
                geom = fo.pair_geometry(x1)
                sv, _, adj, deg = fo.helpers(x1, comm_radius, True, geom)
                want_u = fo.controller(x1, comm_radius, action_scalar, centralized, geom)
                want_r = fo.reward(x1)
            frn.same_bits(rec["x"][t, b], x1, what + "state")
            np.testing.assert_array_equal(rec["adj_bits"][t, b], frn.pack_bits(adj), err_msg=what + "adjacency bits")
            np.testing.assert_array_equal(rec["degree"][t, b], deg, err_msg=what + "degree")
            frn.close(rec["state_values"][t, b], sv, frn.SV_RTOL, frn.SV_ATOL, what + "state_values")
            frn.close(rec["controls"][t, b], want_u, frn.CTRL_RTOL, frn.CTRL_ATOL, what + "controls")
            frn.close(rec["rewards"][t, b], want_r, frn.REWARD_RTOL, 0.0, what + "reward")
            agg = rec["agg"][t, b]
            same_f32(agg[:, 0], rec["state_values"][t, b], what + "tap 0")
            radj = frn.unpack_bits(rec["adj_bits"][t, b], n)
            want_z, bound = next_taps(zp, rec["state_values"][t, b], radj, rec["degree"][t, b], mean_pooling)
            err = np.abs(agg[:, 1:].astype(np.float64) - want_z[:, 1:].astype(np.float64))
            assert (err <= bound[:, 1:]).all(), what + "taps: worst excess %g" % float((err - bound[:, 1:]).max())
            same_f32(rec["policy"][t, b], mlp(flat(agg), weights, biases, clip, check_normal), what + "policy")
