"""The closed-loop expert rollout (flock_rollout_kernel, fe_step_expert,
VecFlockingRelative.expert_steps) on the device: per-step parity of the recording with the
oracle consuming the engine's own actions, one rollout step against the single step,
chunking and determinism bit for bit, the reference's golden episode, the variants, and
the edges of the C-ABI contract. Needs an MI355X.

Tolerances are those of tests/test_flock_gpu.py: state, adjacency bits and degree
bit-exact, state_values rtol 1e-5 atol 1e-9, controls rtol 1e-9 atol 1e-12, reward rtol
1e-12."""
import json
import os
import subprocess
import sys
import types

import numpy as np
import pytest

from conftest import GOLDEN, ROOT

import flock_rollout_numpy as frn

pytestmark = pytest.mark.gpu

nat = pytest.importorskip("gym_flock._native")
from gym_flock.init_states import synthetic_batch  # noqa: E402
from gym_flock.vec import VARIANTS, VecFlockingRelative  # noqa: E402

ALL = frn.RECORDS
B = 3


def started(n, x0, **kw):
    """A batch at x0 with a controller output (what expert_steps needs); returns (v, u0)."""
    v = VecFlockingRelative(x0.shape[0], n, **kw)
    v.reset(x=x0)
    return v, v.controller()


def equal_records(a, b, keys=ALL):
    """Bit for bit (NaN payloads and the sign of zero included)."""
    for k in keys:
        assert a[k].shape == b[k].shape and a[k].dtype == b[k].dtype, k
        np.testing.assert_array_equal(np.ascontiguousarray(a[k]).view(np.uint8),
                                      np.ascontiguousarray(b[k]).view(np.uint8), err_msg=k)


# ------------------------------------------------------ 1. per-step parity on the recording
@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 100, 128, 129, 256])
def test_recording_matches_oracle_step_by_step(n):
    """Every column layout (16, 32 and 64 columns per thread, at their upper edges), the
    last full and first ragged adjacency word, one and two agents, and the largest env."""
    x0 = synthetic_batch(B, n, seed0=700 + n)
    v, u0 = started(n, x0)
    rec = v.expert_steps(12, record=ALL)
    assert rec["x"].shape == (12, B, n, 4) and rec["adj_bits"].shape == (12, B, n, (n + 63) // 64)
    assert rec["state_values"].dtype == np.float32 and rec["degree"].dtype == np.int32
    frn.check_recording(rec, x0, u0)
    v.close()


def test_recording_from_an_accepted_device_reset():
    """N = 100 (the reference's default) from reset()'s own distribution: every env an
    accepted draw (min degree >= 2, min distance >= 0.1)."""
    n = 100
    v = VecFlockingRelative(B, n)
    tries, status = v.reset_device(seed=5, max_tries=4096)
    assert (status == 0).all(), (tries, status)
    x0, u0 = v.get_state(), v.controller()
    rec = v.expert_steps(12, record=ALL)
    assert rec["degree"][0].min() >= 1
    frn.check_recording(rec, x0, u0)
    v.close()


@pytest.mark.parametrize("mean_pooling,centralized", [(True, False), (False, True), (False, False)])
def test_recording_with_config_switches(mean_pooling, centralized):
    n = 65
    x0 = synthetic_batch(B, n, seed0=810)
    v, u0 = started(n, x0, mean_pooling=mean_pooling, centralized=centralized)
    rec = v.expert_steps(12, record=ALL)
    frn.check_recording(rec, x0, u0, centralized=centralized)
    v.close()


# ------------------------------------------------------- 2. one step is the single step
@pytest.mark.parametrize("n", [64, 100, 256])
def test_one_step_is_the_single_step(n):
    x0 = synthetic_batch(B, n, seed0=900 + n)
    v, _ = started(n, x0)
    rec = v.expert_steps(1, record=ALL)
    w, _ = started(n, x0)
    w.step(expert=True, controller=True, network="packed")
    bits, deg = w.network_packed()
    frn.same_bits(rec["x"][0], w.get_state(), "state")
    np.testing.assert_array_equal(rec["adj_bits"][0], bits)
    np.testing.assert_array_equal(rec["degree"][0], deg)
    frn.close(rec["state_values"][0], w.state_values(), frn.SV_RTOL, frn.SV_ATOL, "state_values")
    frn.close(rec["controls"][0], w.controls(), frn.CTRL_RTOL, frn.CTRL_ATOL, "controls")
    frn.close(rec["rewards"][0], w.rewards(), frn.REWARD_RTOL, 0.0, "rewards")
    v.close()
    w.close()


# ------------------------------------------------- 3. chunking and determinism, bit for bit
@pytest.fixture(scope="module")
def ten_steps():
    """(x0, the every=1 recording of 10 steps at N = 100), shared and left unchanged."""
    n = 100
    x0 = synthetic_batch(B, n, seed0=1000)
    v, _ = started(n, x0)
    rec = v.expert_steps(10, record=ALL)
    v.close()
    for a in rec.values():
        a.setflags(write=False)
    return x0, rec


def test_two_runs_are_equal(ten_steps):
    x0, rec = ten_steps
    v, _ = started(100, x0)
    equal_records(v.expert_steps(10, record=ALL), rec)
    v.close()


def test_two_chunks_equal_one_rollout(ten_steps):
    x0, rec = ten_steps
    v, _ = started(100, x0)
    a = v.expert_steps(5, record=ALL)
    b = v.expert_steps(5, record=ALL)  # continues without a new controller()
    equal_records({k: np.concatenate([a[k], b[k]]) for k in ALL}, rec)
    v.close()


def test_record_every_fifth_step(ten_steps):
    x0, rec = ten_steps
    v, _ = started(100, x0)
    part = v.expert_steps(10, record=ALL, every=5)
    assert part["x"].shape[0] == 2 and part["rewards"].shape == (10, B)
    equal_records(part, {k: (rec[k] if k == "rewards" else rec[k][[4, 9]]) for k in ALL})
    v.close()


def test_unfetched_rollout_leaves_the_last_record_in_the_getters(ten_steps):
    x0, rec = ten_steps
    v, _ = started(100, x0)
    assert v.expert_steps(10, fetch=False) is None
    bits, deg = v.network_packed()
    last = dict(x=v.get_state(), state_values=v.state_values(), adj_bits=bits, degree=deg, controls=v.controls())
    equal_records(last, {k: rec[k][9] for k in last}, keys=last)
    np.testing.assert_array_equal(v.rewards(), rec["rewards"][9])
    v.close()


_TORCH_CHILD = r"""
import json, sys
import numpy as np
import torch
assert torch.cuda.is_available()
sys.path[:0] = [{root!r}, {pkg!r}]
from gym_flock.init_states import synthetic_batch
from gym_flock.vec import VecFlockingRelative
B, n, T = 3, 100, 10
x0 = synthetic_batch(B, n, seed0=1000)
def started():
    v = VecFlockingRelative(B, n)
    v.reset(x=x0)
    v.controller()
    return v
v = started()
host = v.expert_steps(T, record=("x", "state_values", "adj_bits", "degree", "controls", "rewards"), every=5)
v.close()
v = started()
shapes = v.h.rollout_shapes(T, 5)
tdt = dict(x=torch.float64, state_values=torch.float32, adj_bits=torch.int64, degree=torch.int32,
           controls=torch.float64, rewards=torch.float64)
dev = {{k: torch.full(shapes[k][0], -1, dtype=tdt[k], device="cuda") for k in shapes}}
torch.cuda.synchronize()
out = v.expert_steps(T, every=5, device_ptrs={{k: t.data_ptr() for k, t in dev.items()}})
v.sync()
ok = {{k: bool(np.array_equal(dev[k].cpu().numpy().view(np.uint8), host[k].view(np.uint8))) for k in shapes}}
ok["returns_none"] = out is None
v.close()
print("RESULT " + json.dumps(ok))
"""


def test_device_destinations_equal_host_destinations():
    """Records written straight into torch tensors (data_ptr(), FE_ROLLOUT_DEVICE) equal
    the host records. torch is imported before gym_flock in a child
    process: this one stays torch-free."""
    code = _TORCH_CHILD.format(root=ROOT, pkg=os.path.join(ROOT, "gym-flock_amd"))
    p = subprocess.run([sys.executable, "-c", code], capture_output=True, timeout=240)
    assert p.returncode == 0, p.stderr.decode()[-3000:]
    line = [ln for ln in p.stdout.decode().splitlines() if ln.startswith("RESULT ")][-1]
    out = json.loads(line[len("RESULT "):])
    assert all(out.values()) and len(out) == 7, out


# ------------------------------------------------------ 4. the reference's own episode
def test_reference_episode_free_run():
    """flock_n10_episode.npz opens with 20 expert steps: the rollout from its x0 records
    the reference's adjacency exactly (the nearest pair stays 1.76e-3 from either
    threshold) and its states within 10 x the free-run sensitivity, computed here: the
    oracle's closed loop with every action moved by +- the controller tolerance, 20 sign
    patterns, worst deviation from the golden states (1.2e-9; the factor 10 allows for
    device sums whose error the random signs do not reach)."""
    f = np.load(os.path.join(GOLDEN, "flock_n10_episode.npz"))
    v, u0 = started(10, f["x0"][None])
    np.testing.assert_allclose(u0[0], f["u"][0], rtol=1e-9, atol=1e-12)
    rec = v.expert_steps(20, record=("x", "adj_bits", "degree", "rewards"))
    v.close()
    for t in range(20):
        np.testing.assert_array_equal(frn.unpack_bits(rec["adj_bits"][t, 0], 10), f["net"][t] > 0)
        np.testing.assert_array_equal(rec["degree"][t, 0], (f["net"][t] > 0).sum(axis=1))
    sens = frn.free_run_sensitivity(f)
    dev = float(np.abs(rec["x"][:, 0] - f["x"][:20]).max())
    print("free-run sensitivity %.3e, rollout's deviation from the golden states %.3e" % (sens, dev))
    assert dev <= 10 * sens


# ---------------------------------------------------------------------------- 5. variants
class _StepView:
    """Step t of a recording behind the getters check_env reads (the dense network rebuilt
    from the recorded bits and degree)."""

    def __init__(self, rec, t, n):
        self.rec, self.t, self.n = rec, t, n
        self.h = types.SimpleNamespace(get_state=lambda b: rec["x"][t, b])

    def network(self, b):
        adj = frn.unpack_bits(self.rec["adj_bits"][self.t, b], self.n)
        deg = self.rec["degree"][self.t, b]
        return (adj / np.where(deg == 0, 1, deg).astype(np.float64)[:, None]).astype(np.float32)

    def state_values(self, b):
        return self.rec["state_values"][self.t, b]

    def rewards(self):
        return self.rec["rewards"][self.t]

    def controls(self, b):
        return self.rec["controls"][self.t, b]


@pytest.mark.parametrize("name", ["relative", "leader", "obstacle", "stochastic"])
def test_variants_step_by_step(name):
    """The variant matrix's per-step protocol (oracle_step, check_env) on the recording;
    the stochastic variant with a per-env dt set once. Leaders keep their velocity and
    obstacles (at rest) their whole state, bit for bit."""
    from test_flock_variant_matrix_gpu import check_env, oracle_step
    n, T = 20, 6
    var = VARIANTS[name]
    x0 = synthetic_batch(B, n, seed0=1200)
    nf = var.get("n_frozen", 0)
    if name == "obstacle":
        x0[:, :nf, 2:4] = 0.0
    v = VecFlockingRelative(B, n, variant=name)
    v.reset(x=x0)
    dt = np.array([0.1, 0.12, 0.145]) if name == "stochastic" else None
    if dt is not None:
        v.h.set_dt(dt)
    u = v.controller()
    rec = v.expert_steps(T, record=ALL)
    v.close()
    x = x0
    for t in range(T):
        x = np.stack([oracle_step(x[b], u[b], 0.01 if dt is None else dt[b], var) for b in range(B)])
        view = _StepView(rec, t, n)
        for b in range(B):
            check_env(view, b, x[b], var)
        x, u = rec["x"][t], rec["controls"][t]  # the oracle follows the engine's trajectory
        if nf:
            frn.same_bits(x[:, :nf, 2:4], x0[:, :nf, 2:4], "frozen velocities")
        if name == "obstacle":
            frn.same_bits(x[:, :nf], x0[:, :nf], "obstacles")


# ------------------------------------------------------------------------------- 6. edges
def test_refusals():
    n = 20
    x0 = synthetic_batch(B, n, seed0=1300)
    v = VecFlockingRelative(B, n)
    v.reset(x=x0)  # an observation, but no controller output
    with pytest.raises(nat.GymFlockError) as e:
        v.expert_steps(4)
    assert e.value.code == nat.GF_ESTATE and "FE_U_EXPERT needs a previous controller output" in str(e.value)
    v.controller()
    for bad in (dict(n_steps=12, every=5), dict(n_steps=0), dict(n_steps=4, every=0)):
        with pytest.raises(nat.GymFlockError) as e:
            v.expert_steps(**bad)
        assert e.value.code == nat.GF_EINVAL, bad
    assert v.expert_steps(4)["rewards"].shape == (4, B)  # the handle is still usable
    v.close()
    w, _ = started(257, synthetic_batch(1, 257, seed0=1))
    with pytest.raises(nat.GymFlockError) as e:
        w.expert_steps(1)
    assert e.value.code == nat.GF_EINVAL and "fe_step(FE_U_EXPERT" in str(e.value)
    w.close()


def test_nan_env_matches_the_single_step_and_spares_its_neighbours():
    n = 65
    x0 = synthetic_batch(B, n, seed0=1400)
    clean, _ = started(n, x0)
    want = clean.expert_steps(3, record=ALL)
    clean.close()
    x0[1, 7, 0] = np.nan
    v, _ = started(n, x0)
    rec = v.expert_steps(3, record=ALL)
    w, _ = started(n, x0)
    w.step(expert=True, controller=True, network="packed")
    bits, deg = w.network_packed()
    single = dict(x=w.get_state(), state_values=w.state_values(), controls=w.controls(), rewards=w.rewards())
    for k, ref in single.items():
        np.testing.assert_array_equal(np.isnan(rec[k][0]), np.isnan(ref), err_msg=k + " NaN positions")
    assert np.isnan(rec["x"][0, 1]).all() and np.isnan(rec["rewards"][0, 1])
    np.testing.assert_array_equal(rec["adj_bits"][0], bits)
    np.testing.assert_array_equal(rec["degree"][0], deg)
    for b in (0, 2):
        equal_records({k: rec[k][:, b] for k in ALL}, {k: want[k][:, b] for k in ALL})
    v.close()
    w.close()


def test_dense_network_is_stale_until_written_again():
    """After a rollout network() raises until compute_helpers(); a plain step afterwards
    stores the same dense network as a fresh handle set to that state (the delta store's
    record is rebuilt)."""
    n = 100
    x0 = synthetic_batch(B, n, seed0=1500)
    u = np.random.RandomState(3).uniform(-1, 1, size=(B, n, 2)).astype(np.float32)
    v = VecFlockingRelative(B, n)
    v.reset(x=x0)
    v.step(u)  # a plain step: the delta store's record now describes the buffer
    v.controller()
    v.expert_steps(6, fetch=False)
    with pytest.raises(nat.GymFlockError) as e:
        v.network()
    assert e.value.code == nat.GF_ESTATE
    x1 = v.get_state()
    fresh = VecFlockingRelative(B, n)
    fresh.reset(x=x1)
    v.compute_helpers()
    np.testing.assert_array_equal(v.network(), fresh.network())
    v.controller()
    v.expert_steps(2, fetch=False)
    x2 = v.get_state()
    v.step(u)  # straight after the rollout: stores in full
    fresh.set_state(x2)
    fresh.step(u)
    np.testing.assert_array_equal(v.network(), fresh.network())
    frn.same_bits(v.get_state(), fresh.get_state(), "state")
    v.close()
    fresh.close()


def test_rollout_queued_behind_a_split_step():
    """The rollout waits for both halves of a two-stream step that is still queued."""
    n = 100
    x0 = synthetic_batch(4, n, seed0=1600)
    recs = []
    for streams in (2, 1):
        v, _ = started(n, x0)
        v.h.set_streams(streams)
        v.sync()  # both streams idle: the next step splits (with two streams)
        for _ in range(3):
            v.step(expert=True, controller=True, network="packed")
        recs.append(v.expert_steps(4, record=ALL))
        v.close()
    equal_records(recs[0], recs[1])
    assert np.isfinite(recs[0]["x"]).all()
