"""The DAgger rollout (flock_policy_rollout_kernel, fe_step_policy,
VecFlockingRelative.policy_steps) on the device: per-step parity of the recording with the
NumPy restatement consuming the engine's own actions (tests/flock_policy_numpy.py), the
mixing draws against NumPy's stream, chunking, subsampling and determinism bit for bit, the
handle's state afterwards, and the C-ABI's error contract. Needs an MI355X.

Tolerances: flock_policy_numpy.check_recording's (state, bits, degree, tap 0, policy and
applied bit-exact; the taps within the derived bound; the rest as test_flock_rollout_gpu)."""
import ctypes
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

import flock_policy_numpy as fpn
import flock_rollout_numpy as frn

pytestmark = pytest.mark.gpu

nat = pytest.importorskip("gym_flock._native")
from gym_flock.init_states import synthetic_batch  # noqa: E402
from gym_flock.vec import VecFlockingRelative  # noqa: E402

ALL = fpn.RECORDS
B = 3
BIG = (24, 64, 64, 2)


def equal_records(a, b, keys=ALL):
    for k in keys:
        assert a[k].shape == b[k].shape and a[k].dtype == b[k].dtype, k
        np.testing.assert_array_equal(np.ascontiguousarray(a[k]).view(np.uint8),
                                      np.ascontiguousarray(b[k]).view(np.uint8), err_msg=k)


def started(n, x0, widths=BIG, n_taps=4, clip=1.0, seed=1, scale=0.3, **kw):
    """A batch at x0 with a policy and a controller output: (v, u0, z0, weights, biases)."""
    v = VecFlockingRelative(x0.shape[0], n, **kw)
    ws, bs = fpn.make_policy(widths, seed, scale)
    v.set_policy(ws, bs, n_taps, clip)
    v.reset(x=x0)
    u0 = v.controller()
    return v, u0, v.aggregation(), ws, bs


# ------------------------------------------------------ 1. per-step parity on the recording
@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 128, 129, 256])
def test_recording_matches_restatement_step_by_step(n):
    x0 = synthetic_batch(B, n, seed0=1700 + n)
    v, u0, z0, ws, bs = started(n, x0)
    rec = v.policy_steps(6, beta=0.0, record=ALL)
    assert rec["agg"].shape == (6, B, n, 4, 6) and rec["policy"].shape == (6, B, n, 2)
    assert rec["applied"].shape == (6, B, n, 2) and rec["used_expert"].shape == (6, B)
    assert not rec["used_expert"].any()
    np.testing.assert_array_equal(z0[:, :, 1:], 0.0)
    fpn.check_recording(rec, x0, u0, z0, ws, bs, clip=1.0)
    v.close()


@pytest.mark.parametrize("case", ["k1_l1", "k2_l2", "sum_pooling", "decentralized", "no_clip"])
def test_recording_with_other_settings(case):
    n = 65
    widths, n_taps, clip, scale, kw = BIG, 4, 1.0, 0.3, {}
    if case == "k1_l1":
        widths, n_taps = (6, 2), 1
    elif case == "k2_l2":
        widths, n_taps = (12, 4, 2), 2
    elif case == "sum_pooling":
        kw = dict(mean_pooling=False)
    elif case == "decentralized":
        kw = dict(centralized=False)
    else:
        clip, scale = 0.0, 0.01
    x0 = synthetic_batch(B, n, seed0=1810)
    v, u0, z0, ws, bs = started(n, x0, widths, n_taps, clip, scale=scale, **kw)
    rec = v.policy_steps(6, beta=0.0, record=ALL)
    fpn.check_recording(rec, x0, u0, z0, ws, bs, clip=clip, centralized=kw.get("centralized", True),
                        mean_pooling=kw.get("mean_pooling", True))
    v.close()


# ------------------------------------------------------------------- 2. mixing and streams
def seeded(n, widths=BIG, n_taps=4, clip=1.0, seed=7):
    """A batch from reset_device(seed, reject=False): state, streams, zero taps."""
    v = VecFlockingRelative(B, n)
    ws, bs = fpn.make_policy(widths, 1)
    v.set_policy(ws, bs, n_taps, clip)
    v.reset_device(seed=seed, reject=False)
    x0, u0 = v.get_state(), v.controller()
    return v, x0, u0, v.aggregation(), ws, bs


def streams(v):
    return [v.h.get_rng_state(b) for b in range(B)]


def same_streams(a, b):
    for sa, sb in zip(a, b):
        np.testing.assert_array_equal(sa[1], sb[1])
        assert sa[2:] == sb[2:]


def test_beta_one_is_the_expert_rollout():
    v, x0, u0, z0, ws, bs = seeded(65)
    before = streams(v)
    rec = v.policy_steps(6, beta=1.0, record=ALL)
    assert (rec["used_expert"] == 1).all()
    same_streams(streams(v), before)
    w, _, _, _, _, _ = seeded(65)
    equal_records(rec, w.expert_steps(6, record=frn.RECORDS), keys=frn.RECORDS)
    v.close()
    w.close()


def test_beta_half_draws_from_each_env_stream():
    n, steps = 100, 6
    v, x0, u0, z0, ws, bs = seeded(n)
    rs = np.random.RandomState(5)
    rs.normal()  # leaves a cached Gaussian
    v.h.set_rng(rs, env=0)
    gens = [v.np_random(b) for b in range(B)]
    assert gens[0].get_state()[3] == 1
    want = np.stack([g.random_sample(steps) < 0.5 for g in gens], axis=1)
    rec = v.policy_steps(steps, beta=0.5, record=ALL)
    np.testing.assert_array_equal(rec["used_expert"], want.astype(np.uint8))
    for b in range(B):
        st, ref = v.h.get_rng_state(b), gens[b].get_state()
        np.testing.assert_array_equal(st[1], ref[1])
        assert st[2] == ref[2] and st[3] == ref[3] and st[4] == ref[4], b
    fpn.check_recording(rec, x0, u0, z0, ws, bs, clip=1.0)
    v.close()


@pytest.mark.parametrize("pos,steps", [(623, 6), (100, 320)])
def test_awkward_stream_positions(pos, steps):
    """A double whose words straddle the regeneration; a regeneration inside the draw."""
    n = 5
    v = VecFlockingRelative(B, n)
    v.set_policy(*fpn.make_policy((6, 2), 1), 1)
    v.reset(x=synthetic_batch(B, n, seed0=1900))
    v.controller()
    gens = []
    for b in range(B):
        g = np.random.RandomState(30 + b)
        g.random_sample(400)  # (a regenerated key)
        st = list(g.get_state())
        st[2] = pos
        g.set_state(tuple(st))
        gens.append(g)
    v.h.set_rng(gens)
    want = np.stack([g.random_sample(steps) < 0.5 for g in gens], axis=1)
    rec = v.policy_steps(steps, beta=0.5, record=("used_expert",))
    np.testing.assert_array_equal(rec["used_expert"], want.astype(np.uint8))
    for b in range(B):
        st, ref = v.h.get_rng_state(b), gens[b].get_state()
        np.testing.assert_array_equal(st[1], ref[1])
        assert st[2] == ref[2], b
    v.close()


# -------------------------------------------- 3. chunking, subsampling, determinism, twins
@pytest.fixture(scope="module")
def twelve_steps():
    """(the every=1 recording of 12 steps at N = 100 with beta = 0.5, the final aggregation
    and streams), shared and left unchanged."""
    v, x0, u0, z0, ws, bs = seeded(100)
    rec = v.policy_steps(12, beta=0.5, record=ALL)
    agg, st = v.aggregation(), streams(v)
    v.close()
    for a in rec.values():
        a.setflags(write=False)
    assert rec["used_expert"].any() and not rec["used_expert"].all()
    return rec, agg, st, x0


def test_two_runs_are_equal(twelve_steps):
    rec, agg, st, _ = twelve_steps
    v = seeded(100)[0]
    equal_records(v.policy_steps(12, beta=0.5, record=ALL), rec)
    np.testing.assert_array_equal(v.aggregation().view(np.uint32), agg.view(np.uint32))
    v.close()


def test_two_chunks_equal_one_rollout(twelve_steps):
    rec, agg, st, _ = twelve_steps
    v = seeded(100)[0]
    a = v.policy_steps(6, beta=0.5, record=ALL)
    b = v.policy_steps(6, beta=0.5, record=ALL)
    equal_records({k: np.concatenate([a[k], b[k]]) for k in ALL}, rec)
    np.testing.assert_array_equal(v.aggregation().view(np.uint32), agg.view(np.uint32))
    same_streams(streams(v), st)
    v.close()


@pytest.mark.parametrize("every", [2, 3])
def test_record_every(twelve_steps, every):
    rec = twelve_steps[0]
    v = seeded(100)[0]
    part = v.policy_steps(12, beta=0.5, record=ALL, every=every)
    per_step = ("rewards", "applied", "used_expert")
    idx = np.arange(every - 1, 12, every)
    assert part["agg"].shape[0] == len(idx) and part["applied"].shape[0] == 12
    equal_records(part, {k: (rec[k] if k in per_step else rec[k][idx]) for k in ALL})
    v.close()


def test_twin_stepped_with_the_applied_actions(twelve_steps):
    rec, _, _, x0 = twelve_steps
    w = VecFlockingRelative(B, 100)
    w.reset(x=x0)
    for t in range(6):
        w.step(u=np.ascontiguousarray(rec["applied"][t]), network="packed")
        bits, deg = w.network_packed()
        frn.same_bits(w.get_state(), rec["x"][t], "state %d" % t)
        np.testing.assert_array_equal(bits, rec["adj_bits"][t])
        np.testing.assert_array_equal(deg, rec["degree"][t])
    w.close()


def test_handle_after_a_call(twelve_steps):
    rec, agg, _, _ = twelve_steps
    v = seeded(100)[0]
    assert v.policy_steps(12, beta=0.5, fetch=False) is None
    bits, deg = v.network_packed()
    last = dict(x=v.get_state(), state_values=v.state_values(), adj_bits=bits, degree=deg, controls=v.controls(),
                agg=v.aggregation())
    equal_records(last, {k: rec[k][11] for k in last}, keys=last)
    np.testing.assert_array_equal(v.rewards(), rec["rewards"][11])
    with pytest.raises(nat.GymFlockError) as e:
        v.network()
    assert e.value.code == nat.GF_ESTATE
    x, u = v.get_state(), v.controls()
    more = v.expert_steps(2, record=frn.RECORDS)
    frn.check_recording(more, x, u)
    x, u = v.get_state(), v.controls()
    v.step(expert=True, controller=True, network="packed")
    frn.same_bits(v.get_state(), np.stack([frn.fo.integrate(x[b], u[b]) for b in range(B)]), "step after")
    v.close()


_TORCH_CHILD = r"""
import json, sys
import numpy as np
import torch
assert torch.cuda.is_available()
sys.path[:0] = [{root!r}, {pkg!r}, {tests!r}]
import flock_policy_numpy as fpn
from gym_flock.vec import VecFlockingRelative
B, n, T = 3, 100, 6
def seeded():
    v = VecFlockingRelative(B, n)
    v.set_policy(*fpn.make_policy((24, 64, 64, 2), 1), 4, 1.0)
    v.reset_device(seed=7, reject=False)
    v.controller()
    return v
v = seeded()
host = v.policy_steps(T, beta=0.5, record=fpn.RECORDS, every=3)
v.close()
v = seeded()
shapes = v.h.policy_shapes(T, 3)
tdt = dict(x=torch.float64, state_values=torch.float32, adj_bits=torch.int64, degree=torch.int32,
           controls=torch.float64, rewards=torch.float64, agg=torch.float32, policy=torch.float32,
           applied=torch.float64, used_expert=torch.uint8)
dev = {{k: torch.full(shapes[k][0], 3, dtype=tdt[k], device="cuda") for k in shapes}}
torch.cuda.synchronize()
out = v.policy_steps(T, beta=0.5, every=3, device_ptrs={{k: t.data_ptr() for k, t in dev.items()}})
v.sync()
ok = {{k: bool(np.array_equal(dev[k].cpu().numpy().view(np.uint8), host[k].view(np.uint8))) for k in shapes}}
ok["returns_none"] = out is None
v.close()
print("RESULT " + json.dumps(ok))
"""


def test_device_destinations_equal_host_destinations():
    """Records written straight into torch tensors equal the host records (torch imported
    before gym_flock, in a child process: this one stays torch-free)."""
    code = _TORCH_CHILD.format(root=ROOT, pkg=os.path.join(ROOT, "gym-flock_amd"), tests=os.path.join(ROOT, "tests"))
    p = subprocess.run([sys.executable, "-c", code], capture_output=True, timeout=240)
    assert p.returncode == 0, p.stderr.decode()[-3000:]
    line = [ln for ln in p.stdout.decode().splitlines() if ln.startswith("RESULT ")][-1]
    out = json.loads(line[len("RESULT "):])
    assert all(out.values()) and len(out) == 11, out


# --------------------------------------------------------------------- 4. resetting taps
def test_reset_aggregation_of_one_env(twelve_steps):
    v = seeded(100)[0]
    v.policy_steps(6, beta=0.0, fetch=False)
    before = v.aggregation()
    assert all(np.abs(before[b, :, 1:]).max() > 0 for b in range(B))
    v.reset_aggregation(envs=[1])
    after = v.aggregation()
    np.testing.assert_array_equal(after[1, :, 1:], 0.0)
    np.testing.assert_array_equal(after[1, :, 0].view(np.uint32), before[1, :, 0].view(np.uint32))
    np.testing.assert_array_equal(after[[0, 2]].view(np.uint32), before[[0, 2]].view(np.uint32))
    v.close()


def test_reset_device_resets_the_taps_of_its_envs():
    v = seeded(100)[0]
    v.policy_steps(6, beta=0.0, fetch=False)
    before = v.aggregation()
    v.reset_device(seed=None, envs=[0, 2], reject=False)
    after = v.aggregation()
    np.testing.assert_array_equal(after[[0, 2], :, 1:], 0.0)
    np.testing.assert_array_equal(after[1].view(np.uint32), before[1].view(np.uint32))
    v.close()


# ------------------------------------------------------------------- 5. the error contract
def code_of(fn):
    with pytest.raises(nat.GymFlockError) as e:
        fn()
    return e.value.code


def raw_policy(widths, n_taps, clip=0.0, activation=0, drop=None):
    ws, bs = fpn.make_policy(widths, 1)
    pol = nat.FePolicy()
    pol.n_taps, pol.n_layers, pol.clip, pol.activation = n_taps, len(ws), clip, activation
    for l in range(len(ws)):
        pol.weight[l], pol.bias[l] = ws[l].ctypes.data, bs[l].ctypes.data
        pol.width[l], pol.width[l + 1] = ws[l].shape[1], ws[l].shape[0]
    if drop == "weight":
        pol.weight[0] = None
    if drop == "bias":
        pol.bias[len(ws) - 1] = None
    return pol, (ws, bs)


def test_einval_cases_leave_the_handle_usable():
    n = 8
    x0 = synthetic_batch(B, n, seed0=2000)
    v, u0, z0, ws, bs = started(n, x0, (12, 8, 2), 2, 0.0)
    h, lib = v.h, v.h.lib
    bad = [raw_policy((30, 8, 2), 5), raw_policy((0, 2), 0), raw_policy((12, 6, 2), 2), raw_policy((12, 68, 2), 2),
           raw_policy((12, 8, 2), 2, clip=-1.0), raw_policy((12, 8, 2), 2, clip=float("nan")),
           raw_policy((12, 8, 2), 2, activation=1), raw_policy((12, 8, 2), 2, drop="weight"),
           raw_policy((12, 8, 2), 2, drop="bias"), raw_policy((12, 8, 2), 3), raw_policy((12, 8, 3), 2)]
    for pol, keep in bad:
        assert lib.fe_set_policy(h.h, ctypes.byref(pol)) == nat.GF_EINVAL
    pol, keep = raw_policy((12, 8, 2), 2)
    pol.n_layers = 4
    assert lib.fe_set_policy(h.h, ctypes.byref(pol)) == nat.GF_EINVAL
    for beta in (-0.1, 1.1, float("nan")):
        assert code_of(lambda: v.policy_steps(2, beta=beta)) == nat.GF_EINVAL
    assert code_of(lambda: v.policy_steps(0)) == nat.GF_EINVAL
    assert code_of(lambda: v.policy_steps(4, every=0)) == nat.GF_EINVAL
    assert code_of(lambda: v.policy_steps(4, every=3)) == nat.GF_EINVAL
    rec = nat.FePolicyRollout()
    rec.record_every, rec.flags = 1, 2
    assert lib.fe_step_policy(h.h, 2, 0.0, ctypes.byref(rec)) == nat.GF_EINVAL
    h.set_variant(u_scale=1.0, n_frozen=2)
    assert code_of(lambda: v.policy_steps(2)) == nat.GF_EINVAL
    h.clear_variant()
    h.set_dt(np.full(B, 0.02))
    assert code_of(lambda: v.policy_steps(2)) == nat.GF_EINVAL
    h.set_dt(None)
    h.set_dt_noise(0.01, 0.001)
    assert code_of(lambda: v.policy_steps(2)) == nat.GF_EINVAL
    h.set_dt_noise(None)
    rec = v.policy_steps(6, beta=0.0, record=ALL)  # the rejected policies changed nothing
    fpn.check_recording(rec, x0, u0, z0, ws, bs)
    v.close()
    big = VecFlockingRelative(1, 257)
    big.set_policy(ws, bs, 2)
    big.reset(x=synthetic_batch(1, 257, seed0=3))
    big.controller()
    assert code_of(lambda: big.policy_steps(2)) == nat.GF_EINVAL
    big.close()


def test_estate_cases_leave_the_handle_usable():
    n = 8
    x0 = synthetic_batch(B, n, seed0=2001)
    ws, bs = fpn.make_policy((12, 8, 2), 1)
    v = VecFlockingRelative(B, n)
    v.reset(x=x0)
    v.controller()
    assert code_of(lambda: v.policy_steps(2)) == nat.GF_ESTATE  # no policy
    v.set_policy(ws, bs, 2)
    v.set_state(x0)
    assert code_of(lambda: v.policy_steps(2)) == nat.GF_ESTATE  # no controller output
    v.compute_helpers()
    assert code_of(lambda: v.policy_steps(2)) == nat.GF_ESTATE
    u0, z0 = v.controller(), v.aggregation()
    assert code_of(lambda: v.policy_steps(2, beta=0.5)) == nat.GF_ESTATE  # streams never seeded
    v.h.comm_init(1, 0, nat.FlockHandle.comm_unique_id(), timeout=60.0)  # a communicator of one rank
    assert code_of(lambda: v.policy_steps(2)) == nat.GF_ESTATE
    v.h.comm_destroy()
    rec = v.policy_steps(6, beta=0.0, record=ALL)
    fpn.check_recording(rec, x0, u0, z0, ws, bs)
    v.close()
