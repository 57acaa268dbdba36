"""The DAgger rollout's NumPy restatement (tests/flock_policy_numpy.py) checked on the CPU,
no kernel launched: the tap recursion against the dense product form, the float32 network
against float64 matrix products, check_recording on the restatement's own recording and on
single corrupted entries, and the C-ABI's declarations and bindings."""
import ctypes
import os
import re

import numpy as np
import pytest

from conftest import ROOT

from oracle import flocking as fo

import flock_policy_numpy as fpn
import flock_rollout_numpy as frn

nat = pytest.importorskip("gym_flock._native")

WIDTHS = (24, 32, 32, 2)
N, T, B = 20, 8, 2


def synthetic(n, seed):
    return fo.synthetic_state(n, seed)


@pytest.fixture(scope="module")
def own_recording():
    """(x0, u0, z0, weights, biases, the restatement's every-step recording), read-only."""
    ws, bs = fpn.make_policy(WIDTHS, seed=11)
    x0 = np.stack([synthetic(N, 40 + b) for b in range(B)])
    used = np.random.RandomState(3).random_sample((T, B)) < 0.5
    assert used.any() and not used.all()
    rec = fpn.rollout_batch(x0, T, ws, bs, 4, used, clip=1.0)
    u0 = np.stack([fo.controller(x0[b]) for b in range(B)])
    z0 = np.stack([fpn.initial_agg(fo.helpers(x0[b])[0], 4) for b in range(B)])
    for a in rec.values():
        a.setflags(write=False)
    return x0, u0, z0, ws, bs, rec


def check(rec, own):
    x0, u0, z0, ws, bs, _ = own
    fpn.check_recording(rec, x0, u0, z0, ws, bs, clip=1.0)


def test_recursion_equals_the_dense_product_form():
    """z_t[:, k] = S_t S_{t-1} ... S_{t-k+1} state_values_{t-k} (S the dense mean-pooling
    network, zero before the episode's start), element-wise within the recursion's derived
    bound accumulated over its k applications: E_t[:, k] = S_t E_{t-1}[:, k-1] + bound_t[:, k]
    with E[:, 0] = 0 (tap 0 is the same float32 on both sides). An application's own bound is
    next_taps'; the error it inherits passes through the same averaging as the values."""
    n, steps, k_taps = 20, 8, 4
    x = synthetic(n, 7)
    sv, net, adj, deg = fo.helpers(x)
    z = fpn.initial_agg(sv, k_taps)
    err = np.zeros((n, k_taps, 6))
    svs, nets, zs, errs = [sv.astype(np.float32)], [net], [z], [err]
    for t in range(steps):
        x = fo.integrate(x, fo.controller(x))
        sv, net, adj, deg = fo.helpers(x)
        z, bound = fpn.next_taps(z, sv.astype(np.float32), adj, deg)
        nerr = np.zeros_like(err)
        for k in range(1, k_taps):
            nerr[:, k] = net @ err[:, k - 1] + bound[:, k]
        err = nerr
        svs.append(sv.astype(np.float32)), nets.append(net), zs.append(z), errs.append(err)
    seen = 0
    for t in range(1, steps + 1):
        for k in range(1, k_taps):
            if t - k < 0:
                np.testing.assert_array_equal(zs[t][:, k], 0.0)
                continue
            prod = svs[t - k].astype(np.float64)
            for s in range(t - k + 1, t + 1):
                prod = nets[s] @ prod
            assert (np.abs(zs[t][:, k] - prod) <= errs[t][:, k]).all(), (t, k)
            seen += 1
    assert seen > 10


def test_float32_network_is_close_to_the_float64_product():
    """Per layer, on the same float32 inputs: within width * 2^-23 * sum_i |w[o, i] * x[i]| of
    the float64 product (width products and width sums, half an ulp each)."""
    ws, bs = fpn.make_policy(WIDTHS, seed=5)
    z = np.random.RandomState(1).uniform(-2.0, 2.0, size=(50, 24)).astype(np.float32)
    x32 = z
    for l, (w, b) in enumerate(zip(ws, bs)):
        out32 = fpn.mlp(x32, [w], [b])  # one layer: no ReLU
        x64, w64 = x32.astype(np.float64), w.astype(np.float64)
        out64 = x64 @ w64.T + b.astype(np.float64)
        mag = np.abs(x64) @ np.abs(w64).T
        assert (np.abs(out32 - out64) <= w.shape[1] * 2.0 ** -23 * mag).all(), l
        if l < len(ws) - 1:
            x32 = np.where(out32 > 0, out32, np.float32(0))
    fpn.same_f32(fpn.mlp(z, ws, bs), out32, "the layers one by one")
    assert np.abs(out32 - fpn.mlp_f64(z, ws, bs)).max() < 1e-4


def test_relu_and_clip():
    w = [np.array([[1, 0, 0, 0, 0, 0], [-1, 0, 0, 0, 0, 0], [0, 1, 0, 0, 0, 0], [0, 0, 0, 0, 0, 0]], np.float32),
         np.array([[1, 0, 0, 0], [0, 1, 1, 1]], np.float32)]
    b = [np.array([0, 0, 0, -0.0], np.float32), np.zeros(2, np.float32)]
    z = np.array([[2.5, 3.0, 0, 0, 0, 0], [-2.5, -3.0, 0, 0, 0, 0]], np.float32)
    out = fpn.mlp(z, w, b)
    np.testing.assert_array_equal(out, np.array([[2.5, 3.0], [0.0, 2.5]], np.float32))
    out = fpn.mlp(z, w, b, clip=1.0)
    np.testing.assert_array_equal(out, np.array([[1.0, 1.0], [0.0, 1.0]], np.float32))
    neg = fpn.mlp(z, [np.array([[-1, 0, 0, 0, 0, 0], [0, -1, 0, 0, 0, 0]], np.float32)], [np.zeros(2, np.float32)], clip=2.0)
    np.testing.assert_array_equal(neg, np.array([[-2.0, -2.0], [2.0, 2.0]], np.float32))


def test_chosen_weights_and_inputs_stay_normal():
    """The GPU tests' networks (uniform in +-0.3 and +-0.01, seeded) on an oracle rollout: the
    restatement asserts that no product or partial sum is subnormal (check_normal)."""
    x0 = np.stack([synthetic(20, 90)])
    used = np.zeros((6, 1), bool)
    fpn.rollout_batch(x0, 6, *fpn.make_policy((24, 64, 64, 2), 1), 4, used, clip=1.0, check_normal=True)
    fpn.rollout_batch(x0, 6, *fpn.make_policy((24, 64, 64, 2), 2, scale=0.01), 4, used, check_normal=True)
    with pytest.raises(AssertionError):
        fpn.mlp(np.full((1, 6), 1e-30, np.float32), [np.full((2, 6), 1e-10, np.float32)], [np.zeros(2, np.float32)])


def test_check_recording_accepts_its_own_recording(own_recording):
    check(own_recording[5], own_recording)


def corrupted(own, name, index, bump):
    rec = {k: v.copy() for k, v in own[5].items()}
    rec[name][index] = bump(rec[name][index])
    return rec


def test_check_recording_rejects_a_policy_output_one_ulp_off(own_recording):
    rec = corrupted(own_recording, "policy", (3, 1, 5, 0), lambda v: np.nextafter(v, np.float32(np.inf)))
    with pytest.raises(AssertionError):
        check(rec, own_recording)


def test_check_recording_rejects_a_flipped_used_expert(own_recording):
    rec = corrupted(own_recording, "used_expert", (4, 0), lambda v: 1 - v)
    with pytest.raises(AssertionError):
        check(rec, own_recording)


def test_check_recording_rejects_a_tap_four_ulp_off(own_recording):
    base = own_recording[5]["agg"]
    idx = np.unravel_index(np.argmax(np.abs(base[5, 1, :, 2, :])), base[5, 1, :, 2, :].shape)
    index = (5, 1, idx[0], 2, idx[1])
    assert base[index] != 0

    def bump(v):
        for _ in range(4):
            v = np.nextafter(v, np.float32(np.inf))
        return v
    rec = corrupted(own_recording, "agg", index, bump)
    with pytest.raises(AssertionError):
        check(rec, own_recording)


def test_check_recording_rejects_an_applied_entry_one_ulp_off(own_recording):
    rec = corrupted(own_recording, "applied", (2, 0, 7, 1), lambda v: np.nextafter(v, np.inf))
    with pytest.raises(AssertionError):
        check(rec, own_recording)


def test_struct_sizes():
    assert ctypes.sizeof(nat.FePolicy) == 88
    assert ctypes.sizeof(nat.FePolicyRollout) == 88


NEW_SYMBOLS = ("fe_set_policy", "fe_reset_aggregation", "fe_get_aggregation", "fe_step_policy")


def test_new_symbols_are_declared_and_bound():
    with open(os.path.join(ROOT, "include", "gymflock.h")) as f:
        header = f.read()
    for name in NEW_SYMBOLS:
        assert re.search(r"\bint\s+%s\s*\(" % name, header), name
        assert name in nat.SIGNATURES, name
    for name in ("fe_policy", "fe_policy_rollout"):
        assert re.search(r"}\s*%s\s*;" % name, header), name
    assert "#define GF_ABI_VERSION 1" in header
    for method in ("set_policy", "step_policy", "aggregation", "reset_aggregation"):
        assert hasattr(nat.FlockHandle, method), method
    from gym_flock.vec import VecFlockingRelative
    for method in ("set_policy", "policy_steps", "aggregation", "reset_aggregation"):
        assert hasattr(VecFlockingRelative, method), method
