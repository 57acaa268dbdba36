"""CPU side of the closed-loop expert rollout (fe_step_expert): the NumPy restatement the
GPU tests compare against (tests/flock_rollout_numpy.py) checked on the reference's own
golden episode, the parity protocol's own sharpness, and the binding's layout. No kernel
is launched here."""
import ctypes
import os
import re
import types

import numpy as np
import pytest

from conftest import GOLDEN, ROOT
from oracle import flocking as fo

import flock_rollout_numpy as frn


@pytest.fixture(scope="module")
def episode():
    return np.load(os.path.join(GOLDEN, "flock_n10_episode.npz"))


def test_restatement_follows_the_reference_episode(episode):
    """The golden episode opens with 20 expert steps. The restatement's free run from x0
    reproduces their adjacency exactly (the nearest pair stays 1.76e-3 from either
    threshold) and their states within 10 x the free-run sensitivity (the bound the GPU
    test uses; the oracle itself sits ~2e-16 away)."""
    f = episode
    rec = frn.rollout(f["x0"], 20)
    for t in range(20):
        np.testing.assert_array_equal(frn.unpack_bits(rec["adj_bits"][t], 10), f["net"][t] > 0)
        np.testing.assert_array_equal(rec["degree"][t], (f["net"][t] > 0).sum(axis=1))
    sens = frn.free_run_sensitivity(f)
    dev = float(np.abs(rec["x"] - f["x"][:20]).max())
    margin = min(float(np.abs(fo.pair_geometry(f["x"][t])[4] - thr).min()) for t in range(20) for thr in (0.81, 0.9))
    print("free-run sensitivity %.3e, restatement's deviation %.3e, threshold margin %.3e" % (sens, dev, margin))
    assert 0 < sens < 1e-6  # a tolerance-sized push stays tolerance-sized over 20 steps
    assert dev <= 10 * sens
    np.testing.assert_allclose(rec["controls"][:19], f["u"][1:20], rtol=1e-9, atol=1e-12)
    np.testing.assert_allclose(rec["rewards"], f["reward"][:20], rtol=1e-12)
    np.testing.assert_allclose(rec["state_values"], f["sv"][:20], rtol=1e-5, atol=1e-9)


def test_restatement_records_every_kth_step_and_every_reward():
    x0 = fo.synthetic_state(65, 3)
    full = frn.rollout(x0, 10)
    part = frn.rollout(x0, 10, every=5)
    for k in ("x", "state_values", "adj_bits", "degree", "controls"):
        assert part[k].shape[0] == 2
        np.testing.assert_array_equal(part[k], full[k][[4, 9]])
    np.testing.assert_array_equal(part["rewards"], full["rewards"])
    assert full["rewards"].shape == (10,)


@pytest.mark.parametrize("n", [1, 63, 64, 65, 130])
def test_bit_packing_round_trip(n):
    adj = np.random.RandomState(n).uniform(size=(n, n)) < 0.3
    bits = frn.pack_bits(adj)
    assert bits.shape == (n, (n + 63) // 64) and bits.dtype == np.uint64
    np.testing.assert_array_equal(frn.unpack_bits(bits, n), adj)
    if n % 64:  # no bit past column N - 1
        assert not (bits[:, -1] >> np.uint64(n % 64)).any()


def test_parity_protocol_accepts_the_restatement_and_sees_one_ulp():
    """check_recording on the restatement's own recording passes; a state entry moved by
    one ulp, one flipped adjacency bit or a control off by 1e-8 relative fails it."""
    B, n = 2, 20
    x0 = np.stack([fo.synthetic_state(n, 40 + b) for b in range(B)])
    u0 = np.stack([fo.controller(x0[b]) for b in range(B)])
    recs = [frn.rollout(x0[b], 4) for b in range(B)]
    rec = {k: np.stack([r[k] for r in recs], axis=1) for k in frn.RECORDS}
    frn.check_recording(rec, x0, u0)

    def broken(key, idx, fn):
        bad = {k: v.copy() for k, v in rec.items()}
        bad[key][idx] = fn(bad[key][idx])
        with pytest.raises(AssertionError):
            frn.check_recording(bad, x0, u0)

    broken("x", (2, 1, 7, 0), lambda v: np.nextafter(v, np.inf))
    broken("adj_bits", (1, 0, 3, 0), lambda v: v ^ np.uint64(1 << 5))
    broken("degree", (3, 1, 0), lambda v: v + 1)
    # an unclipped control entry (|u| < 1): off by 1e-8 relative
    free = np.argwhere(np.abs(rec["controls"]) < 0.99)
    assert len(free)
    broken("controls", tuple(free[0]), lambda v: v * (1 + 1e-8) + 1e-11)
    broken("rewards", (0, 0), lambda v: v * (1 + 1e-11))


def test_binding_matches_the_header():
    from gym_flock import _native as nat
    txt = open(os.path.join(ROOT, "include", "gymflock.h")).read()
    body = re.search(r"typedef struct fe_rollout \{(.*?)\} fe_rollout;", txt, re.S).group(1)
    names = re.findall(r"^\s*\w+\*?\s+(\w+);", body, re.M)
    assert names == [f[0] for f in nat.FeRollout._fields_]
    assert ctypes.sizeof(nat.FeRollout) == 6 * 8 + 2 * 4
    assert "fe_step_expert" in nat.SIGNATURES
    assert int(re.search(r"#define FE_ROLLOUT_DEVICE\s+(\w+)", txt).group(1), 0) == nat.FE_ROLLOUT_DEVICE
    shapes = nat.FlockHandle.rollout_shapes(types.SimpleNamespace(n_envs=3, n_agents=65), 10, 5)
    assert shapes["x"] == ((2, 3, 65, 4), np.float64)
    assert shapes["adj_bits"] == ((2, 3, 65, 2), np.uint64)
    assert shapes["rewards"] == ((10, 3), np.float64)
    assert set(shapes) == set(frn.RECORDS)


def test_null_handle_is_refused_before_any_device_work():
    from gym_flock import _native as nat
    lib = nat.load()
    assert lib.fe_step_expert(None, 1, None) == nat.GF_EINVAL
