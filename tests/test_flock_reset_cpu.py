"""The NumPy restatement of reset()'s rejection loop (tests/flock_reset_numpy.py) against the
recorded fixture and the oracle, and the margin condition that lets the GPU tests
(test_flock_reset_gpu.py) compare acceptance decisions with a device whose cos / sin differ
from NumPy's in the last place. No kernel is launched here."""
import os
import sys

import numpy as np
import pytest

from conftest import GOLDEN

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import flock_reset_numpy as frn  # noqa: E402

from oracle import flocking as orc  # noqa: E402


def test_helper_reproduces_the_recorded_reset():
    """np.random.seed(11), N=64, r_max=8: the fixture's x0 bit for bit, after 169 tries."""
    f = np.load(os.path.join(GOLDEN, "flock_n64_reset.npz"))
    np.random.seed(int(f["seed"]))
    r = frn.reset_rejection(np.random, 64, r_max=float(f["r_max"]))
    assert r["accepted"] and r["tries"] == 169
    np.testing.assert_array_equal(r["x"], f["x0"])
    g = frn.golden_case(int(f["seed"]), 64, float(f["r_max"]))
    np.testing.assert_array_equal(g["x"], f["x0"])
    assert g["tries"] == 169


@pytest.mark.parametrize("n,seed", [(10, 3), (37, 2), (64, 11), (100, 7)])
def test_helper_equals_oracle_on_the_same_stream(n, seed):
    a = frn.reset_rejection(np.random.RandomState(seed), n)
    rs = np.random.RandomState(seed)
    x = orc.reset_rejection(n, r_max=np.sqrt(n), rng=rs)
    np.testing.assert_array_equal(a["x"], x)
    sa, sb = a["state"], rs.get_state()
    np.testing.assert_array_equal(sa[1], sb[1])
    assert sa[2] == sb[2]


def test_helper_cap_and_no_reject():
    """max_tries stops the loop on the last candidate with the stream after that many
    tries; reject=False is the synthetic init."""
    from gym_flock.init_states import synthetic_state
    r = frn.reset_rejection(np.random.RandomState(1), 10, max_tries=5)
    assert r["tries"] == 5 and not r["accepted"]  # seed 1 needs 127
    rs = np.random.RandomState(1)
    for _ in range(5):
        rs.uniform(size=42)  # 4N+2 doubles per try
    assert rs.get_state()[2] == r["state"][2]
    np.testing.assert_array_equal(rs.get_state()[1], r["state"][1])
    s = frn.reset_rejection(np.random.RandomState(17), 300, reject=False)
    np.testing.assert_array_equal(s["x"], synthetic_state(300, 17))


def _check(r, tries, what):
    assert r["tries"] == tries, what
    assert r["dist_margin"].min() >= frn.MARGIN, (what, r["dist_margin"].min())
    assert r["a_margin"].min() >= frn.MARGIN, (what, r["a_margin"].min())


@pytest.mark.parametrize("key", sorted(frn.CASES), ids=lambda k: "%s-n%d" % k[:2])
def test_gpu_cases_have_the_recorded_tries_and_wide_margins(key):
    """Every candidate of every stream the GPU tests use is decided with both margins at
    least 1e-12 (about a thousand times what a last-ulp difference of cos / sin moves
    a_ij), so device and NumPy must agree on each acceptance; the try counts are the
    recorded ones."""
    kind, n, max_tries = key
    for s, tries in frn.CASES[key].items():
        r = frn.case(kind, n, max_tries, s)
        _check(r, tries, (key, s))
        assert r["accepted"] == (max_tries != 8)
        if kind == "odd":
            assert frn.stream(kind, s).get_state()[2] % 2 == 1


def test_masked_and_drop_in_cases_have_wide_margins():
    for b in frn.MASKED["reset"]:
        r = frn.masked_case(b)
        assert r["accepted"]
        _check(r, r["tries"], ("masked", b))
    f = np.load(os.path.join(GOLDEN, "flock_n64_reset.npz"))
    _check(frn.golden_case(int(f["seed"]), 64, float(f["r_max"])), 169, "drop-in")
