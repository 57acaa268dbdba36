"""The large Coverage maps' inputs, without a GPU: the recorded ExploreFullEnv pool
(tests/golden/coverage_explore_full.npz, made by tests/golden/make_golden_explore_full.py)
and the walled grids of tests/test_coverage_large_gpu.py against the NumPy restatement of
the occupancy pool (tests/coverage_arl_numpy.py), and the pool cap the bindings state."""
import os
import sys

import numpy as np
import pytest

from conftest import GOLDEN

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import coverage_arl_numpy as an  # noqa: E402
from coverage_large_inputs import WALLED, walled_grid, walled_pool, walled_reference  # noqa: E402


def test_recorded_full_pool_is_the_restatement():
    grid = np.load(os.path.join(GOLDEN, "grid_slice10.npy"))
    f = np.load(os.path.join(GOLDEN, "coverage_explore_full.npz"))
    raw, pool, lo, hi, sub = an.load_graph(grid, 5.5, perimeter_delta=12.0, num_subgraphs=1)
    assert len(raw) == 5855 and len(pool) == 5659
    assert int(f["n_targets"]) == 5659 and int(f["max_nodes"]) == 5759 and int(f["n_robots"]) == 100
    np.testing.assert_array_equal(f["targets"], pool)
    np.testing.assert_array_equal(f["x0"][100:, :2], pool)
    # the digest's shape: every source, and 8 full rows from the first to the last source
    assert f["tm_count"].shape == f["tm_sum"].shape == (5659,)
    assert f["tm_cost_rows"].shape == f["tm_prev_rows"].shape == (8, 5659)
    assert f["tm_rows"][0] == 0 and f["tm_rows"][-1] == 5658 and (np.diff(f["tm_rows"]) > 0).all()
    assert os.path.getsize(os.path.join(GOLDEN, "coverage_explore_full.npz")) < 300 * 1024


@pytest.mark.parametrize("block,pool_size", sorted(WALLED.items()))
def test_walled_grids_give_the_stated_pools(block, pool_size):
    """All ones with an a x b block of zeros inside, perimeter_delta = max(a, b) + 2: every
    free cell is kept and the pool is the block's lattice, one component. The grid one past
    the cap is checked before the component step only (the device refuses it from the count
    of kept cells), and with the restatement's window cut to 2 cells: its loop over the
    (2 * 2733 + 1)^2 offsets takes minutes, the kept set only grows with perimeter_delta, and
    at 2 (every free cell of the 3-cell corridor is at most 2 from a wall) it already holds
    every free cell, which no larger perimeter_delta can exceed."""
    g = walled_grid(*block)
    assert g.shape == (block[0] + 2, block[1] + 2)
    if pool_size <= 8192:
        raw, pool, lo, hi, sub = walled_reference(*block)
        assert len(pool) == pool_size
        np.testing.assert_array_equal(pool, raw)
    else:
        raw = an.occupancy_targets(g, perimeter_delta=2.0)
        assert len(raw) == int((g == 0).sum())
    assert len(raw) == pool_size == block[0] * block[1]
    np.testing.assert_array_equal(raw, walled_pool(*block))


def test_bindings_state_the_pool_cap():
    src = open(os.path.join(os.path.dirname(GOLDEN), "..", "include", "gymflock.h")).read()
    assert "#define COV_POOL_CAP      8192" in src
    from gym_flock import _native
    assert _native.COV_POOL_CAP == 8192


def test_tm_plan_refuses_a_null_handle():
    from gym_flock import _native
    lib = _native.load()
    assert lib.cov_set_tm_plan(None, 0, 0) == _native.GF_EINVAL
    assert b"null handle" in lib.fe_last_error()
