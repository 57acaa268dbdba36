"""get_stats on the device (flock_stats_kernel, flock_stats_summary_kernel through
fe_get_stats_ex and fe_stats_summary) against oracle.flocking.stats and the adjacency row
sums of oracle.flocking.helpers, at the sizes and states where the kernel can go wrong:
N = 1 and 2, a ragged last workgroup (N % 256 != 0) in a batch whose grid is no multiple
of 8, more than one 1024-agent LDS tile, and degenerate states. Needs an MI355X.

Tolerances (tests/test_flock_gpu.py): vel_diffs rtol 1e-12, min_dists and degree
bit-exact, the summary rtol 1e-13. Where a case holds NaN by construction the NaN masks
must be equal and the tolerance applies to the other entries."""
import numpy as np
import pytest

from oracle import flocking as orc

pytestmark = pytest.mark.gpu

nat = pytest.importorskip("gym_flock._native")
from gym_flock.vec import VecFlockingRelative  # noqa: E402


WORST = {}  # rtol -> largest relative error seen, as a fraction of that tolerance


@pytest.fixture(scope="module", autouse=True)
def _report_worst():
    yield
    print("\nstats, largest error / tolerance:", {k: float("%.3g" % v) for k, v in sorted(WORST.items())})


def close_masked(ours, ref, rtol):
    """Equal NaN masks, and rtol on every other entry (infinities must be equal)."""
    ours, ref = np.asarray(ours), np.asarray(ref)
    np.testing.assert_array_equal(np.isnan(ours), np.isnan(ref))
    ok = np.isfinite(ref) & np.isfinite(ours) & (ref != 0)
    if ok.any():
        WORST[rtol] = max(WORST.get(rtol, 0.0), float((np.abs(ours[ok] - ref[ok]) / (rtol * np.abs(ref[ok]))).max()))
    ok = ~np.isnan(ref)
    np.testing.assert_allclose(ours[ok], ref[ok], rtol=rtol, atol=0)


def check_stats(h, b, x, comm_radius=0.9):
    """stats(b) of the handle against the oracle on the state x; returns the oracle's
    (mean vel_diffs, mean min_dists)."""
    with np.errstate(all="ignore"):
        st = orc.stats(x)
        deg = orc.helpers(x, comm_radius)[3]
        want = np.array([st["vel_diffs"].mean(), st["min_dists"].mean()])
    vd, md, dg = h.stats(b)
    close_masked(vd, st["vel_diffs"], 1e-12)
    np.testing.assert_array_equal(md, st["min_dists"])  # bit-exact, NaN and inf included
    assert dg.dtype == np.int32
    np.testing.assert_array_equal(dg, deg)
    return want


@pytest.mark.parametrize("n", [1, 2, 255, 256, 257, 1024, 1025, 2049])
def test_stats_sizes_vs_oracle(n):
    """B = 3 distinct synthetic states after one step: grids of 3, 6, 12, 15 and 27
    workgroups (none a multiple of 8), a last workgroup of 1, 2, 255 or 256 agents, and at
    N = 1025 and 2049 a second and third LDS tile of one agent."""
    B = 3
    v = VecFlockingRelative(B, n)
    x0 = np.stack([orc.synthetic_state(n, 400 + 7 * n + b) for b in range(B)])
    v.reset(x=x0)
    u = np.random.RandomState(n).uniform(-1, 1, size=(B, n, 2)).astype(np.float32)
    v.step(u, network=False)
    x1 = v.get_state()
    summ = v.stats_summary()
    assert summ.shape == (B, 2)
    for b in range(B):
        np.testing.assert_array_equal(x1[b], orc.integrate(x0[b], u[b]))
        want = check_stats(v, b, x1[b])
        close_masked(summ[b], want, 1e-13)
    if n == 1:  # no other agent: the reference's minimum over the infinite diagonal
        vd, md, dg = v.stats(0)
        assert vd[0] == 0.0 and md[0] == np.inf and dg[0] == 0
    v.close()


def _degenerate_cases():
    n = 300
    rs = np.random.RandomState(19)
    base = np.zeros((n, 4))
    base[:, :2] = rs.uniform(-6, 6, size=(n, 2))
    base[:, 2:] = rs.uniform(-2, 2, size=(n, 2))
    cases = {}
    x = base.copy()
    x[257, :2] = x[3, :2]  # a coincident pair, in two workgroups
    cases["coincident"] = (x, 0.9)
    x = base.copy()
    g = np.stack(np.meshgrid(np.arange(20), np.arange(15)), -1).reshape(-1, 2)
    x[:, :2] = g[rs.permutation(n)] * 0.5  # exact in float64: r2 = 0.25 is not < 0.5 * 0.5
    cases["lattice"] = (x, 0.5)
    x = base.copy()
    x[:, :2] += 3.0e5
    cases["offset"] = (x, 0.9)
    x = base.copy()
    x[5, 0] = np.inf
    cases["one_inf"] = (x, 0.9)
    x = base.copy()
    x[5, 0] = np.inf
    x[290, 0] = np.inf  # inf - inf: the pair's r2 is NaN
    cases["two_inf"] = (x, 0.9)
    x = base.copy()
    x[5, 1] = np.nan
    cases["nan_position"] = (x, 0.9)
    x = base.copy()
    x[5, 2] = np.nan
    cases["nan_velocity"] = (x, 0.9)
    return cases


DEGENERATE = _degenerate_cases()


@pytest.mark.parametrize("case", sorted(DEGENERATE))
def test_stats_degenerate_states(case):
    """np.min over the reference's r2 propagates NaN: one agent with a NaN position makes
    every agent's min_dists NaN, and two agents at +inf make each other's NaN. The degree
    never counts a NaN or an infinite r2, nor one equal to comm_radius**2."""
    x, cr = DEGENERATE[case]
    n = x.shape[0]
    h = nat.FlockHandle(n, 1, comm_radius=cr)
    h.set_state(x[None])
    want = check_stats(h, 0, x, cr)
    close_masked(h.stats_summary()[0], want, 1e-13)
    vd, md, dg = h.stats(0)
    if case == "coincident":
        assert md[3] == 0.0 and md[257] == 0.0
        r2 = np.sum((x[:, None, :2] - x[None, :, :2]) ** 2, axis=2)
        others = np.delete(np.arange(n), [3, 257])
        # each of the pair counts the other on top of the neighbours they share
        assert dg[3] == dg[257] == (r2[3, others] < cr * cr).sum() + 1
    elif case == "lattice":
        assert (dg == 0).all() and (md == 0.5).all()
    elif case == "one_inf":
        assert md[5] == np.inf and dg[5] == 0 and np.isfinite(np.delete(md, 5)).all()
    elif case == "two_inf":
        assert np.isnan(md[[5, 290]]).all() and np.isfinite(np.delete(md, [5, 290])).all()
    elif case == "nan_position":
        assert np.isnan(md).all() and dg[5] == 0 and np.isfinite(vd).all()
    elif case == "nan_velocity":
        assert np.isnan(vd).all() and np.isfinite(md).all()
    h.close()


def test_stats_after_split_step_match_single_stream():
    """Stats taken right after a step that went out as two half-batch launches on two
    streams wait for both halves: the same bits as after the same step on one stream, and
    the oracle's values."""
    B, n = 5, 257
    x0 = np.stack([orc.synthetic_state(n, 900 + b) for b in range(B)])
    rs = np.random.RandomState(901)
    us = [rs.uniform(-1, 1, size=(B, n, 2)).astype(np.float32) for _ in range(3)]
    outs = []
    for streams in (2, 1):
        v = VecFlockingRelative(B, n)
        v.h.set_streams(streams)
        v.reset(x=x0)
        for u in us:  # back to back: with two streams the second and third are split
            v.step(u, network=False)
        got = [v.stats_summary()] + [a for b in range(B) for a in v.stats(b)] + [v.get_state()]
        if streams == 2:
            for b in range(B):
                want = check_stats(v, b, got[-1][b])
                np.testing.assert_allclose(got[0][b], want, rtol=1e-13, atol=0)
        outs.append(got)
        v.close()
    for a, b in zip(*outs):
        np.testing.assert_array_equal(a, b)
