"""The compacted drain of the delta network store ("Compacted drain"): a
handle that stores deltas and a handle set to FE_NET_FULL are driven through the same
calls, and after every call the delta handle's whole dense network must equal the full
handle's bit for bit and, at N <= 132, the oracle's.

The shapes cover one float4 pair per row with many rows per batch (N=8), a last word of
4 bits (68, 132), the bench's row (1024), a row stride that is no multiple of 64 bytes with
a last group of one float4 (1028) and the smallest N whose rows take more than one batch
(4100: 65 words, the last chunk holds one). The sequences cover an empty list, a list of
all 256 entries and the dense branch, a share in between, a value-only change and the
forced launch after a full store."""
import numpy as np
import pytest

from gym_flock import _native as nat
from gym_flock.init_states import synthetic_batch
from oracle import flocking as orc

pytestmark = pytest.mark.gpu

SHAPES = [(3, 8), (3, 68), (3, 132), (2, 1024), (2, 1028), (1, 4100)]
ORACLE_MAX_N = 132
FAR = 1.0e3  # a comm_radius beyond any swarm's diameter here: every pair adjacent


def as_bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def same_bits(got, want, what):
    g, w = as_bits(got), as_bits(want)
    if not np.array_equal(g, w):
        where = np.argwhere(g != w)
        first = tuple(where[0])
        raise AssertionError("%s: %d of %d floats differ, first at %s: got %r, want %r"
                             % (what, len(where), g.size, first, got[first], want[first]))


class Twin:
    """The delta handle `d` and the full handle `f`, always given the same calls."""

    def __init__(self, B, N, seed, comm_radius=0.9):
        self.B, self.N, self.cr = B, N, comm_radius
        self.d = nat.FlockHandle(N, B, comm_radius=comm_radius)
        self.f = nat.FlockHandle(N, B, comm_radius=comm_radius)
        self.d.set_network_store(nat.FE_NET_DELTA)
        self.f.set_network_store(nat.FE_NET_FULL)
        self.rs = np.random.RandomState(77 + seed)
        self.calls = 0
        self.set_state(synthetic_batch(B, N, seed0=seed))

    def close(self):
        self.d.close()
        self.f.close()

    def set_state(self, x):
        self.d.set_state(x)
        self.f.set_state(x)

    def set_radius(self, cr):
        for h in (self.d, self.f):
            h.set_params(cr, 0.01, 10.0, True, True)
        self.cr = cr

    def random_actions(self):
        return self.rs.uniform(-1, 1, size=(self.B, self.N, 2)).astype(np.float32)

    def zero_actions(self):
        return np.zeros((self.B, self.N, 2), np.float32)

    def step(self, u=None, flags=0):
        """One step of both handles, then the whole network compared. Returns it."""
        u = self.random_actions() if u is None else u
        x0 = self.d.get_state() if self.N <= ORACLE_MAX_N else None
        self.d.step(u, flags)
        self.f.step(u, flags)
        self.calls += 1
        what = "call %d (B=%d, N=%d)" % (self.calls, self.B, self.N)
        got = self.d.network()
        same_bits(got, self.f.network(), what + ": delta handle against FE_NET_FULL handle")
        np.testing.assert_array_equal(self.d.get_state(), self.f.get_state())
        if x0 is not None:
            for b in range(self.B):
                ref = orc.step(x0[b], u[b], comm_radius=self.cr)["network"].astype(np.float32)
                same_bits(got[b], ref, what + ": delta handle against the oracle, env %d" % b)
        return got


@pytest.fixture
def twin():
    made = []

    def make(*a, **kw):
        made.append(Twin(*a, **kw))
        return made[-1]

    yield make
    for t in made:
        t.close()


def at_rest(x):
    x = np.array(x, dtype=np.float64)
    x[..., 2:] = 0.0
    return x


@pytest.mark.parametrize("B,N", SHAPES)
def test_eight_ordinary_steps(twin, B, N):
    t = twin(B, N, seed=1)
    for _ in range(8):
        t.step()


@pytest.mark.parametrize("B,N", SHAPES)
def test_nothing_moves_empty_drain(twin, B, N):
    t = twin(B, N, seed=2)
    t.set_state(at_rest(t.d.get_state()))
    first = t.step(t.zero_actions())  # the forced launch that fills the record
    for _ in range(2):                # no group is dirty: nothing to list, nothing to store
        again = t.step(t.zero_actions())
        same_bits(again, first, "a step at rest")
    t.step()


@pytest.mark.parametrize("B,N", SHAPES)
def test_every_group_dirty_and_back(twin, B, N):
    t = twin(B, N, seed=3, comm_radius=FAR)
    t.set_state(at_rest(t.d.get_state()))
    dense = t.step(t.zero_actions())
    assert np.count_nonzero(dense) == B * N * (N - 1), "not an all-adjacent network: the case tests nothing"
    t.step(t.zero_actions())          # a delta step over full rows with nothing to do
    t.set_radius(0.9)
    sparse = t.step(t.zero_actions())  # every group held 16 (or the row's last) bits and loses most
    if N > 8:
        assert np.count_nonzero(sparse) < B * N * (N - 1) // 4
    t.set_radius(FAR)
    same_bits(t.step(t.zero_actions()), dense, "back to the all-adjacent network")
    t.set_radius(0.9)
    same_bits(t.step(t.zero_actions()), sparse, "and sparse again")
    t.step()


@pytest.mark.parametrize("B,N", SHAPES)
def test_unrelated_swarm_by_set_state(twin, B, N):
    t = twin(B, N, seed=4)
    t.step()
    t.step()
    t.set_state(synthetic_batch(B, N, seed0=400))
    t.step()
    t.step()


@pytest.mark.parametrize("B,N", SHAPES)
def test_value_only_change(twin, B, N):
    t = twin(B, N, seed=5)
    t.set_state(at_rest(t.d.get_state()))
    before = t.step(t.zero_actions())
    t.step(t.zero_actions())
    # the last agent lands beside agent 0: the rows of agent 0's neighbourhood gain one
    # neighbour, so their 1/deg changes while all their other bits stay
    x = t.d.get_state()
    x[:, N - 1, 0:2] = x[:, 0, 0:2] + [0.03, 0.04]
    t.set_state(x)
    after = t.step(t.zero_actions())
    assert after[0, 0, N - 1] > 0
    if N > 8:
        kept = (before[0, 0, :N - 1] > 0) & (after[0, 0, :N - 1] > 0)
        assert kept.any() and (after[0, 0, :N - 1][kept] != before[0, 0, :N - 1][kept]).all(), \
            "row 0 kept no bit with a new value: the case tests nothing"
    t.step()


@pytest.mark.parametrize("B,N", SHAPES)
def test_controller_step_then_forced_then_delta(twin, B, N):
    t = twin(B, N, seed=6)
    t.step()
    t.step()
    t.step(flags=nat.FE_WITH_CONTROLLER)  # stores in full and clears the record
    t.step()                              # forced: every group, the whole record
    t.step()                              # delta again
    t.step()
