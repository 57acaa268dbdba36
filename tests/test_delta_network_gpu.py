"""The delta network store (fe_set_network_store): after every step or
compute_helpers the handle's dense network is, bit for bit, what a full store leaves
there, through every interleaving of API calls that can come between two plain steps.

Every check compares the whole h.network() bitwise with the oracle's
step(...)["network"].astype(float32) (small shapes) and with a second handle set to
FE_NET_FULL that is driven through the same calls (every shape)."""
import ctypes

import numpy as np
import pytest

from gym_flock import _native as nat
from gym_flock.init_states import synthetic_batch
from oracle import flocking as orc

pytestmark = pytest.mark.gpu

VEC_SHAPES = [(3, 8), (3, 68), (3, 132), (2, 1024), (2, 1028)]  # (B, N), N % 4 == 0: the delta form
SCALAR_SHAPES = [(2, 10), (1, 1030)]                              # N % 4 != 0: stays full
SMALL = [(3, 8), (3, 68), (3, 132)]
ORACLE_MAX_N = 132  # the oracle's dense float64 pair arrays: small shapes only


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def assert_same_bits(got, want, what=""):
    g, w = bits(got), bits(want)
    if not np.array_equal(g, w):
        bad = np.argwhere(g != w)
        raise AssertionError("%s: %d of %d floats differ, first at %s: got %r want %r"
                             % (what, len(bad), g.size, tuple(bad[0]), got[tuple(bad[0])], want[tuple(bad[0])]))


class Pair:
    """A delta handle and a full handle driven through the same calls."""

    def __init__(self, B, N, seed=0, **kw):
        self.B, self.N = B, N
        self.cr, self.mp = kw.get("comm_radius", 0.9), kw.get("mean_pooling", True)
        self.d = nat.FlockHandle(N, B, **kw)
        self.f = nat.FlockHandle(N, B, **kw)
        self.d.set_network_store(nat.FE_NET_DELTA)
        self.f.set_network_store(nat.FE_NET_FULL)
        self.rs = np.random.RandomState(1000 + seed)
        self.set_state(synthetic_batch(B, N, seed0=seed))

    def both(self):
        return (self.d, self.f)

    def close(self):
        for h in self.both():
            h.close()

    def set_state(self, x):
        for h in self.both():
            h.set_state(x)

    def actions(self, scale=1.0):
        return (scale * self.rs.uniform(-1, 1, size=(self.B, self.N, 2))).astype(np.float32)

    def step(self, flags=0, u=None, check=True, scale=1.0):
        u = self.actions(scale) if u is None else u
        own_u = not (flags & nat.FE_U_EXPERT)  # (else the oracle checks the new state's network)
        x0 = self.d.get_state() if (check and own_u and self.N <= ORACLE_MAX_N) else None
        for h in self.both():
            h.step(u, flags)
        if check:
            self.check(x0, u)

    def helpers(self, flags=0, check=True):
        for h in self.both():
            h.compute_helpers(flags)
        if check:
            self.check()

    def check(self, x0=None, u=None):
        """The delta handle's whole network against the full handle's and, at small
        shapes, the oracle's (of the step from x0 with u, or of the current state)."""
        got = self.d.network()
        assert_same_bits(got, self.f.network(), "delta vs FE_NET_FULL handle")
        np.testing.assert_array_equal(self.d.get_state(), self.f.get_state())
        if self.N <= ORACLE_MAX_N:
            for b in range(self.B):
                if x0 is not None:
                    ref = orc.step(x0[b], u[b], comm_radius=self.cr, mean_pooling=self.mp)["network"]
                else:
                    ref = orc.helpers(self.d.get_state(b), self.cr, self.mp)[1]
                assert_same_bits(got[b], ref.astype(np.float32), "delta vs oracle, env %d" % b)


@pytest.fixture
def pair():
    made = []

    def make(B, N, **kw):
        made.append(Pair(B, N, **kw))
        return made[-1]

    yield make
    for p in made:
        p.close()


# 1 ------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,N", VEC_SHAPES + SCALAR_SHAPES)
def test_eight_ordinary_steps(pair, B, N):
    p = pair(B, N, seed=11)
    for _ in range(8):
        p.step()


def test_prefetching_instantiation_two_steps(pair):
    p = pair(1, 8192, seed=12)
    for _ in range(2):
        p.step()


# 2 ------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,N", VEC_SHAPES)
def test_helpers_twice_then_step(pair, B, N):
    p = pair(B, N, seed=21)
    p.helpers()
    p.helpers()  # same state: nothing changes, nothing to store
    p.step()
    p.helpers()


# 3 ------------------------------------------------------------------------------------
def line_state(N, gap):
    """Agents on a line `gap` apart, at rest."""
    x = np.zeros((N, 4))
    x[:, 0] = np.arange(N) * gap
    return x


@pytest.mark.parametrize("B,N", SMALL + [(2, 1024)])
def test_set_state_full_rows_then_empty_rows(pair, B, N):
    p = pair(B, N, seed=31)
    p.helpers()
    near = np.zeros((B, N, 4))
    near[:, :, 0] = np.arange(N) * (0.5 / N)       # all within the radius: full rows
    p.set_state(near)
    p.helpers()
    far = np.stack([line_state(N, 2.0)] * B)       # dispersed: no row keeps a neighbour
    p.set_state(far)
    p.helpers()
    assert not p.d.network().any()  # deg == 0 rows: value 1, no bits, all zeros
    p.set_state(near)
    p.helpers()
    p.step()


@pytest.mark.parametrize("B,N", SMALL)
def test_set_state_value_only_and_group_back_to_zero(pair, B, N):
    p = pair(B, N, seed=32)
    # agents 0..3 close together (one 16-byte group of row 0), agent N-1 also near agent 0
    # but alone in its group, everyone else far away
    x = np.stack([line_state(N, 3.0)] * B)
    x[:, 0:4, 0] = [0.0, 0.1, 0.2, 0.3]
    x[:, 0:4, 1] = 100.0
    x[:, N - 1, 0:2] = [0.15, 100.4]
    p.set_state(x)
    p.helpers()
    # agent 3 leaves: the group of rows 0..2 that holds agent N-1 keeps its bits, only its
    # value 1/deg changes
    x1 = x.copy()
    x1[:, 3, 1] = 200.0
    p.set_state(x1)
    p.helpers()
    # agent N-1 leaves: it was alone in its group of rows 0..2, which return to zero
    x2 = x1.copy()
    x2[:, N - 1, 1] = 300.0
    p.set_state(x2)
    p.helpers()
    assert not p.d.network()[:, 0, N - 4:].any()
    p.set_state(x)
    p.helpers()


# 4 ------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,N", SMALL + [(2, 1024)])
def test_no_network_steps_between_delta_steps(pair, B, N):
    p = pair(B, N, seed=41)
    p.step()
    p.step()
    adj0 = p.d.network() > 0
    for _ in range(12):  # the buffer is left alone while the adjacency moves on
        p.step(nat.FE_NO_NETWORK, check=False)
    p.step()
    assert ((p.d.network() > 0) != adj0).any(), "the adjacency did not change: the case tests nothing"
    p.step()


# 5 ------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,N", [(3, 68), (2, 1024)])
def test_step_host_page_locked_and_pageable_network(pair, B, N):
    p = pair(B, N, seed=51)
    p.step()
    pool = nat.HostPool()
    for pinned in (True, False, True):
        u = p.actions()
        outs = []
        for h in p.both():
            if pinned:  # the kernel writes the network to the host array: the device buffer stays
                net, addr = pool.array_addr((B, N, N), np.float32)
                assert addr is not None
            else:       # through the device buffer, then a copy
                net = np.empty((B, N, N), np.float32)
                addr = net.ctypes.data
            rew = np.empty(B)
            h.step_host(u.ctypes.data, False, None, addr, rew.ctypes.data, None)
            h.sync()
            outs.append(net)
        assert_same_bits(outs[0], outs[1], "step_host network (pinned=%s)" % pinned)
        p.step()
        p.step()


# 6 ------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,N", SMALL + [(2, 1024)])
def test_controller_and_packed_steps_interleaved(pair, B, N):
    p = pair(B, N, seed=61)
    p.step()
    p.step(nat.FE_WITH_CONTROLLER)
    p.step()
    p.step()
    p.step(nat.FE_PACKED_NETWORK)
    p.step()
    p.step(nat.FE_PACKED_NETWORK | nat.FE_NO_NETWORK, check=False)
    p.step()
    p.helpers(nat.FE_WITH_CONTROLLER)
    p.step(nat.FE_U_EXPERT)  # a plain step whose actions are the controller's output
    p.step()


@pytest.mark.parametrize("B,N", [(3, 68), (3, 132), (2, 1024)])
def test_knn_steps_interleaved(pair, B, N):
    p = pair(B, N, seed=62, n_neighbors=7)
    p.step()
    p.step(nat.FE_WITH_KNN)
    p.step()
    p.step()
    p.step(nat.FE_WITH_KNN)
    p.step(nat.FE_WITH_KNN)
    p.step()


# 7 ------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,N", SMALL + [(2, 1024)])
def test_set_params_mid_run(pair, B, N):
    p = pair(B, N, seed=71)
    p.step()
    p.step()
    for cr, mp in ((0.9, False), (1.4, False), (1.4, True), (0.6, True)):
        for h in p.both():
            h.set_params(cr, 0.01, 10.0, mp, True)
        p.cr, p.mp = cr, mp
        p.step()
        p.step()


# 8 ------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,N", [(3, 8), (3, 132), (2, 1024)])
def test_split_and_single_launch_steps_alternate(pair, B, N):
    p = pair(B, N, seed=81)      # both split (the default)
    q = pair(B, N, seed=81)      # both one launch per step
    for h in q.both():
        h.set_streams(1)
    for t in range(10):
        u = p.actions()
        if t == 4:
            for h in p.both():
                h.set_streams(1)
            for h in q.both():
                h.set_streams(2)
        if t == 7:
            for h in p.both():
                h.set_streams(2)
        chk = t % 3 != 1           # a getter between steps makes the next step one launch
        p.step(u=u, check=chk)
        q.step(u=u, check=chk)
        if chk:
            assert_same_bits(p.d.network(), q.d.network(), "split vs one-launch, step %d" % t)
            np.testing.assert_array_equal(p.d.get_state(), q.d.get_state())
            assert_same_bits(p.d.state_values(), q.d.state_values(), "state_values, step %d" % t)
    p.check()
    q.check()
    assert_same_bits(p.d.network(), q.d.network(), "split vs one-launch, end")


# 9 ------------------------------------------------------------------------------------
def hip_runtime():
    nat.load()
    with open("/proc/self/maps") as f:
        paths = {ln.split()[-1] for ln in f if "libamdhip64.so" in ln}
    assert paths, "libamdhip64 is not mapped after loading libgymflock"
    hip = ctypes.CDLL(sorted(paths)[0])
    hip.hipMemcpy.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int]
    return hip


@pytest.mark.parametrize("B,N", [(3, 68), (2, 1024)])
def test_buffer_overwritten_by_the_caller_then_touched(pair, B, N):
    hip = hip_runtime()
    p = pair(B, N, seed=91)
    p.step()
    p.step()
    junk = np.full((B, N, N), 7.5, np.float32)
    for h in p.both():
        h.sync()
        buf = h.device_buffers()
        assert hip.hipMemcpy(buf.network, junk.ctypes.data, junk.nbytes, 1) == 0  # host to device
        h.network_touched()
    assert_same_bits(p.d.network(), junk, "the caller's bytes are in the buffer")
    p.step()
    p.step()
    # a step that changes nothing after the overwrite must still restore every row
    for h in p.both():
        h.sync()
        assert hip.hipMemcpy(h.device_buffers().network, junk.ctypes.data, junk.nbytes, 1) == 0
        h.network_touched()
    p.helpers()


# 10 -----------------------------------------------------------------------------------
@pytest.mark.parametrize("B,N", [(3, 68), (2, 1024)])
def test_diag_network_fill_then_step(pair, B, N):
    p = pair(B, N, seed=101)
    p.step()
    p.step()
    for h in p.both():
        h.diag_fill(reps=1)
    assert (p.d.network() == 0.5).any(), "the fill did not reach the buffer"
    p.helpers()
    p.step()


# 11 -----------------------------------------------------------------------------------
@pytest.mark.parametrize("B,N", SMALL + [(2, 1024)])
def test_store_mode_switched_mid_run(pair, B, N):
    p = pair(B, N, seed=111)
    p.step()
    p.step()
    for mode in (nat.FE_NET_FULL, nat.FE_NET_DELTA, nat.FE_NET_FULL, nat.FE_NET_FULL, nat.FE_NET_DELTA):
        p.d.set_network_store(mode)
        p.step()
        p.step()
    with pytest.raises(nat.GymFlockError):
        p.d.set_network_store(2)


# 12 -----------------------------------------------------------------------------------
def test_variant_handle_is_unaffected(pair):
    B, N = 3, 68
    p = pair(B, N, seed=121)
    for h in p.both():
        h.set_variant(u_scale=1.0, n_frozen=4, n_vel_zero=4)
    for _ in range(3):
        p.step(check=False)
        assert_same_bits(p.d.network(), p.f.network(), "variant step")
    for h in p.both():
        h.clear_variant()
    p.step()  # plain again: the record is rebuilt
    p.step()


def test_drop_in_env_episode():
    import gym_flock
    env = gym_flock.make("FlockingRelative-v0")
    N = env.n_agents
    env.x = orc.synthetic_state(N, 5)
    rs = np.random.RandomState(6)
    for _ in range(10):
        x0 = np.array(env.x, dtype=np.float64)
        u = rs.uniform(-1, 1, size=(N, 2))
        (sv, net), _, _, _ = env.step(u)
        ref = orc.step(x0, u, comm_radius=env.comm_radius, dt=env.dt)
        np.testing.assert_array_equal(np.asarray(env.x), ref["x"])
        assert_same_bits(np.asarray(net), ref["network"].astype(np.float32), "drop-in episode")
