"""NumPy / plain-Python restatement of what gym-flock_amd/csrc/flock_dt_noise.hip does on an
env's MT19937 stream, with state, for the tests of fe_set_dt_noise and fe_reset_variant:

  Stream          RandomState's generator with its cached Gaussian: random_sample (two
                  tempered words, the first carried across a key regeneration), legacy_gauss
                  and legacy_normal, word by word as the kernel draws them.
  grid resets     the two flocks' and the obstacle course's reset as the kernel computes
                  them, agent by agent.
  leader_reset    the relative rejection reset (flock_reset_numpy) and the leaders' draw.
  tolerances      the bound on a device dt against NumPy's, and the sensitivity D of the
                  closed-loop oracle rollout to dts moved by that bound.

The device's log may differ from the host's in the last places; everything else in a dt
(uniforms, rejection test, division, square root) is exact. dt_bound assumes a log within
3 ulp (OpenCL's double-precision bound) and one rounding each for f * x, sigma * g and the
sum: sigma * |g| * 4 * 2^-52 + 2^-53 * |dt|.
"""
import math

import numpy as np

import flock_reset_numpy as frn_reset
from oracle import flocking_variants as fv
from oracle import mt19937 as mt

MEAN, SIGMA = 0.12, 0.018  # flocking_stoch.py:20
STOCH = dict(u_scale=6.0, n_frozen=0, u_clip=0.5, x_scale=6.0)  # fv.integrate's switches (:20-22, :36)


class Stream:
    """(key, pos, has_gauss, gauss) of a legacy RandomState, advanced in plain Python."""

    def __init__(self, state):
        state = state.get_state() if hasattr(state, "get_state") else state
        assert state[0] == "MT19937"
        self.key = [int(k) for k in state[1]]
        self.pos = int(state[2])
        self.has_gauss = int(state[3]) if len(state) > 3 else 0
        self.gauss = float(state[4]) if len(state) > 4 else 0.0

    def word(self):
        if self.pos == mt.N:
            mt.regenerate(self.key)
            self.pos = 0
        w = mt.temper(self.key[self.pos])
        self.pos += 1
        return w

    def sample(self):
        a, b = self.word() >> 5, self.word() >> 6
        return (a * 67108864.0 + b) / 9007199254740992.0

    def gauss_next(self):
        if self.has_gauss:
            g, self.has_gauss, self.gauss = self.gauss, 0, 0.0
            return g
        while True:
            x1 = 2.0 * self.sample() - 1.0
            x2 = 2.0 * self.sample() - 1.0
            r2 = x1 * x1 + x2 * x2
            if not (r2 >= 1.0 or r2 == 0.0):
                break
        f = math.sqrt(-2.0 * math.log(r2) / r2)
        self.gauss, self.has_gauss = f * x1, 1
        return f * x2

    def normal(self, mean=MEAN, sigma=SIGMA):
        return mean + sigma * self.gauss_next()

    def uniform(self, lo, hi):
        return lo + (hi - lo) * self.sample()

    def state(self):
        return ("MT19937", np.array(self.key, np.uint32), self.pos, self.has_gauss, self.gauss)


def random_state(state):
    rs = np.random.RandomState()
    rs.set_state(state)
    return rs


# ----------------------------------------------------------------------------- resets
def grid_point(i, side, side2):
    """Agent i of utils.py:26-33 grid(n, side), x fastest."""
    return 0.8 * (float(i % side) - side / 2.0), 0.8 * (float(i // side) - side2 / 2.0)


def twoflocks_ok(n):
    side = n // 10
    return side >= 1 and side * (n // side) == n


def twoflocks_reset(stream, n, v_bias=5.0):
    """flocking_twoflocks.py:8-28 on a Stream (two uniforms), agent by agent."""
    lo, hi = -v_bias / 2.0, v_bias / 2.0
    b0, b1 = stream.uniform(lo, hi), stream.uniform(lo, hi)
    side = n // 10
    x = np.zeros((n, 4))
    for i in range(n):
        gx, gy = grid_point(i, side, n // side)
        x[i] = gx, gy, -gx + b0, -gy + b1
    return x


def obstacle_reset(n, n_obstacles=4):
    """flocking_obstacle.py:59-74, agent by agent."""
    x = np.zeros((n, 4))
    for i in range(n):
        gx, gy = grid_point(i, 5, n // 5)
        x[i] = gx, gy, 0.0, -7.0
        if i < n_obstacles:
            gx, gy = grid_point(i, 2, 2)
            x[i] = gx * 0.5, gy * 0.5 - 10.0, 0.0, 0.0
    return x


def leader_reset(rs, n, n_leaders=2, v_max=5.0, max_tries=None):
    """flocking_leader.py:37-41 on the RandomState rs: the relative reset's loop, then one
    uniform into both velocity components of the leaders. Returns reset_rejection's dict
    with x overridden, w and the stream afterwards."""
    out = frn_reset.reset_rejection(rs, n, v_max=v_max, max_tries=max_tries)
    w = rs.uniform(low=-v_max, high=v_max)
    out["x"][:n_leaders, 2:4] = w
    out["w"] = w
    out["state"] = rs.get_state()
    return out


# ------------------------------------------------------------------------- tolerances
def dt_bound(dt, mean=MEAN, sigma=SIGMA):
    """Largest |device dt - NumPy dt| (module docstring); dt may be an array."""
    dt = np.asarray(dt, np.float64)
    g = np.abs(dt - mean) / sigma if sigma > 0 else np.zeros_like(dt)
    return sigma * g * 4 * 2.0 ** -52 + 2.0 ** -53 * np.abs(dt)


def gauss_bound(g):
    """The same for the cached Gaussian f * x1: the log's 3 ulp and one rounding."""
    return abs(g) * 4 * 2.0 ** -52


def oracle_rollout(x0, dts):
    """The stochastic env's closed loop on the oracle: u = controller() clipped to 0.5
    (flocking_stoch.py:39-46), step with dts[t]; returns the states (T,N,4)."""
    x, xs = np.array(x0, np.float64), []
    for dt in dts:
        u = fv.controller(x, clip=0.5)
        x = fv.integrate(x, u, float(dt), **STOCH)
        xs.append(x)
    return np.array(xs)


def rollout_sensitivity(x0, dts, mean=MEAN, sigma=SIGMA, patterns=64, seed=0):
    """D: the largest |x' - x| of oracle_rollout over `patterns` random sign patterns, every
    dt moved by +- dt_bound. Sign patterns sample the worst case and do not bound it: the
    tests allow 4 D."""
    dts = np.asarray(dts, np.float64)
    base = oracle_rollout(x0, dts)
    bound = dt_bound(dts, mean, sigma)
    rs = np.random.RandomState(seed)
    d = 0.0
    for _ in range(patterns):
        sign = rs.choice([-1.0, 1.0], size=dts.shape)
        d = max(d, float(np.abs(oracle_rollout(x0, dts + sign * bound) - base).max()))
    return d, base
