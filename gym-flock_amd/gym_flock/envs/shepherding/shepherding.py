"""Shepherding-v0 on the MI355X engine — drop-in for
gym_flock/envs/shepherding/shepherding.py of the reference.

Same class name, attributes and method signatures as the reference (`__init__` :16-70,
`seed` :72-78, `step` :80-117, `reset` :187-202, `controller` :204-233, `render`
:275-325, `close` :327-331). The pair pass, the unicycle update, the weighted adjacency,
the reward and the shepherd controller run in the HIP kernel of libgymflock.so
(csrc/shepherd.hip) through the C-ABI (gym_flock._native); `reset()` draws on the host
with NumPy, so its state is the reference's bit for bit. `set_reset_mode("device")` (or
`gym_flock.make(..., reset_mode="device")`) moves the draws into one launch on
`np_random`'s stream (csrc/shepherd_rollout.hip): the stream stays NumPy's bit for bit,
the positions then carry the device's cos / sin.

Differences a caller can observe:
  - `x` is a host mirror of the device state, fetched after every step and uploaded by
    the next call when the caller replaced or edited it;
  - the adjacency, the reward and the sheep's part of the control are the reference's bit
    for bit for the same state; the integrated state and `controller()` match it to
    rounding, because cos / sin / atan2 on the device are not NumPy's to the last bit.
"""
import numpy as np

from ... import _native as nat
from ..._spaces import Box, Env, np_random
from ...init_states import draw_shepherding

font = {'family': 'sans-serif', 'weight': 'bold', 'size': 14}


class ShepherdingEnv(Env):

    def __init__(self, device=0):
        self.mean_pooling = True  # :19 (unused by the reference too)

        self.nx = 3  # 2D position + orientation
        self.nu = 2

        self.n_sheep = 20
        self.n_shepherds = 10
        self.n_agents = self.n_sheep + self.n_shepherds
        self.agent_identities = np.vstack((np.ones((self.n_shepherds, 1)), np.zeros((self.n_sheep, 1))))

        self.dt = 0.01
        self.v_max = 2.0
        self.action_scalar = 5.0

        self.r_max_init = 1.0
        self.r_max = self.r_max_init * np.sqrt(self.n_agents)

        self.goal_offset = np.array([-self.r_max * 3, 0])
        self.goal_region_radius = 0.5 * self.r_max

        self.comm_radius = 2.0
        self.comm_radius_2 = self.comm_radius * self.comm_radius

        self.force_weights = 0.15 * np.hstack((3.0 * np.ones((1, self.n_shepherds, 1)),
                                               0.5 * np.ones((1, self.n_sheep, 1))))

        self.x = np.zeros((self.n_agents, self.nx))

        self.action_space = Box(low=-self.v_max, high=self.v_max, shape=(self.n_shepherds, self.nu),
                                dtype=np.float32)
        self.observation_space = Box(low=-np.inf, high=np.inf, shape=(self.n_agents, self.nx),
                                     dtype=np.float32)

        self.fig = None
        self.line1 = None
        self.line2 = None
        self.ax = None

        self.device = device
        self._h = None
        self._hkey = None
        self._synced = None  # the state the device holds, as last mirrored into self.x
        self.reset_mode = "reference"  # set_reset_mode
        self._rng_synced = None  # np_random's state as the device last left it, and on which handle
        self._rng_handle = None

        self.np_random = None
        self.seed()

    def seed(self, seed=None):
        self.np_random, seed = np_random(seed)
        return [seed]

    # ------------------------------------------------------------------ device
    def _handle(self):
        """The device handle for the current attributes (the reference reads them at call
        time); a change re-creates it, and the state is uploaded again from self.x."""
        key = (self.n_shepherds, self.n_sheep, float(self.dt), float(self.comm_radius), float(self.action_scalar),
               float(self.force_weights[0, 0, 0]), float(self.force_weights[0, -1, 0]),
               float(self.goal_region_radius), self.device)
        if self._h is not None and key != self._hkey:
            self._h.close()
            self._h = None
        if self._h is None:
            self._h = nat.ShepherdHandle(key[0], key[1], 1, key[2], key[3], key[4], (key[5], key[6]), key[7], key[8])
            self._hkey = key
            self._synced = None
        return self._h

    def _upload(self):
        """The handle holding self.x (uploaded when the caller changed it since the mirror)."""
        h = self._handle()
        if self._synced is None or not np.array_equal(self._synced, self.x):
            h.set_state(np.asarray(self.x, np.float64).reshape(1, self.n_agents, self.nx))
            self._synced = np.array(self.x, np.float64)
        return h

    def _outputs(self, h):
        """(observation (N,4), adjacency (N,N), reward) in one copy and one wait."""
        obs, adj, rew = h.outputs()
        return obs[0], adj[0], float(rew[0])

    # ------------------------------------------------------------------ gym API
    def step(self, u):
        """:80-117. Returns ((observations (N,4), adjacency (N,N)), reward, False, {})."""
        assert u.shape == (self.n_shepherds, self.nu)
        h = self._upload()
        h.step(np.asarray(u)[None])
        obs, adj, reward = self._outputs(h)
        self.x = obs[:, :self.nx].copy()  # the observation's first columns are the new state
        self._synced = self.x.copy()
        return (obs, adj), reward, False, {}

    def set_reset_mode(self, reset_mode):
        """"reference" (default): reset() draws on the host with NumPy, the reference's
        state bit for bit. "device": the draws run in one launch on self.np_random's stream
        (shep_reset_device); lengths, angles and the stream afterwards are NumPy's bit for
        bit, the positions are to the device's cos / sin instead of NumPy's."""
        if reset_mode not in ("reference", "device"):
            raise ValueError("reset_mode must be \"reference\" or \"device\"")
        self.reset_mode = reset_mode

    def _rng_changed(self, st):
        s = self._rng_synced
        return s is None or st[2] != s[2] or not np.array_equal(st[1], s[1]) or tuple(st[3:]) != tuple(s[3:])

    def _reset_device(self):
        """reset() with reset_mode="device": the stream goes up when the caller seeded or
        drew from np_random since the last one came down; the state comes back with the
        observation, the stream after it, so np_random stands where the reference's would."""
        h = self._upload()
        st = self.np_random.get_state()
        if self._rng_handle is not h or self._rng_changed(st):
            h.set_rng(st[:3], env=0)
        h.reset_device(self.r_max, self.goal_offset)
        obs, adj, _ = self._outputs(h)
        key, pos = h.get_rng(0)
        # a cached Gaussian (st[3:]) is the host's alone: uniform draws do not touch it
        self._rng_synced = ("MT19937", key, pos) + tuple(st[3:])
        self._rng_handle = h
        self.np_random.set_state(self._rng_synced)
        self.x = obs[:, :self.nx].copy()
        self._synced = self.x.copy()
        return obs, adj

    def reset(self):
        """:187-202: agents on a disk of radius sqrt(r_max) around goal_offset, drawn from
        np_random on the host (on the device with set_reset_mode("device")); headings keep
        their previous values, as in the reference."""
        if self.reset_mode == "device":
            return self._reset_device()
        self.x[:, :2] = draw_shepherding(self.n_agents, self.r_max, self.goal_offset, self.np_random)
        h = self._upload()
        h.observe()
        return self._outputs(h)[:2]

    def controller(self):
        """The baseline shepherd controller (:204-233), (n_shepherds, 2)."""
        return self._upload().controller()[0]

    def render(self, mode='human'):
        """:275-325: shepherds green, sheep red, the goal region a red circle."""
        import matplotlib.patches as patches
        import matplotlib.pyplot as plt

        uv = [np.cos(self.x[:, 2]), np.sin(self.x[:, 2])]
        ns = self.n_shepherds
        if self.fig is None:
            plt.ion()
            fig = plt.figure()
            self.ax = fig.add_subplot(111, aspect='equal')
            quiver = dict(units='xy', scale=2, width=0.1, headlength=4.5, headwidth=3)
            self.line1 = self.ax.quiver(self.x[:ns, 0], self.x[:ns, 1], uv[0][:ns], uv[1][:ns], color='g', **quiver)
            self.line2 = self.ax.quiver(self.x[ns:, 0], self.x[ns:, 1], uv[0][ns:], uv[1][ns:], color='r', **quiver)
            self.ax.add_patch(patches.Circle((0, 0), self.goal_region_radius, fill=False, edgecolor='r'))
            self.ax.plot([0], [0], 'kx')
            plt.xlim(-3.0 * self.r_max + self.goal_offset[0], self.r_max)
            plt.ylim(-3.0 * self.r_max + self.goal_offset[1], self.r_max)
            self.fig = fig

        self.line1.set_offsets(self.x[:ns, 0:2])
        self.line1.set_UVC(uv[0][:ns], uv[1][:ns])
        self.line2.set_offsets(self.x[ns:, 0:2])
        self.line2.set_UVC(uv[0][ns:], uv[1][ns:])
        self.fig.canvas.draw()
        self.fig.canvas.flush_events()

    def close(self):
        if self._h is not None:
            self._h.close()
            self._h = None
