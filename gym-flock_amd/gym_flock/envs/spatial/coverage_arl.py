"""CoverageARL-v0 on the MI355X engine — drop-in for gym_flock/envs/spatial/coverage_arl.py.

The target graph comes from an occupancy grid (make_map.from_occupancy, make_map.py:234-271)
instead of random cities: load_graph() (:46-62) builds the pool of targets once, and with
num_subgraphs > 1 every reset() samples a random window of it, keeps the window's largest
connected component and retries until that holds MIN_GRAPH_SIZE targets
(_generate_targets :64-83). Both run in libgymflock.so (cov_load_occupancy,
cov_generate_submaps); the step, observation and greedy expert are CoverageEnv's.

The sampler's draws come from the global np.random, as in the reference: K tries are
drawn at once, the device walks them, and the stream is then rewound to where the
reference's loop would have left it.

The reference reads its map from gym_flock/envs/spatial/maps/grid_slice<rate>.npy. Those
maps are the reference's data and are not shipped here: pass `occupancy=` (an array or a
.npy path), or put grid_slice<rate>.npy into the directory named by GYM_FLOCK_MAPS or
into a maps/ folder beside this module.
"""
import os

import numpy as np

from ... import _native as nat
from .coverage import CoverageEnv

MIN_GRAPH_SIZE = 200
MAP_RES = 0.5
HIDE_NODES = False
SAMPLER_TRIES = 16  # tries drawn and sent to the device per launch


def find_occupancy(downsample_rate):
    """grid_slice<rate>.npy from $GYM_FLOCK_MAPS, then from maps/ beside this module."""
    name = "grid_slice%s.npy" % downsample_rate
    tried = []
    for d in (os.environ.get("GYM_FLOCK_MAPS"), os.path.join(os.path.dirname(os.path.abspath(__file__)), "maps")):
        if not d:
            continue
        path = os.path.join(d, name)
        if os.path.isfile(path):
            return path
        tried.append(path)
    raise FileNotFoundError(
        "no occupancy map %s: the reference's maps are not shipped with this package. Pass occupancy= (an array "
        "or a .npy path), or set GYM_FLOCK_MAPS to the directory that holds it (looked for %s)"
        % (name, ", ".join(tried) if tried else "GYM_FLOCK_MAPS is not set and there is no maps/ folder"))


class CoverageARLEnv(CoverageEnv):

    def __init__(self, n_robots=4, episode_length=50, pad_nodes=True, max_nodes=1000,
                 nearby_starts=True, num_subgraphs=3.0, check_connected=True,
                 downsample_rate=10, perimeter_delta=2.0, horizon=-1, hide_nodes=HIDE_NODES, n_node_feat=3,
                 occupancy=None, device=0, reset_mode="reference"):
        if occupancy is None:
            occupancy = find_occupancy(downsample_rate)
        if isinstance(occupancy, (str, os.PathLike)):
            occupancy = np.load(occupancy)
        self.occupancy = np.asarray(occupancy)
        if self.occupancy.ndim != 2:
            raise ValueError("occupancy must be a 2-D grid, got shape %s" % (self.occupancy.shape,))
        self.check_connected = check_connected
        self.downsample_rate = downsample_rate
        self.perimeter_delta = perimeter_delta
        self.num_subgraphs = num_subgraphs
        self.all_targets = None
        self.min_xy = None
        self.max_xy = None
        self.range_xy = None
        self.subgraph_size = None
        self._placed = None  # the robots' nodes after update_state, until the next step
        super(CoverageARLEnv, self).__init__(n_robots=n_robots, init_graph=False, episode_length=episode_length,
                                             res=MAP_RES * downsample_rate, pad_nodes=pad_nodes, max_nodes=max_nodes,
                                             nearby_starts=nearby_starts, horizon=horizon, hide_nodes=hide_nodes,
                                             n_node_feat=n_node_feat, device=device, reset_mode=reset_mode)
        self.load_graph()
        targets, sampled = self._generate_targets()
        self._initialize_graph(targets, on_device=sampled)

    def _fixed_node_count(self):
        return self.num_subgraphs <= 1  # the map is the whole pool

    def load_graph(self):
        """coverage_arl.py:46-62 on the device (cov_load_occupancy)."""
        cfg = nat.occupancy_config(self.downsample_rate, self.perimeter_delta, self.check_connected,
                                   self.num_subgraphs, MIN_GRAPH_SIZE)
        n_pool = self._h.load_occupancy(self.occupancy, cfg)
        if not self.pad_nodes and self.max_nodes != n_pool + self.n_robots:
            self.max_nodes = n_pool + self.n_robots  # coverage.py:540-541
            self._make_handle()
            self._h.load_occupancy(self.occupancy, cfg)
        self.all_targets, lo, hi, sub = self._h.pool()
        if self.num_subgraphs > 1:
            self.min_xy, self.max_xy, self.subgraph_size = lo, hi, sub
            self.range_xy = self.max_xy - self.min_xy

    def _generate_targets(self):
        """coverage_arl.py:64-83. The tries' graph_start draws come from the global
        np.random exactly as the reference draws them, SAMPLER_TRIES at a time; one launch
        walks them (cov_generate_submaps) and says how many it consumed, and the stream is
        set back and advanced by exactly those, so it ends where the reference's does."""
        if not self.num_subgraphs > 1:
            return self.all_targets, False
        low, high = self.min_xy, self.max_xy - self.subgraph_size
        drawn = 0
        while True:
            state = np.random.get_state()
            draws = np.random.uniform(low=low, high=high, size=(SAMPLER_TRIES, 1, 2))
            try:
                n, st, tries = self._h.generate_submaps(draws=draws, env=0)
            except nat.GymFlockError as e:
                st = getattr(e, "status", None)
                if st is None or not st[0] & (nat.COV_MAP_TOO_MANY | nat.COV_MAP_TOO_FEW):
                    raise
                self.map_status = int(st[0])
                raise ValueError("could not fit a map of %d targets and %d robots into max_nodes = %d (%s)"
                                 % (int(e.n_targets[0]), self.n_robots, self.max_nodes, e)) from e
            if not st[0] & nat.COV_MAP_NO_WINDOW:
                break
            drawn += SAMPLER_TRIES
            if drawn >= self._h.occ.max_tries:  # the reference would spin forever
                raise nat.GymFlockError(nat.GF_EINVAL, "no window with a component of %d targets in %d tries"
                                        % (MIN_GRAPH_SIZE, drawn))
        np.random.set_state(state)
        np.random.uniform(low=low, high=high, size=(int(tries[0]), 1, 2))
        self.map_status = int(st[0])
        return self._h.targets(0, int(n[0])), True

    def update_state(self, state):
        """coverage_arl.py:42-44: the robots are put on the targets closest to `state`
        (cov_set_robot_positions)."""
        state = np.asarray(state, dtype=np.float64).reshape(self.n_robots, 2)
        r = np.linalg.norm(state.reshape((self.n_robots, 1, 2)) - self.targets.reshape((1, self.n_targets, 2)), axis=2)
        nearest = np.argmin(r, axis=1)
        self._h.set_robot_positions(0, self.targets[nearest])
        self._placed = nearest.astype(np.int64) + self.n_robots
        self._closest = self._placed
        self._greedy_cache = None

    @property
    def closest_targets(self):
        if self._placed is not None:
            return self._placed
        return CoverageEnv.closest_targets.fget(self)

    def step(self, action):
        self._placed = None
        return super(CoverageARLEnv, self).step(action)

    def reset(self):
        self._placed = None
        return super(CoverageARLEnv, self).reset()
