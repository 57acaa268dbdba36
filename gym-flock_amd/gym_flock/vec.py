"""Batched FlockingRelative / Flocking-v0: B independent envs stepped by one launch.

This is the data-parallel form of the reference's per-env loop (one
FlockingRelativeEnv.step per env per step, flocking_relative.py:91-109). Outputs
stay in device memory; the getters copy to the host on demand, so a trainer that
only needs rewards or a few envs' observations never pays for the (B,N,N) network
transfer.
"""
import numpy as np

from . import _native as nat
from .init_states import draw_shepherding, synthetic_batch


# fe_variant presets of the registered flocking variants (include/gymflock.h)
VARIANTS = {
    "relative": {},
    "leader": dict(u_scale=1.0, n_frozen=2),                      # flocking_leader.py
    "obstacle": dict(u_scale=1.0, n_frozen=4, n_vel_zero=4),      # flocking_obstacle.py
    "stochastic": dict(u_scale=6.0, u_clip=0.5, x_scale=6.0, ctrl_clip=0.5),  # flocking_stoch.py
    "twoflocks": {},                                              # reset only
}


class VecFlockingRelative:
    """B FlockingRelative-v0 envs of N agents on one GPU.

    env_offset: global index of this shard's first env (seeds are env_offset + b),
    so a batch sharded over ranks reproduces the single-device batch.
    variant: a VARIANTS key or a dict of fe_variant fields (flocking variants).
    dt_noise: (mean, sigma): every step's dt is drawn ~ N(mean, sigma) per env on the
    device, from the env's own stream (FlockingStochastic-v0: (0.12, 0.018); the streams
    come from reset_device(seed) or h.set_rng). variant="stochastic" alone keeps a fixed dt.
    """

    def __init__(self, n_envs, n_agents, comm_radius=0.9, dt=0.01, v_max=5.0,
                 action_scalar=10.0, mean_pooling=True, centralized=True, n_neighbors=0,
                 device=0, env_offset=0, variant=None, dt_noise=None):
        self.n_envs, self.n_agents = int(n_envs), int(n_agents)
        self.v_max = v_max
        self.env_offset = int(env_offset)
        self.h = nat.FlockHandle(n_agents, n_envs, comm_radius, dt, action_scalar,
                                 mean_pooling, centralized, n_neighbors, device)
        v = VARIANTS[variant] if isinstance(variant, str) else variant
        if v:
            self.h.set_variant(**v)
        if dt_noise is not None:
            self.h.set_dt_noise(*dt_noise)

    # ------------------------------------------------------------------- state
    def reset(self, seed=0, x=None):
        """Synthetic init for envs seed+env_offset+b, or a given (B,N,4)."""
        if x is None:
            x = synthetic_batch(self.n_envs, self.n_agents, seed + self.env_offset, self.v_max)
        self.h.set_state(x)
        self.h.compute_helpers()
        if self.h.n_taps:  # a policy is set (set_policy here or on the handle)
            self.h.reset_aggregation()
        return x

    def reset_device(self, seed=None, envs=None, reject=True, max_tries=4096, r_max=None, fetch=True,
                     kind="relative"):
        """reset() of the reference (flocking_relative.py:156-192) on the device, one launch
        for the selected envs: env b draws from its own stream, RandomState(seed + env_offset
        + b) or, with seed None, continued where its last reset left it, until a draw passes
        the reference's acceptance test (min degree >= 2, min distance >= 0.1) or max_tries
        are spent (the last draw is kept; status bit FE_RESET_EXHAUSTED). envs: None (all),
        a bool mask or an index list; the other envs keep state and stream, so a trainer
        resets the envs whose episode ended between two steps. reject=False keeps the first
        draw (reset()'s synthetic init, any N). r_max: the reference's self.r_max, sqrt(N)
        by default. Ends with compute_helpers(). Returns (tries, status) per env, or None
        with fetch=False (nothing waits for the device then).
        kind: the variants' own resets from the same streams (fe_reset_variant): "leader"
        (flocking_leader.py:37-41: the reset above, then one draw into both leaders'
        velocities; unlike the reference's reset(), the observation computed here is of the
        state after that override), "twoflocks" (flocking_twoflocks.py:8-28, n_agents a
        multiple of int(n_agents / 10)) and "obstacle" (flocking_obstacle.py:59-74, no
        draws, n_agents a multiple of 5); the last two report tries = 1."""
        s = None if seed is None else int(seed) + self.env_offset
        out = self.h.reset_device(s, envs, reject, max_tries, r_max, self.v_max, fetch=fetch, kind=kind)
        self.h.compute_helpers()
        if self.h.n_taps:  # a policy is set (set_policy here or on the handle)
            self.h.reset_aggregation(envs)
        return out

    def np_random(self, env):
        """A RandomState at env `env`'s device stream position (after its last reset or dt
        draw), its cached Gaussian included."""
        rs = np.random.RandomState()
        rs.set_state(self.h.get_rng_state(env))
        return rs

    def set_state(self, x):
        self.h.set_state(x)

    def get_state(self):
        return self.h.get_state()

    # ---------------------------------------------------------------- hot path
    def step(self, u=None, controller=False, knn=False, network=True, expert=False,
             resident=False, device_ptr=None, dt=None):
        """Advance every env one step.

        network: True (dense (N,N) rows), False (none), "packed" (adjacency bits +
        degree only) or "both".
        u: (B,N,2) host actions (float32 or float64 arithmetic like the reference); or
        expert=True to feed back the previous controller() output (closed loop); or
        resident=True to reuse the actions last given to set_actions(); or
        device_ptr=<int> for a device buffer of float32 actions.
        dt: per-env (B,) time step for this and later steps (the stochastic variant).
        Asynchronous: returns once the launch is queued (host actions are copied first).
        """
        if dt is not None:
            self.h.set_dt(dt)
        flags = 0
        if controller:
            flags |= nat.FE_WITH_CONTROLLER
        if knn:
            flags |= nat.FE_WITH_KNN
        if network == "packed":  # adjacency bits + degree instead of the dense (N,N) rows
            flags |= nat.FE_PACKED_NETWORK | nat.FE_NO_NETWORK
        elif network == "both":
            flags |= nat.FE_PACKED_NETWORK
        elif not network:
            flags |= nat.FE_NO_NETWORK
        if expert:
            self.h.step(None, flags | nat.FE_U_EXPERT)
        elif resident:
            self.h.step(None, flags | nat.FE_U_RESIDENT)
        elif device_ptr is not None:
            self.h.step(device_ptr, flags | nat.FE_U_DEVICE)
        else:
            self.h.step(u, flags)

    def expert_steps(self, n_steps, record=("rewards",), every=1, fetch=True, device_ptrs=None):
        """n_steps of the expert loop u = controller(); step(u) for every env in ONE launch
        (fe_step_expert, n_agents <= 256), for demonstrations: the same states, adjacency
        and degrees as n_steps calls of step(expert=True, controller=True,
        network="packed"), bit for bit. Needs a controller output of the current state
        (controller(), or a step with controller=True).
        record: what to keep of every `every`-th step (`every` divides n_steps), among
        "x" (K,B,N,4), "state_values" (K,B,N,6), "adj_bits" (K,B,N,ceil(N/64)) uint64,
        "degree" (K,B,N), "controls" (K,B,N,2) (the controller of the recorded state) with
        K = n_steps // every, and "rewards" (n_steps,B), always every step's; with dt_noise
        also "dt" (n_steps,B), the dt every step integrated with. Returns a
        dict of arrays. device_ptrs={name: device address}: those records are written to
        the caller's device buffers in stream order instead (e.g. tensor.data_ptr());
        nothing waits and None is returned, as with fetch=False (nothing recorded).
        Afterwards get_state(), controls(), rewards(), state_values() and network_packed()
        are the last step's; network() raises until compute_helpers() or a step that
        writes the dense network."""
        return self.h.step_expert(n_steps, record, every, fetch, device_ptrs)

    def set_policy(self, weights, biases, n_taps, clip=0.0):
        """The learner of policy_steps: one network shared by all agents over n_taps (1..4)
        delayed aggregation taps of 6 features each (tap 0 the state_values, tap k the
        neighbourhood mean, or sum without mean_pooling, of the previous state's tap k - 1;
        zero at an episode's start). weights / biases: lists of up to 3 arrays in
        torch.nn.Linear's layout ((out, in) and (out)), cast to float32; 6 * n_taps inputs,
        hidden widths multiples of 4 up to 64, 2 outputs, ReLU between layers; clip > 0
        clips the outputs to [-clip, clip]. weights=None removes it. Zeroes every env's taps."""
        self.h.set_policy(weights, biases, n_taps, clip)

    def policy_steps(self, n_steps, beta=0.0, record=("rewards",), every=1, fetch=True, device_ptrs=None):
        """n_steps of the DAgger loop for every env in ONE launch (fe_step_policy, n_agents <=
        256, FlockingRelative only): each step integrates the expert's action with
        probability beta (one random_sample() of the env's device stream per step, the
        stream of reset_device; beta 0 and 1 draw nothing), else the policy's action for the
        current aggregation; the expert's action of every state reached is recorded as
        the label. Needs set_policy and a controller output of the current state.
        record: expert_steps' names, and "agg" (K,B,N,n_taps,6) float32, "policy"
        (K,B,N,2) float32 (the learner's action for the recorded state), "applied"
        (n_steps,B,N,2) (what each step integrated) and "used_expert" (n_steps,B) uint8.
        (agg, controls) of a record is one DAgger pair. every / fetch / device_ptrs and the
        getters afterwards as expert_steps; aggregation() is the final state's."""
        return self.h.step_policy(n_steps, beta, record, every, fetch, device_ptrs)

    def aggregation(self, env=None):
        """The current state's aggregation features (B,N,n_taps,6) float32, or one env's."""
        return self.h.aggregation(env)

    def reset_aggregation(self, envs=None):
        """Zero the taps k >= 1 of the envs (None: all): an episode's start. reset() and
        reset_device() do it for the envs they touch; after set_state() it is the caller's."""
        self.h.reset_aggregation(envs)

    def compute_helpers(self):
        """compute_helpers() on the current state: every observation buffer anew."""
        self.h.compute_helpers()

    def set_actions(self, u):
        self.h.set_actions(u)

    def controller(self, centralized=None):
        return self.h.controller(centralized)

    # ----------------------------------------------------------------- outputs
    def state_values(self, env=None):
        return self.h.state_values(env)

    def network(self, env=None):
        return self.h.network(env)

    def rewards(self):
        return self.h.rewards()

    def network_packed(self, env=None):
        """Adjacency bits and degrees of the last step(network="packed" or "both")."""
        return self.h.network_packed(env)

    def controls(self, env=None):
        return self.h.controls(env)

    def knn(self, env=None):
        return self.h.knn(env)

    def stats(self, env=0):
        return self.h.stats(env)

    def stats_summary(self):
        """(B, 2) per-env np.mean(vel_diffs), np.mean(min_dists) (get_stats, :136-143)."""
        return self.h.stats_summary()

    def sync(self):
        self.h.sync()

    def close(self):
        self.h.close()


class VecCoverage:
    """B Coverage-v0 envs (R robots each) on one GPU, one workgroup per env.

    Each env gets its own target graph (set_targets(env=b)) or all share one
    (env=-1); reset() draws starts and the unvisited set per env from
    np.random.RandomState(seed + env_offset + b) in the reference's order.

    CoverageARL-v0 batches: VecCoverage(B, 4, max_nodes=1000, episode_length=50, res=5.0),
    then load_occupancy(grid); reset(new_maps=True) then samples every env's map from the
    pool (generate_submaps). reset() draws uniform starts for every env from fresh streams
    (cov_reset_seeded); reset_envs() resets chosen envs (a mask, an index list, or the envs
    that are done) from their continued np_random streams on the device, with the
    reference's nearby_starts region when nearby_starts=True (cov_reset_device).

    ExploreEnv batches: the same with hide_nodes=True (and horizon=19). obs(), flat_obs()
    and graphs_tuple() then give the hidden observation (4 node features, hidden senders),
    step(greedy=True) masks undiscovered targets, and expert_steps() is refused.
    """

    def __init__(self, n_envs, n_robots, max_nodes=1000, episode_length=75, res=5.5,
                 frac_active_targets=0.5, device=0, env_offset=0, hide_nodes=False, horizon=10,
                 nearby_starts=False):
        self.n_envs, self.n_robots = int(n_envs), int(n_robots)
        self.nearby_starts = bool(nearby_starts)  # reset_envs: nearby = n_robots * NEARBY_DENSITY (5)
        self.frac = frac_active_targets
        self.env_offset = int(env_offset)
        self.hide_nodes = bool(hide_nodes)
        self.h = nat.CoverageHandle(n_robots, n_envs, max_nodes, episode_length, res, None, device, horizon=horizon)
        if self.hide_nodes:
            self.h.set_hidden(True)
        self.n_targets = np.zeros(self.n_envs, np.int64)
        self._rngs = None          # host-held np_random streams (else on the device)
        self._dev_streams = False  # the device holds every env's np_random stream
        self._pool = False         # an occupancy pool is loaded: new maps are sampled from it

    def load_occupancy(self, grid, downsample_rate=10, perimeter_delta=2.0, check_connected=True, num_subgraphs=3.0,
                       min_targets=200, max_tries=4096):
        """The target pool of an occupancy grid, shared by every env (cov_load_occupancy;
        coverage_arl.py:46-62). Returns the pool's size. With num_subgraphs <= 1 every
        env's map is the whole pool, set here."""
        cfg = nat.occupancy_config(downsample_rate, perimeter_delta, check_connected, num_subgraphs, min_targets,
                                   max_tries)
        n = self.h.load_occupancy(grid, cfg)
        self._pool = True
        self._sampled = num_subgraphs > 1
        if not self._sampled:
            self.set_targets(self.h.pool()[0])
        return n

    def generate_submaps(self, map_seed=None):
        """A new sampled map for every env (coverage_arl.py:64-83, cov_generate_submaps):
        env b's window draws come from its own map stream, seeded np.random.seed(map_seed +
        env_offset + b) when map_seed is given, else continued from its previous map.
        Returns (n_targets (B,), status (B,), tries (B,)). With num_subgraphs <= 1 nothing
        is drawn: the maps stay the pool."""
        if not self._pool:
            raise nat.GymFlockError(nat.GF_ESTATE, "load_occupancy first")
        if not self._sampled:
            z = np.zeros(self.n_envs, np.int32)
            return self.n_targets.astype(np.int32), z, z.copy()
        seed = None if map_seed is None else int(map_seed) + self.env_offset
        n, st, tries = self.h.generate_submaps(map_seed=seed)
        self.n_targets[:] = n
        return n, st, tries

    def set_targets(self, targets, env=-1):
        self.h.set_targets(targets, env)
        if env < 0:
            self.n_targets[:] = len(targets)
        else:
            self.n_targets[env] = len(targets)

    def generate_maps(self, map_seed=None):
        """A new target map for every env on the device (coverage.py:516-527, as each
        reference reset() draws one): env b's cities come from its own map stream, seeded
        np.random.seed(map_seed + env_offset + b) when map_seed is given, else continued
        from its previous map, as the reference's global np.random continues from one
        reset to the next. Returns (n_targets (B,), status (B,))."""
        seed = None if map_seed is None else int(map_seed) + self.env_offset
        n, st, _ = self.h.generate_maps(map_seed=seed)
        self.n_targets[:] = n
        return n, st

    def targets(self, env):
        """Env `env`'s current map, (n_targets, 2) float64 (cov_get_targets)."""
        return self.h.targets(env, int(self.n_targets[env]))

    def reset(self, seed=0, draws="device", new_maps=False, map_seed=None):
        """Env b is a reference env whose np_random was seeded seed + env_offset + b: its
        reset draws (coverage.py:405-424), then its stream continues on the device for the
        greedy expert's fallback draws (step(greedy=True)); np_random(b) reads it back.
        draws="device" (cov_reset_seeded): the draws run on the device, one wave per env;
        "host": RandomState loops here (~0.5 ms per env), then cov_reset and cov_set_rng.
        Both return (start (B,R) target-local, visited (B, max_nodes-R)), bit-identical.
        new_maps: each env first draws a new map on the device (generate_maps(map_seed), or
        generate_submaps(map_seed) once an occupancy pool is loaded), as every reference
        reset() does (:378-397)."""
        if new_maps and self._pool:
            self.generate_submaps(map_seed)
        elif new_maps:
            self.generate_maps(map_seed)
        self._rngs = None
        if draws == "device":
            out = self.h.reset_seeded(seed + self.env_offset, self.frac)
            self._dev_streams = True
            return out
        R, tmax = self.n_robots, self.h.t_max
        start = np.empty((self.n_envs, R), np.int32)
        visited = np.ones((self.n_envs, tmax), np.uint8)
        rngs = []
        for b in range(self.n_envs):
            rs = np.random.RandomState(seed + self.env_offset + b)
            T = int(self.n_targets[b])
            start[b] = rs.choice(np.arange(T), size=(R,), replace=False)
            drop = rs.choice(np.arange(T) + R, size=(int(T * self.frac),), replace=False)
            visited[b, drop - R] = 0
            rngs.append(rs)
        self.h.reset(start, visited)
        if R <= 624:  # device draws (COV_GREEDY_RNG): one key regeneration per step at most
            self.h.set_rng(rngs)
            self._dev_streams = True
        else:
            self._rngs, self._dev_streams = rngs, False
        return start, visited

    def reset_envs(self, envs=None, new_maps=False, nearby=None, seed=None):
        """Reset chosen envs on the device and leave every other env as it is, bit for bit
        (cov_reset_device). envs: None (all), a bool mask (B), a list of env indices, or
        "done" (the envs whose last step set done). Each selected env continues its own
        np_random stream (the reference's reset(), coverage.py:398-414), or starts from
        RandomState(seed + env_offset + b) with seed given; nearby (default: n_robots * 5
        with nearby_starts=True, else 0) draws the start region of get_n_nearest(choice(T),
        nearby); new_maps first draws the selected envs' next maps from their map streams.
        Returns (n_reset, start (B,R), visited (B, max_nodes-R), status (B)); rows of envs
        that were not reset are zero."""
        if self._rngs is not None:  # the host holds the streams: back onto the device
            self.h.set_rng(self._rngs)
            self._rngs, self._dev_streams = None, True
        if nearby is None:
            nearby = self.n_robots * 5 if self.nearby_starts else 0
        mask, done = None, False
        if isinstance(envs, str):
            if envs != "done":
                raise ValueError("envs: None, a mask, a list of indices or \"done\"")
            done = True
        elif envs is not None:
            e = np.asarray(envs)
            if e.dtype == bool or e.dtype == np.uint8 and e.shape == (self.n_envs,):
                mask = e.astype(bool)
            else:
                mask = np.zeros(self.n_envs, bool)
                mask[e.astype(np.int64)] = True
        sd = None if seed is None else int(seed) + self.env_offset
        try:
            n, start, visited, region, status = self.h.reset_device(mask, self.frac, nearby, sd, new_maps, done)
        finally:
            if new_maps:  # the selected envs' new sizes
                self.n_targets[:] = self.h.n_targets()
        if seed is not None:
            self._dev_streams = True
        return n, start, visited, status

    def _device_draws(self):
        """Whether the fused greedy step can draw the fallback robots' np_random.choice(4)
        on the device (COV_GREEDY_RNG): the streams live there, n_robots <= 624 (one key
        regeneration per step) and the per-node greedy lists exist (max_nodes - n_robots
        <= 1024). Never with hidden nodes: the fused step does not know the discovered set."""
        return not self.hide_nodes and self._dev_streams and self._rngs is None and self.n_robots <= 624 and self.h.t_max <= 1024

    def _explore_fused(self):
        """Whether a greedy step of a hidden batch can run as one fused launch
        (cov_explore_expert): the streams live on the device, n_robots <= 624 (one key
        regeneration per step) and the per-node greedy lists exist (max_nodes - n_robots <=
        1024)."""
        return self.hide_nodes and self._dev_streams and self._rngs is None and self.n_robots <= 624 and self.h.t_max <= 1024

    def _host_rngs(self):
        """The envs' np_random streams as host RandomStates (read back from the device the
        first time; the host keeps them from then on, until the next reset)."""
        if self._rngs is None:
            if not self._dev_streams:
                raise nat.GymFlockError(nat.GF_ESTATE, "reset first (no np_random streams)")
            keys, pos = self.h.get_rng()
            self._rngs = []
            for b in range(self.n_envs):
                rs = np.random.RandomState()
                rs.set_state(("MT19937", keys[b], int(pos[b])))
                self._rngs.append(rs)
            self._dev_streams = False
        return self._rngs

    def np_random(self, env):
        """Env `env`'s np_random after the fallback draws of the steps so far (a RandomState
        continuing the device stream, or the host one)."""
        if self._rngs is not None:
            return self._rngs[env]
        keys, pos = self.h.get_rng()
        rs = np.random.RandomState()
        rs.set_state(("MT19937", keys[env], int(pos[env])))
        return rs

    def step(self, actions=None, resident=False, greedy=False, fallback="draw"):
        """actions (B,R); or resident=True (the last set/greedy actions); or greedy=True
        (controller(greedy=True), coverage.py:800-872, computed in the step's own launch).
        fallback: robots the reference hands to np_random.choice(4) (:861-864) draw it from
        their env's stream ("draw", the reference's semantics: on the device inside the
        step when _device_draws(), or with hidden nodes when _explore_fused(); else the
        greedy kernel, the draws on the host in robot order and a resident step) or take
        action 0 ("zero"); include/gymflock.h COV_ACTIONS_GREEDY, COV_GREEDY_RNG,
        cov_explore_expert."""
        if resident or greedy:
            if greedy and fallback == "draw" and self._explore_fused():
                self.h.explore_expert(1, fetch=False)  # the masked expert, its draws, the step and the discovery
                return
            if greedy and fallback == "draw" and not self._device_draws():
                a, rnd = self.h.controller_greedy()
                if rnd.any():
                    rngs = self._host_rngs()
                    for b in np.nonzero(rnd.any(axis=1))[0]:
                        k = np.nonzero(rnd[b])[0]
                        a[b, k] = rngs[b].choice(4, size=len(k))
                    self.h.set_actions(a)
                rc = self.h._step_resident()
            elif greedy and self.hide_nodes:  # fallback="zero": the masked expert, then a resident step
                self.h.controller_greedy(fetch=False)
                rc = self.h._step_resident()
            elif greedy:
                rc = self.h._step_greedy_rng() if fallback == "draw" else self.h._step_greedy()
            else:
                rc = self.h._step_resident()
            if rc:
                nat.check(rc)
            return
        self.h.step(actions)

    def expert_steps(self, n_steps, fetch=True):
        """n_steps of the reference's greedy expert (controller(greedy=True) with its
        np_random.choice(4) fallback draws, then step) for every env in ONE launch
        (cov_step_expert): the same states, rewards and streams as n_steps calls of
        step(greedy=True), for expert rollouts. Needs the streams on the device (a reset with
        draws="device", or R <= 624 with host draws) and the greedy lists
        (max_nodes - n_robots <= 1024). Returns (rewards (n_steps,B), done (n_steps,B)) or
        None with fetch=False."""
        if self.hide_nodes:
            return self.h.step_expert(n_steps, fetch=fetch)  # the library refuses it (GF_EINVAL)
        if not self._device_draws():
            raise RuntimeError("expert_steps needs the envs' np_random streams on the device, n_robots <= 624 "
                               "and max_nodes - n_robots <= 1024")
        return self.h.step_expert(n_steps, fetch=fetch)

    def expert_rollout(self, n_steps, record=("rewards", "done"), every=1, auto_reset=False, nearby=None, fetch=True,
                       device_ptrs=None):
        """expert_steps with records, and across episode ends, in ONE launch
        (cov_expert_rollout): the reference driver's loop `reset(); while not done: a =
        controller(greedy=True); step(a)` for every env, its output the demonstrations.
        record: names among rewards, done, actions, needs_random (every step's) and flat_obs
        (the flat float32 row after every `every`-th step); returns a dict of host arrays
        (done and needs_random as bool). auto_reset: an env whose step sets done is reset
        inside the launch as reset_envs("done", nearby=nearby) right after that step would
        reset it (same map, frac_active_targets of the constructor, nearby defaulting as in
        reset_envs); the dict then also has n_resets (B) and reset_status (B), and flat_obs
        after a done step is the reset observation (the terminal one is not recorded). An env
        whose start region has fewer nodes than robots is not reset and goes on stepping
        (COV_RESET_REGION_SMALL in reset_status). device_ptrs: {name: device address} of
        caller-owned buffers (h.rollout_shapes(n_steps, every); n_resets / reset_status (B)
        int32), written in stream order; returns None, as with fetch=False. The preconditions
        are expert_steps's; refused with hide_nodes (explore_expert_steps is the form there)."""
        if self.hide_nodes:
            raise RuntimeError("expert_rollout is for envs that do not hide nodes; explore_expert_steps is the "
                               "form for hide_nodes=True")
        if not self._device_draws():
            raise RuntimeError("expert_steps needs the envs' np_random streams on the device, n_robots <= 624 "
                               "and max_nodes - n_robots <= 1024")
        ar = None
        if auto_reset:
            if nearby is None:
                nearby = self.n_robots * 5 if self.nearby_starts else 0
            ar = (self.frac, int(nearby))
        out = self.h.expert_rollout(n_steps, record, every, fetch, device_ptrs, auto_reset=ar)
        if out is not None:
            for k in ("done", "needs_random"):
                if k in out:
                    out[k] = out[k].astype(bool)
        return out

    def explore_expert_steps(self, n_steps, record=("rewards", "done"), every=1, fetch=True, device_ptrs=None):
        """n_steps of the reference's greedy expert on envs that hide nodes (ExploreEnv:
        controller(greedy=True) masks visited or undiscovered targets and draws
        np_random.choice(4) where it gives up, then step and the discovery) for every env in
        ONE launch (cov_explore_expert): the same states, observations, rewards and streams as
        n_steps calls of step(greedy=True). record: names among rewards, done, actions,
        needs_random (every step's) and flat_obs (the hidden flat row after every `every`-th
        step, float32); returns a dict of host arrays (done as bool). device_ptrs: {name:
        device address} of caller-owned buffers (h.rollout_shapes(n_steps, every)), written
        in stream order; returns None, as with fetch=False."""
        if not self.hide_nodes:
            raise RuntimeError("explore_expert_steps is for envs that hide nodes (hide_nodes=True); "
                               "expert_steps is the form for the others")
        if not (self._dev_streams and self._rngs is None):
            raise RuntimeError("explore_expert_steps needs the envs' np_random streams on the device (a reset with "
                               "draws=\"device\", or host draws with n_robots <= 624, and no host-drawn step since)")
        out = self.h.explore_expert(n_steps, record, every, fetch, device_ptrs)
        if out is not None:
            for k in ("done", "needs_random"):
                if k in out:
                    out[k] = out[k].astype(bool)
        return out

    def set_actions(self, actions):
        self.h.set_actions(actions)

    def rewards(self):
        return self.h.rewards()

    def obs(self, env=0):
        return self.h.hidden_obs(env) if self.hide_nodes else self.h.obs(env)

    def flat_obs(self, f32=False, device_ptr=None):
        """Every env's observation as one FlattenDictWrapper row (B, 15*max_nodes + 1), or
        (B, 16*max_nodes + 1) with hidden nodes."""
        return self.h.flat_obs(f32, device_ptr)

    def graphs_tuple(self, mask_all=False):
        """The batch as unpack_obs's graph tuple (coverage.py:689-741)."""
        return self.h.graphs_tuple(mask_all)

    def sync(self):
        self.h.sync()

    def close(self):
        self.h.close()


class VecShepherding:
    """B Shepherding-v0 envs (reference gym_flock/envs/shepherding/shepherding.py) of
    n_shepherds + n_sheep unicycle agents on one GPU, one launch per step for the whole
    batch; expert_steps(n) runs n closed-loop steps of the heuristic shepherd controller in
    one launch, the states never leaving the chip.

    The adjacency, the reward and the sheep's controls are the reference's bit for bit for
    a given state; the integrated state matches it to rounding (the device's cos / sin are
    not NumPy's to the last bit)."""

    def __init__(self, n_envs, n_shepherds=10, n_sheep=20, dt=0.01, comm_radius=2.0, action_scalar=5.0,
                 r_max_init=1.0, device=0):
        self.n_envs, self.n_shepherds, self.n_sheep = int(n_envs), int(n_shepherds), int(n_sheep)
        self.n_agents = self.n_shepherds + self.n_sheep
        self.r_max = r_max_init * np.sqrt(self.n_agents)           # :39
        self.goal_offset = np.array([-self.r_max * 3, 0])          # :42
        self.goal_region_radius = 0.5 * self.r_max                 # :43
        self.h = nat.ShepherdHandle(n_shepherds, n_sheep, n_envs, dt, comm_radius, action_scalar,
                                    goal_region_radius=self.goal_region_radius, device=device)

    # ------------------------------------------------------------------- state
    def reset(self, seed=0):
        """Env b draws from RandomState(seed + b) as the reference's reset() does after
        seed(seed + b) (host draws: the state is the reference's bit for bit; headings start
        at 0). Returns the (B,N,3) state; obs() / adj() hold its observation. The device
        form is reset_device(seed, headings="zero"): one launch, positions to the device's
        cos / sin."""
        x = np.zeros((self.n_envs, self.n_agents, 3))
        for b in range(self.n_envs):
            rs = np.random.RandomState(seed + b)
            x[b, :, :2] = draw_shepherding(self.n_agents, self.r_max, self.goal_offset, rs)
        self.set_state(x)
        return x

    def reset_device(self, seed=None, envs=None, headings="keep", fetch=True):
        """reset() of the reference (:187-202) on the device, one launch for the selected
        envs (shep_reset_device): env b draws its lengths, then its angles, from its own
        stream, RandomState(seed + b) or, with seed None, continued where it stands
        (np_random(b), h.set_rng). Lengths, angles and streams are NumPy's bit for bit, the
        positions to the device's cos / sin. envs: None (all), a bool mask or an index list;
        the other envs keep state, outputs and stream. headings: "keep" (the reference's
        reset() does not touch them; a batch that never had a state starts from zeros) or
        "zero". The launch also writes obs() / adj() / rewards() of the new state and zeroes
        the selected envs' episode step counts. Returns the (B,N,3) state, or None with
        fetch=False (nothing waits for the device then)."""
        if headings not in ("keep", "zero"):
            raise ValueError("headings must be 'keep' or 'zero', not %r" % (headings,))
        self.h.reset_device(self.r_max, self.goal_offset, seed, envs, headings == "zero")
        return self.h.get_state() if fetch else None

    def np_random(self, env):
        """A RandomState holding env `env`'s device stream."""
        keys, pos = self.h.get_rng(env)
        rs = np.random.RandomState()
        rs.set_state(("MT19937", keys, pos))
        return rs

    def set_state(self, x):
        """A (B,N,3) state and its observation, adjacency and reward."""
        self.h.set_state(x)
        self.h.observe()

    def get_state(self):
        return self.h.get_state()

    # ---------------------------------------------------------------- hot path
    def step(self, u=None, resident=False, device_ptr=None, expert=False, f64=False):
        """Advance every env one step. u: (B,n_shepherds,2) host actions (float32 or
        float64 arithmetic like the reference's u * 5.0); or resident=True to reuse the
        action buffer (the last host actions or controller() output); or device_ptr=<int>
        for a device buffer of float32 (f64=True: float64) actions, read on the handle's
        stream; or expert=True: controller() of the current state computed in the step's
        launch. Asynchronous."""
        if expert:
            self.h.step(None, nat.SHEP_U_EXPERT)
        elif resident:
            self.h.step(None, nat.SHEP_U_RESIDENT)
        elif device_ptr is not None:
            self.h.step(device_ptr, nat.SHEP_U_DEVICE | (nat.SHEP_U_F64 if f64 else 0))
        else:
            self.h.step(u)

    def controller(self, fetch=True):
        """The heuristic shepherd controller (:204-273) of every env, (B,n_shepherds,2)."""
        return self.h.controller(fetch)

    def expert_steps(self, n_steps, fetch=True):
        """n_steps of u = controller(); step(u) in one launch; rewards (n_steps,B)."""
        return self.h.step_expert(n_steps, fetch)

    def expert_rollout(self, n_steps, record=("rewards", "done"), every=1, episode_length=None, f32=False, fetch=True,
                       device_ptrs=None):
        """expert_steps with records, and across episode ends, in ONE launch
        (shep_expert_rollout): the reference driver's loop `reset(); for t in
        range(episode_length): u = controller(); step(u)`, episode after episode on each
        env's own stream, its output the demonstrations. record: names among obs (K,B,N,4)
        and adj (K,B,N,N) after every `every`-th step (K = n_steps // every; `every` divides
        n_steps), actions (n_steps,B,n_shepherds,2) (controller() of the state before the
        step, before action_scalar), rewards (n_steps,B), done (n_steps,B) bool and n_resets
        (B); f32: obs, adj and actions as float32. episode_length: None or 0 never resets;
        else an env whose episode step count (h.episode_steps(); every step advances it,
        set_state and reset_device zero it) reaches it is reset inside the launch right after
        that step, as reset_device(envs=[b]) would reset it: done is 1 there, rewards holds
        that step's reward, and the row recorded after it is the reset state's. So (obs()
        before the call, actions[0]) and (obs[t], actions[t + 1]) are (observation, expert
        action) pairs across episode ends; the terminal observation is not recorded. Needs
        the envs' streams (reset_device(seed), h.set_rng). Returns a dict of host arrays;
        device_ptrs: {name: device address} of caller-owned buffers
        (h.rollout_shapes(n_steps, every, f32)), e.g. torch tensors' data_ptr(), written in
        stream order (sync()); returns None, as with fetch=False (nothing recorded)."""
        L = int(episode_length or 0)
        out = self.h.expert_rollout(n_steps, record, every, L, (self.r_max, self.goal_offset) if L > 0 else None, f32,
                                    fetch, device_ptrs)
        if out is not None and "done" in out:
            out["done"] = out["done"].astype(bool)
        return out

    # ----------------------------------------------------------------- outputs
    def obs(self, f32=False, device_ptr=None):
        """(B,N,4) [x, y, theta, identity]; device_ptr: written there instead (stream-ordered)."""
        return self.h.obs(f32, device_ptr)

    def adj(self, f32=False, device_ptr=None):
        """(B,N,N) 1/r within comm_radius, else 0."""
        return self.h.adj(f32, device_ptr)

    def rewards(self, f32=False, device_ptr=None):
        return self.h.rewards(f32, device_ptr)

    def outputs(self):
        """(obs, adj, rewards) as host float64 in one copy and one wait."""
        return self.h.outputs()

    def controls(self):
        """(B,N,2) control of the last step: u * action_scalar, then the sheep's repulsion."""
        return self.h.controls()

    def sync(self):
        self.h.sync()

    def close(self):
        self.h.close()
