"""The Coverage C-ABI's refusals and its device memory, on tiny handles (B=2, R=2, a 3 x 4
grid of targets at spacing 5.5; max_nodes=14 so that the 12 targets fit beside the robots).

Every row of REFUSED is one refused call: its exact return code and the exact
fe_last_error text, as the library gave them before its host side was split into
cov_capi.hip / cov_maps_capi.hip / cov_step_capi.hip. The last rows pin which check fires
first where two would. The leak test walks every lazily allocating path of a handle,
closes it, and compares the device's free memory between cycles."""
import ctypes
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

B, R, M = 2, 2, 14
TM = M - R
XS, YS = np.meshgrid(np.arange(4) * 5.5, np.arange(3) * 5.5)
TARGETS = np.stack([XS.ravel(), YS.ravel()], axis=1)
START = np.array([[0, 5], [3, 8]], np.int32)

HIDDEN_FUSED = ("a handle with hidden nodes has no fused expert (the step kernel reads the visited flags, not the "
                "expert's visited-or-undiscovered mask): take the actions from cov_controller_greedy, then cov_step")
NEED_GRAPH = "set the target graph of every env first (cov_set_targets)"
NEED_RESET = "reset first (cov_reset)"
NEED_STREAMS = "set the envs' np_random streams first (cov_set_rng or cov_reset_seeded)"
MAP_FLAGS = "flags: COV_MAP_SEED | COV_MAP_CITIES"
SUB_FLAGS = "flags: COV_MAP_SEED | COV_MAP_DRAWS"


@pytest.fixture(scope="module")
def nat():
    from gym_flock import _native
    return _native


@pytest.fixture(scope="module")
def handles(nat):
    """The states a refusal can meet: fresh (created), graph (targets set), state (reset from
    given starts: no np_random streams), seeded (reset on the device: streams), and the same
    three with hidden nodes."""
    def make(targets=True, reset=None, hidden=False):
        h = nat.CoverageHandle(R, B, M)
        if targets:
            h.set_targets(TARGETS)
        if reset == "given":
            h.reset(START, np.zeros((B, TM), np.uint8))
        elif reset == "seeded":
            h.reset_seeded(3)
        if hidden:
            h.set_hidden(True)
        return h
    hs = {"fresh": make(targets=False), "graph": make(), "state": make(reset="given"),
          "seeded": make(reset="seeded"), "hidden_graph": make(hidden=True),
          "hidden_state": make(reset="given", hidden=True), "hidden_seeded": make(reset="seeded", hidden=True)}
    yield hs
    for h in hs.values():
        h.close()


def _rollout(nat, every):
    rec = nat.CovRollout()
    rec.record_every = every
    return rec


def _reset_device(nat, lib, h, flags, mask=None):
    rc = nat.CovResetConfig(0.5, 0, flags, 0)
    return lib.cov_reset_device(h, ctypes.byref(rc), nat.ptr(mask), None, None, None, None, None)


def _maps(nat, lib, h, env, flags, seed=0, cities=None, mc="default"):
    mc = nat.map_config_default() if mc == "default" else mc
    return lib.cov_generate_maps(h, ctypes.byref(mc) if mc is not None else None, env, seed, nat.ptr(cities), flags,
                                 None, None, None)


ACTS = np.zeros((B, R), np.int32)
NEXT = np.zeros((B, R), np.int32)
DRAWS = np.zeros((B, 1, 2))
VIS0 = np.zeros((B, TM), np.uint8)

# (id, handle, call(nat, lib, h), code name, text)
REFUSED = [
    # state refusals
    ("reset_before_targets", "fresh", lambda n, l, h: l.cov_reset(h, n.ptr(START), n.ptr(VIS0)), "GF_ESTATE", NEED_GRAPH),
    ("reset_seeded_before_targets", "fresh", lambda n, l, h: l.cov_reset_seeded(h, 0, 0.5, None, None), "GF_ESTATE",
     NEED_GRAPH),
    ("step_before_reset", "graph", lambda n, l, h: l.cov_step(h, n.ptr(ACTS), 0), "GF_ESTATE", NEED_RESET),
    ("greedy_rng_without_greedy", "state", lambda n, l, h: l.cov_step(h, None, n.COV_GREEDY_RNG), "GF_EINVAL",
     "COV_GREEDY_RNG needs COV_ACTIONS_GREEDY"),
    ("greedy_rng_without_streams", "state",
     lambda n, l, h: l.cov_step(h, None, n.COV_ACTIONS_GREEDY | n.COV_GREEDY_RNG), "GF_ESTATE",
     "COV_GREEDY_RNG: set the envs' np_random streams first (cov_set_rng)"),
    ("greedy_step_hidden", "hidden_seeded", lambda n, l, h: l.cov_step(h, None, n.COV_ACTIONS_GREEDY), "GF_EINVAL",
     "COV_ACTIONS_GREEDY: " + HIDDEN_FUSED),
    ("step_expert_no_state", "graph", lambda n, l, h: l.cov_step_expert(h, 1, None, None), "GF_ESTATE", NEED_RESET),
    ("step_expert_no_streams", "state", lambda n, l, h: l.cov_step_expert(h, 1, None, None), "GF_ESTATE",
     NEED_STREAMS),
    ("step_expert_hidden", "hidden_seeded", lambda n, l, h: l.cov_step_expert(h, 1, None, None), "GF_EINVAL",
     "cov_step_expert: " + HIDDEN_FUSED),
    ("explore_expert_not_hidden", "seeded", lambda n, l, h: l.cov_explore_expert(h, 1, None), "GF_ESTATE",
     "cov_explore_expert: the handle does not hide nodes (cov_set_hidden); cov_step_expert is its form"),
    ("explore_expert_no_state", "hidden_graph", lambda n, l, h: l.cov_explore_expert(h, 1, None), "GF_ESTATE",
     NEED_RESET),
    ("explore_expert_no_streams", "hidden_state", lambda n, l, h: l.cov_explore_expert(h, 1, None), "GF_ESTATE",
     NEED_STREAMS),
    ("controller_greedy_no_state", "graph", lambda n, l, h: l.cov_controller_greedy(h, None, None, None), "GF_ESTATE",
     NEED_RESET),
    ("get_rng_without_streams", "state", lambda n, l, h: l.cov_get_rng(h, n.ptr(np.zeros((B, 624), np.uint32)),
                                                                      n.ptr(np.zeros(B, np.int32))),
     "GF_ESTATE", "no np_random streams on the device (cov_set_rng)"),
    # argument refusals
    ("step_expert_zero_steps", "seeded", lambda n, l, h: l.cov_step_expert(h, 0, None, None), "GF_EINVAL",
     "n_steps must be at least 1"),
    ("explore_expert_zero_steps", "hidden_seeded", lambda n, l, h: l.cov_explore_expert(h, 0, None), "GF_EINVAL",
     "n_steps must be at least 1"),
    ("explore_expert_record_every", "hidden_seeded",
     lambda n, l, h: l.cov_explore_expert(h, 3, ctypes.byref(_rollout(n, 2))), "GF_EINVAL",
     "record_every must be at least 1 and divide n_steps"),
    ("explore_expert_record_every_zero", "hidden_seeded",
     lambda n, l, h: l.cov_explore_expert(h, 2, ctypes.byref(_rollout(n, 0))), "GF_EINVAL",
     "record_every must be at least 1 and divide n_steps"),
    ("step_host_next_without_flag", "state",
     lambda n, l, h: l.cov_step_host(h, n.ptr(ACTS), None, None, None, None, None, None, None, None, n.ptr(NEXT), None, 0),
     "GF_EINVAL", "next_actions / needs_random need COV_NEXT_GREEDY"),
    ("step_host_hidden", "hidden_state",
     lambda n, l, h: l.cov_step_host(h, n.ptr(ACTS), None, None, None, None, None, None, None, None, None, None, 0),
     "GF_EINVAL", "cov_step_host: " + HIDDEN_FUSED),
    ("step_host_bad_flags", "state",
     lambda n, l, h: l.cov_step_host(h, n.ptr(ACTS), None, None, None, None, None, None, None, None, None, None, 1),
     "GF_EINVAL", "flags: 0 or COV_NEXT_GREEDY"),
    ("maps_null_config", "fresh", lambda n, l, h: _maps(n, l, h, -1, n.COV_MAP_SEED, mc=None), "GF_EINVAL",
     "null map configuration"),
    ("maps_bad_flags", "fresh", lambda n, l, h: _maps(n, l, h, -1, 8), "GF_EINVAL", MAP_FLAGS),
    ("maps_cities_missing", "fresh", lambda n, l, h: _maps(n, l, h, -1, n.COV_MAP_CITIES), "GF_EINVAL",
     "COV_MAP_CITIES needs the cities"),
    ("maps_env_out_of_range", "fresh", lambda n, l, h: _maps(n, l, h, B, n.COV_MAP_SEED), "GF_EINVAL",
     "env index out of range"),
    ("maps_seed_too_large", "fresh", lambda n, l, h: _maps(n, l, h, -1, n.COV_MAP_SEED, seed=2 ** 32 - 1), "GF_EINVAL",
     "map_seed + n_envs must fit in 32 bits (np.random.seed)"),
    ("maps_unseeded_continuation", "fresh", lambda n, l, h: _maps(n, l, h, -1, 0), "GF_ESTATE",
     "the envs' map streams were never seeded (COV_MAP_SEED)"),
    ("submaps_bad_flags", "fresh", lambda n, l, h: l.cov_generate_submaps(h, -1, 0, None, 0, 8, None, None, None),
     "GF_EINVAL", SUB_FLAGS),
    ("submaps_without_pool", "fresh",
     lambda n, l, h: l.cov_generate_submaps(h, -1, 0, None, 0, n.COV_MAP_SEED, None, None, None), "GF_ESTATE",
     "no target pool (cov_load_occupancy)"),
    ("submaps_draws_missing", "fresh",
     lambda n, l, h: l.cov_generate_submaps(h, -1, 0, None, 1, n.COV_MAP_DRAWS, None, None, None), "GF_EINVAL",
     "COV_MAP_DRAWS needs the draws"),
    ("submaps_zero_draws", "fresh",
     lambda n, l, h: l.cov_generate_submaps(h, -1, 0, n.ptr(DRAWS), 0, n.COV_MAP_DRAWS, None, None, None), "GF_EINVAL",
     "COV_MAP_DRAWS needs n_draws >= 1"),
    ("submaps_too_many_draws", "fresh",
     lambda n, l, h: l.cov_generate_submaps(h, -1, 0, n.ptr(DRAWS), (1 << 20) + 1, n.COV_MAP_DRAWS, None, None, None),
     "GF_EINVAL", "n_draws too large"),
    ("submaps_env_out_of_range", "fresh",
     lambda n, l, h: l.cov_generate_submaps(h, B, 0, None, 0, n.COV_MAP_SEED, None, None, None), "GF_EINVAL",
     "env index out of range"),
    ("reset_device_bad_flags", "seeded", lambda n, l, h: _reset_device(n, l, h, 8), "GF_EINVAL",
     "flags: COV_RESET_SEED | COV_RESET_NEW_MAPS | COV_RESET_DONE"),
    ("reset_device_without_streams", "state", lambda n, l, h: _reset_device(n, l, h, 0), "GF_ESTATE",
     "no np_random streams on the device (cov_set_rng, cov_reset_seeded or COV_RESET_SEED)"),
    ("reset_device_done_before_state", "graph",
     lambda n, l, h: _reset_device(n, l, h, n.COV_RESET_SEED | n.COV_RESET_DONE), "GF_ESTATE",
     "COV_RESET_DONE: reset first (no done flags yet)"),
    ("reset_device_before_targets", "fresh", lambda n, l, h: _reset_device(n, l, h, n.COV_RESET_SEED), "GF_ESTATE",
     NEED_GRAPH),
    ("reset_device_new_maps_before_maps", "seeded",
     lambda n, l, h: _reset_device(n, l, h, n.COV_RESET_NEW_MAPS), "GF_ESTATE",
     "COV_RESET_NEW_MAPS: no maps were drawn from the map streams yet (cov_generate_maps / cov_generate_submaps)"),
    ("reset_device_first_must_take_all", "graph",
     lambda n, l, h: _reset_device(n, l, h, n.COV_RESET_SEED, np.array([1, 0], np.uint8)), "GF_ESTATE",
     "the first reset must take every env (the others have no state yet)"),
    # precedence: two checks would fire, the first one's text comes back
    ("first_state_then_flags", "graph", lambda n, l, h: l.cov_step(h, None, n.COV_GREEDY_RNG), "GF_ESTATE", NEED_RESET),
    ("first_hidden_then_rng_flags", "hidden_state", lambda n, l, h: l.cov_step(h, None, n.COV_ACTIONS_GREEDY | n.COV_GREEDY_RNG),
     "GF_EINVAL", "COV_ACTIONS_GREEDY: " + HIDDEN_FUSED),
    ("first_steps_then_hidden", "hidden_state", lambda n, l, h: l.cov_step_expert(h, 0, None, None), "GF_EINVAL",
     "n_steps must be at least 1"),
    ("first_hidden_then_steps", "state", lambda n, l, h: l.cov_explore_expert(h, 0, None), "GF_ESTATE",
     "cov_explore_expert: the handle does not hide nodes (cov_set_hidden); cov_step_expert is its form"),
    ("first_streams_then_steps", "hidden_state", lambda n, l, h: l.cov_explore_expert(h, 0, None), "GF_ESTATE",
     NEED_STREAMS),
    ("first_flags_then_env", "fresh", lambda n, l, h: _maps(n, l, h, B, 8), "GF_EINVAL", MAP_FLAGS),
    ("first_env_then_seed", "fresh", lambda n, l, h: _maps(n, l, h, B, n.COV_MAP_SEED, seed=2 ** 32 - 1), "GF_EINVAL",
     "env index out of range"),
    ("first_draws_then_env", "fresh",
     lambda n, l, h: l.cov_generate_submaps(h, B, 0, None, 1, n.COV_MAP_DRAWS, None, None, None), "GF_EINVAL",
     "COV_MAP_DRAWS needs the draws"),
    ("first_env_then_pool", "fresh",
     lambda n, l, h: l.cov_generate_submaps(h, B, 0, None, 0, n.COV_MAP_SEED, None, None, None), "GF_EINVAL",
     "env index out of range"),
    ("first_flags_then_streams", "state", lambda n, l, h: _reset_device(n, l, h, 8), "GF_EINVAL",
     "flags: COV_RESET_SEED | COV_RESET_NEW_MAPS | COV_RESET_DONE"),
    ("first_graph_then_streams", "fresh", lambda n, l, h: _reset_device(n, l, h, 0), "GF_ESTATE", NEED_GRAPH),
    ("first_flag_then_hidden_step_host", "hidden_state",
     lambda n, l, h: l.cov_step_host(h, n.ptr(ACTS), None, None, None, None, None, None, None, None, None, None, 1),
     "GF_EINVAL", "flags: 0 or COV_NEXT_GREEDY"),
]


@pytest.mark.parametrize("name,which,call,code,text", REFUSED, ids=[r[0] for r in REFUSED])
def test_refused_call_gives_its_code_and_text(nat, handles, name, which, call, code, text):
    lib = nat.load()
    rc = call(nat, lib, handles[which].h)
    got = lib.fe_last_error().decode()
    print("%s: code %d, text %r" % (name, rc, got))
    assert rc == getattr(nat, code)
    assert got == text


def _cycle(nat):
    """One handle through every path that allocates device memory on first use."""
    h = nat.CoverageHandle(R, B, M)
    h.set_targets(TARGETS)
    h.reset_seeded(5)                    # the np_random streams
    h.step(greedy=True, rng=True)        # the time matrices and greedy lists
    h.set_hidden(True)                   # the hidden observation
    out = h.explore_expert(2, record=("rewards", "done", "actions", "needs_random", "flat_obs"))  # the scratch
    assert out["rewards"].shape == (2, B)
    n_reset = h.reset_device(mask=np.array([1, 0]))[0]  # the reset's lists and regions
    assert n_reset == 1
    n, st, _ = h.generate_maps(map_seed=0, map_config=nat.map_config_default(xmax=8, ymax=8, n_cities=4))
    assert (n >= R).all() and (n <= TM).all() and not (st & ~nat.COV_MAP_NEAR_DEGENERATE).any()
    grid = np.zeros((16, 16), bool)
    grid[1::3, 1::3] = True              # every free cell within 1.5 cells of an occupied one
    cfg = nat.occupancy_config(perimeter_delta=1.5, num_subgraphs=5.0, min_targets=2, max_tries=64)
    assert h.load_occupancy(grid, cfg) == 200
    n, st, _ = h.generate_submaps(map_seed=0)
    assert (n >= R).all() and (n <= TM).all() and not st.any()
    h.close()


_LEAK_CHILD = """
import json, sys
import torch
assert torch.cuda.is_available()
sys.path[:0] = [{root!r}, {pkg!r}, {tests!r}]
import test_coverage_capi_errors_gpu as T
from gym_flock import _native as nat
free = []
for k in range(8):
    T._cycle(nat)
    torch.cuda.synchronize()
    free.append(torch.cuda.mem_get_info()[0])
print("FREE " + json.dumps(free))
"""


def test_closing_a_handle_returns_all_its_device_memory():
    """8 create / use / close cycles: the device's free memory (torch.cuda.mem_get_info) after
    the 8th equals that after the 2nd (the first cycles absorb the runtime's one-time
    allocations). torch is imported before gym_flock in a child process:
    this one stays torch-free."""
    here = os.path.dirname(os.path.abspath(__file__))
    root = os.path.dirname(here)
    code = _LEAK_CHILD.format(root=root, pkg=os.path.join(root, "gym-flock_amd"), tests=here)
    p = subprocess.run([sys.executable, "-c", code], capture_output=True, timeout=240)
    assert p.returncode == 0, p.stderr.decode()[-3000:]
    line = [ln for ln in p.stdout.decode().splitlines() if ln.startswith("FREE ")][-1]
    free = json.loads(line[len("FREE "):])
    print("bytes free after each cycle:", free)
    assert len(free) == 8 and free[7] == free[1], free
