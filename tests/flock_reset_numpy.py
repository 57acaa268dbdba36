"""NumPy restatement of the reference's reset() rejection loop (flocking_relative.py:156-192)
on a given RandomState, with a cap on the tries, for the device reset's tests
(gym-flock_amd/csrc/flock_reset.hip). Besides the state it returns what the tests compare
and what keeps them honest: the try count, the stream afterwards, and per candidate the two
margins of the acceptance decision. The device computes positions with its own cos / sin,
so its a_ij can differ from NumPy's in the last places; a decision is only comparable when
both margins are far above that (test_flock_reset_cpu.py asserts 1e-12).

CASES lists every stream the GPU tests reset from, with the try counts the issue recorded;
the CPU test checks the counts and the margins, the GPU tests compare the device with the
same cached results.
"""
import functools

import numpy as np

MIN_DIST = 0.1    # :160
MIN_DEGREE = 2    # :164
MARGIN = 1e-12    # smallest decision margin the GPU tests accept


def reset_rejection(rs, n_agents, r_max=None, v_max=5.0, v_bias=None, comm_radius=0.9, max_tries=None,
                    reject=True, margins=True):
    """reset()'s loop on `rs` (a RandomState, or the np.random module), at most max_tries
    candidates (None: until one is accepted); reject=False keeps the first. Returns a dict:
    x (N,4) the last candidate, tries, accepted, state (rs.get_state() afterwards), dist_margin
    and a_margin (one entry per candidate: |sqrt(min a) - 0.1|, min |a_ij - comm_radius^2|;
    empty with margins=False, the reference's own work per try and nothing else)."""
    if r_max is None:
        r_max = np.sqrt(n_agents)
    if v_bias is None:
        v_bias = v_max
    comm_radius2 = comm_radius * comm_radius
    x = np.zeros((n_agents, 4))
    tries, accepted = 0, False
    dist_margin, a_margin = [], []
    while not accepted and (max_tries is None or tries < max_tries):
        length = np.sqrt(rs.uniform(0, r_max, size=(n_agents,)))
        angle = np.pi * rs.uniform(0, 2, size=(n_agents,))
        x[:, 0] = length * np.cos(angle)
        x[:, 1] = length * np.sin(angle)
        bias = rs.uniform(low=-v_bias, high=v_bias, size=(2,))
        x[:, 2] = rs.uniform(low=-v_max, high=v_max, size=(n_agents,)) + bias[0]
        x[:, 3] = rs.uniform(low=-v_max, high=v_max, size=(n_agents,)) + bias[1]
        tries += 1
        if not reject:
            accepted = True
            break
        x_loc = np.reshape(x[:, 0:2], (n_agents, 2, 1))
        a_net = np.sum(np.square(np.transpose(x_loc, (0, 2, 1)) - np.transpose(x_loc, (2, 0, 1))), axis=2)
        np.fill_diagonal(a_net, np.inf)
        min_dist = np.sqrt(np.min(np.min(a_net)))
        degree = np.min(np.sum((a_net < comm_radius2).astype(int), axis=1))
        if margins:
            dist_margin.append(abs(min_dist - MIN_DIST))
            a_margin.append(np.min(np.abs(a_net - comm_radius2)) if n_agents > 1 else np.inf)
        accepted = not (degree < MIN_DEGREE or min_dist < MIN_DIST)
    return dict(x=x.copy(), tries=tries, accepted=accepted, state=rs.get_state(),
                dist_margin=np.array(dist_margin), a_margin=np.array(a_margin))


def stream(kind, s):
    """The streams of the GPU tests: "seed" RandomState(s); "odd" the same after one
    randint(4), which leaves it at an odd position (a double then takes its two words from
    either side of a key regeneration)."""
    rs = np.random.RandomState(s)
    if kind == "odd":
        rs.randint(4)
    return rs


# (kind, N, max_tries) -> {stream seed: tries}: the counts recorded with the reference's loop
CASES = {
    ("seed", 10, 2048): dict(zip(range(8), (4, 127, 171, 445, 54, 63, 301, 38))),
    ("seed", 100, 2048): dict(zip(range(8), (541, 354, 363, 401, 211, 420, 251, 88))),
    ("odd", 37, 2048): dict(zip(range(8), (4, 14, 395, 108, 41, 359, 152, 212))),
    ("odd", 100, 2048): dict(zip((1, 2, 5, 6), (126, 229, 140, 77))),
    ("seed", 150, 8): dict(zip(range(4), (8, 8, 8, 8))),  # exhaustion: none accepted
}
MASKED = dict(n=10, envs=6, reset=(1, 4), max_tries=2048)  # the masked test: a second reset of two envs


@functools.lru_cache(maxsize=None)
def case(kind, n, max_tries, s):
    """The restatement's result for one stream of CASES (computed once per process)."""
    return reset_rejection(stream(kind, s), n, max_tries=max_tries)


@functools.lru_cache(maxsize=None)
def masked_case(b):
    """Env b of the masked test continued: a second reset on the stream its first one left."""
    rs = np.random.RandomState()
    rs.set_state(case("seed", MASKED["n"], MASKED["max_tries"], b)["state"])
    return reset_rejection(rs, MASKED["n"], max_tries=MASKED["max_tries"])


def golden_case(seed, n, r_max):
    """The drop-in test: the global stream np.random.seed(seed) of the recorded fixture."""
    rs = np.random.RandomState(seed)
    return reset_rejection(rs, n, r_max=r_max)
