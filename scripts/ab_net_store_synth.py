"""The delta network store where it does not pay: in-process interleaved A/B of
FE_NET_FULL against FE_NET_DELTA (two handles, alternating rounds, the device time per step
of each round's window) on two synthetic workloads at N x B (default 1024 x 256), next to
the bench workload itself:

  bench   synthetic_batch, resident random actions (what bench.py times)
  static  zero velocities, zero actions: nothing changes from step to step
  dense   the synthetic positions (and velocities, so that the flock stays as dense over
          the window) scaled by DENSE_SCALE (default 0.25) so that the mean degree exceeds
          N/4, with the random actions: nearly every group holds a neighbour and every
          row's value changes

Prints one JSON object. Usage: [N=1024 B=256 ROUNDS=7 STEPS=30] python scripts/ab_net_store_synth.py"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "gym-flock_amd")]
from gym_flock import _native as nat  # noqa: E402
from gym_flock.init_states import synthetic_batch  # noqa: E402

N = int(os.environ.get("N", 1024))
B = int(os.environ.get("B", 256))
STEPS, ROUNDS = int(os.environ.get("STEPS", 30)), int(os.environ.get("ROUNDS", 7))
SCALE = float(os.environ.get("DENSE_SCALE", 0.25))

x_bench = synthetic_batch(B, N)
u_rand = np.random.RandomState(0).uniform(-1, 1, size=(B, N, 2)).astype(np.float32)
x_static = x_bench.copy()
x_static[:, :, 2:4] = 0.0
x_dense = x_bench.copy()
x_dense *= SCALE
workloads = {"bench": (x_bench, u_rand), "static": (x_static, np.zeros_like(u_rand)), "dense": (x_dense, u_rand)}

handles = {}
for name, mode in (("full", nat.FE_NET_FULL), ("delta", nat.FE_NET_DELTA)):
    h = nat.FlockHandle(N, B)
    h.set_network_store(mode)
    handles[name] = h

out = {"N": N, "B": B, "steps_per_window": STEPS, "rounds": ROUNDS}
for wname, (x0, u) in workloads.items():
    res = {k: [] for k in handles}
    deg = None
    for r in range(ROUNDS):
        for k, h in handles.items():
            h.set_state(x0)
            h.set_actions(u)
            h.step(None, nat.FE_U_RESIDENT)  # (a delta handle's record is filled before the window)
            h.step(None, nat.FE_U_RESIDENT)
            h.timing_start()
            for _ in range(STEPS):
                h.step(None, nat.FE_U_RESIDENT)
            ms, _ = h.timing_stop()
            res[k].append(1e3 * ms)
            if deg is None:
                deg = float(h.stats(0)[2].mean())
    same = np.array_equal(handles["full"].network(0).view(np.uint32), handles["delta"].network(0).view(np.uint32)) and \
        np.array_equal(handles["full"].network(B - 1).view(np.uint32), handles["delta"].network(B - 1).view(np.uint32))
    e = {"mean_degree_env0_after_window": deg, "networks_identical": bool(same)}
    for k, v in res.items():
        e[k + "_us"] = {"median": float(np.median(v)), "min": float(min(v)), "max": float(max(v))}
    e["delta_over_full"] = e["delta_us"]["median"] / e["full_us"]["median"]
    out[wname] = e
print(json.dumps(out, indent=1))
