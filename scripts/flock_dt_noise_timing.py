"""What FlockingStochastic-v0's dt drawn on the device (fe_set_dt_noise) and the variants'
device reset (fe_reset_variant) cost, on one GPU, the modes interleaved in one process.

Writes profiles/flock_dt_noise/flock_dt_noise_timing.json (or --out): recorded figures,
nothing is asserted. Per shape (B envs x N agents, variant "stochastic") and round, each
from the same state with a fresh controller output, in this order:

  rollout_noise   expert_steps(n_steps, fetch=False) with dt_noise=(0.12, 0.018)
  rollout_fixed   the same on a handle with a per-env dt set once (fe_set_dt)
  host_paced      the faithful route without the mode: n_steps x (rs_b.normal(0.12, 0.018)
                  for every env b on the host, then step(expert=True, controller=True,
                  network="packed", dt=...))
  step_noise      n_steps x step(expert=True, controller=True, network="packed") with the
                  mode on: one draw launch and one step launch per step
  step_fixed      the same without the mode (per-env dt set once): split steps

and per shape
  reset_leader_device   reset_device(seed, kind="leader") of all B envs, waiting for tries
  reset_leader_host     the reference's rejection loop and the leaders' draw in NumPy for
                        --host-envs envs (a subset: the loop takes tens of ms per env),
                        reported per env and scaled to B

Every figure is a host-clock time that ends in a stream synchronise; the stepping modes are
divided by n_steps; the median over the rounds after one warm-up round.

Usage:  python scripts/flock_dt_noise_timing.py [--out PATH] [--rounds 3] [--steps 200]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "gym-flock_amd")]

SHAPES = [(512, 100), (4096, 100)]
MEAN, SIGMA = 0.12, 0.018


def host_leader_reset(rs, n, v_max=5.0, comm_radius=0.9):
    """flocking_relative.py:156-192 and flocking_leader.py:37-41 on a RandomState."""
    r_max, x = np.sqrt(n), np.zeros((n, 4))
    tries = 0
    while True:
        length = np.sqrt(rs.uniform(0, r_max, size=(n,)))
        angle = np.pi * rs.uniform(0, 2, size=(n,))
        x[:, 0] = length * np.cos(angle)
        x[:, 1] = length * np.sin(angle)
        bias = rs.uniform(low=-v_max, high=v_max, size=(2,))
        x[:, 2] = rs.uniform(low=-v_max, high=v_max, size=(n,)) + bias[0]
        x[:, 3] = rs.uniform(low=-v_max, high=v_max, size=(n,)) + bias[1]
        tries += 1
        loc = np.reshape(x[:, 0:2], (n, 2, 1))
        a = np.sum(np.square(np.transpose(loc, (0, 2, 1)) - np.transpose(loc, (2, 0, 1))), axis=2)
        np.fill_diagonal(a, np.inf)
        if not (np.min(np.sum((a < comm_radius * comm_radius).astype(int), axis=1)) < 2 or np.sqrt(np.min(a)) < 0.1):
            break
    x[:2, 2:4] = rs.uniform(low=-v_max, high=v_max)
    return x, tries


def summary(t):
    return {"median": statistics.median(t), "min": min(t), "max": max(t), "rounds": len(t)}


def time_shape(B, n, n_steps, rounds, host_envs):
    from gym_flock.init_states import synthetic_batch
    from gym_flock.vec import VecFlockingRelative
    x0 = synthetic_batch(B, n, seed0=0)
    noisy = VecFlockingRelative(B, n, variant="stochastic", dt_noise=(MEAN, SIGMA))
    noisy.reset_device(seed=0, reject=False)  # seeds the streams
    fixed = VecFlockingRelative(B, n, variant="stochastic")
    dt0 = np.random.RandomState(1).normal(MEAN, SIGMA, size=B)
    host_rs = [np.random.RandomState(b) for b in range(B)]

    def start(v):
        v.set_state(x0)
        if v is fixed:
            v.h.set_dt(dt0)
        v.controller()
        v.sync()

    def steps(v):
        for _ in range(n_steps):
            v.step(expert=True, controller=True, network="packed")

    def host_paced():
        for _ in range(n_steps):
            dts = np.array([rs.normal(MEAN, SIGMA) for rs in host_rs])
            fixed.step(expert=True, controller=True, network="packed", dt=dts)

    modes = {"rollout_noise": (noisy, lambda: noisy.expert_steps(n_steps, fetch=False)),
             "rollout_fixed": (fixed, lambda: fixed.expert_steps(n_steps, fetch=False)),
             "host_paced": (fixed, host_paced),
             "step_noise": (noisy, lambda: steps(noisy)),
             "step_fixed": (fixed, lambda: steps(fixed))}
    ts = {k: [] for k in modes}
    reset_dev = []
    for r in range(rounds + 1):  # round 0 warms up
        for name, (v, run) in modes.items():
            start(v)
            t0 = time.perf_counter()
            run()
            v.sync()
            el = time.perf_counter() - t0
            if r:
                ts[name].append(1e6 * el / n_steps)
        t0 = time.perf_counter()
        tries, status = noisy.reset_device(seed=1000 * r, kind="leader")
        noisy.sync()
        if r:
            reset_dev.append(1e3 * (time.perf_counter() - t0))
    t0 = time.perf_counter()
    host_tries = [host_leader_reset(np.random.RandomState(1000 * rounds + b), n)[1] for b in range(host_envs)]
    host_ms = 1e3 * (time.perf_counter() - t0) / host_envs
    same = [int(t) for t in tries[:host_envs]] == host_tries  # the same resets on both sides
    noisy.close()
    fixed.close()
    out = {"n_envs": B, "n_agents": n, "n_steps": n_steps}
    for name, t in ts.items():
        out[name] = dict(summary(t), unit="us per step")
    m = {k: out[k]["median"] for k in ts}
    out["rollout_noise_over_fixed"] = m["rollout_noise"] / m["rollout_fixed"]
    out["host_paced_over_rollout_noise"] = m["host_paced"] / m["rollout_noise"]
    out["step_noise_over_fixed"] = m["step_noise"] / m["step_fixed"]
    out["reset_leader_device"] = dict(summary(reset_dev), unit="ms for all envs", mean_tries=float(np.mean(tries)))
    out["reset_leader_host"] = {"ms_per_env": host_ms, "envs_measured": host_envs, "scaled_to_all_envs_ms": host_ms * B,
                                "same_try_counts_as_device": same,
                                "note": "measured on a subset of the envs (the device's first envs, the same seeds) and scaled"}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "flock_dt_noise", "flock_dt_noise_timing.json"))
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--host-envs", type=int, default=8)
    args = ap.parse_args()
    from gym_flock import _native as nat
    out = {"what": "host clock to a stream synchronise, median of rounds; stepping modes in us per step",
           "runtime": nat.runtime_info(), "shapes": []}
    for B, n in SHAPES:
        out["shapes"].append(time_shape(B, n, args.steps, args.rounds, args.host_envs))
        print(json.dumps(out["shapes"][-1]), flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(out, fh, indent=1, default=str)
        fh.write("\n")


if __name__ == "__main__":
    main()
