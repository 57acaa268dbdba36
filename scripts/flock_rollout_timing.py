"""Time per step of the closed-loop expert rollout (fe_step_expert) against the loop of
closed-loop packed steps it replaces, on one GPU, interleaved in one process.

Writes profiles/flock_rollout/flock_rollout_timing.json (or --out): recorded figures,
nothing is asserted. Per shape (B envs x N agents) and repeat, each from the same state
with a fresh controller output, in this order:

  loop          n_steps calls of step(expert=True, controller=True, network="packed")
  rewards       expert_steps(n_steps) recording the rewards only (host destination)
  none          expert_steps(n_steps, fetch=False): nothing recorded
  full_device   every record at every=1 into device buffers (torch tensors, when torch is
                there; the buffers are allocated once, outside the timed region)
  full_host     the same into host arrays (shapes of at most --host-max-gb of records)

Every figure is a host-clock time that ends in a stream synchronise, divided by n_steps,
the median over the repeats after one warm-up round. --bench also runs bench.py's headline
and its coverage workload on this build and on the library named by --parent-lib,
alternating, and records their result lines.

Usage:  python scripts/flock_rollout_timing.py [--out PATH] [--repeats 5] [--steps 200]
                                               [--bench --parent-lib PATH]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

try:  # before gym_flock; only the device-destination rows need it
    import torch
except ImportError:
    torch = None

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "gym-flock_amd")]

SHAPES = [(512, 100), (4096, 100), (512, 256)]
ALL = ("x", "state_values", "adj_bits", "degree", "controls", "rewards")


def record_bytes(v, n_steps):
    return sum(int(np.prod(s)) * np.dtype(d).itemsize for s, d in v.h.rollout_shapes(n_steps).values())


def time_shape(B, n, n_steps, repeats, host_max_gb):
    from gym_flock.init_states import synthetic_batch
    from gym_flock.vec import VecFlockingRelative
    v = VecFlockingRelative(B, n)
    x0 = synthetic_batch(B, n, seed0=0)
    nbytes = record_bytes(v, n_steps)
    dev = None
    if torch is not None and torch.cuda.is_available():
        tdt = {np.float64: torch.float64, np.float32: torch.float32, np.uint64: torch.int64, np.int32: torch.int32}
        dev = {k: torch.empty(s, dtype=tdt[d], device="cuda") for k, (s, d) in v.h.rollout_shapes(n_steps).items()}
        torch.cuda.synchronize()

    def start():
        v.set_state(x0)
        v.controller()
        v.sync()

    def loop():
        for _ in range(n_steps):
            v.step(expert=True, controller=True, network="packed")

    modes = {"loop": loop,
             "rewards": lambda: v.expert_steps(n_steps),
             "none": lambda: v.expert_steps(n_steps, fetch=False)}
    if dev is not None:
        ptrs = {k: t.data_ptr() for k, t in dev.items()}
        modes["full_device"] = lambda: v.expert_steps(n_steps, device_ptrs=ptrs)
    if nbytes <= host_max_gb * 2 ** 30:
        modes["full_host"] = lambda: v.expert_steps(n_steps, record=ALL)
    ts = {k: [] for k in modes}
    for r in range(repeats + 1):  # round 0 warms up
        for name, run in modes.items():
            start()
            t0 = time.perf_counter()
            run()
            v.sync()
            dt = time.perf_counter() - t0
            if r:
                ts[name].append(1e6 * dt / n_steps)
    v.close()
    out = {"n_envs": B, "n_agents": n, "n_steps": n_steps, "record_bytes_per_step": nbytes // n_steps,
           "columns_per_thread": 16 if n <= 64 else (32 if n <= 128 else 64)}
    for name, t in ts.items():
        out[name] = {"us_per_step": statistics.median(t), "min": min(t), "max": max(t), "repeats": len(t)}
    out["loop_over_rollout_rewards"] = out["loop"]["us_per_step"] / out["rewards"]["us_per_step"]
    return out


def bench_lines(parent_lib, rounds):
    """bench.py's headline and coverage workload, this build and the parent's alternating."""
    res = {"this": {"flocking": [], "coverage": []}, "parent": {"flocking": [], "coverage": []}}
    for _ in range(rounds):
        for who, lib in (("parent", parent_lib), ("this", None)):
            for wl in ("flocking", "coverage"):
                env = dict(os.environ)
                if lib:
                    env["GYMFLOCK_LIB"] = lib
                cmd = ["timeout", "-k", "10", "300", sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1",
                       "--steps", "200", "--warmup", "20", "--no-cpu-baseline", "--workload", wl]
                if wl == "flocking":  # the headline line only
                    cmd += ["--no-other-configs", "--no-controller-line", "--no-packed-line", "--no-host-actions-line",
                            "--no-knn-line"]
                p = subprocess.run(cmd, capture_output=True, env=env)
                if p.returncode != 0:
                    raise SystemExit("bench.py (%s, %s) failed with %d: %s" % (who, wl, p.returncode, p.stderr.decode()[-2000:]))
                line = [ln for ln in p.stdout.decode().splitlines() if ln.startswith("{")][-1]
                res[who][wl].append(json.loads(line))
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "flock_rollout", "flock_rollout_timing.json"))
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--host-max-gb", type=float, default=2.0)
    ap.add_argument("--bench", action="store_true")
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--bench-rounds", type=int, default=2)
    args = ap.parse_args()
    out = {"what": "us per step, host clock to a stream synchronise, median of repeats", "shapes": []}
    if os.path.exists(args.out):  # a bench-only run keeps the shapes and the other way round
        out.update(json.load(open(args.out)))
    if args.bench:
        if not args.parent_lib or not os.path.exists(args.parent_lib):
            raise SystemExit("--bench needs --parent-lib: the parent commit's libgymflock.so")
        out["bench"] = bench_lines(os.path.abspath(args.parent_lib), args.bench_rounds)
    else:
        from gym_flock import _native as nat
        out["runtime"] = nat.runtime_info()
        out["shapes"] = []
        for B, n in SHAPES:
            out["shapes"].append(time_shape(B, n, args.steps, args.repeats, args.host_max_gb))
            print(json.dumps(out["shapes"][-1]), flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(out, fh, indent=1, default=str)
        fh.write("\n")


if __name__ == "__main__":
    main()
