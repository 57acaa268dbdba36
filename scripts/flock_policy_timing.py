"""Time per step of the DAgger rollout (fe_step_policy) against the expert rollout and against
the host-paced loop it replaces, on one GPU, interleaved in one process.

Writes profiles/flock_policy/flock_policy_timing.json (or --out): recorded figures, nothing is
asserted. Per shape (B envs x N agents), network 24 -> 32 -> 32 -> 2 over 4 taps, and round
(modes interleaved, each from the same state and streams), in this order:

  policy_b0 / policy_b05 / policy_b1   policy_steps(n_steps) at beta 0, 0.5, 1 (rewards to the host)
  full_b0 / full_b05 / full_b1         the same with every record at every=1 into torch tensors
  expert                               expert_steps(n_steps) (rewards to the host)
  host_paced                           per step: step(device_ptr=u, controller=True) with the dense
                                       network written, wait, then in torch on the device the
                                       aggregation (products of the dense network with the delayed
                                       taps) and the same network, wait (beta = 0)

Every figure is a host-clock time that ends in a synchronise, divided by n_steps; the median,
minimum and maximum over the rounds after one warm-up round.

--ab --parent-lib PATH instead alternates this build with the parent commit's library (parent
first) on scripts/flock_rollout_timing.py and bench.py's headline, --rounds times each, and
writes profiles/flock_policy/ab_parent_new.txt.

Usage:  python scripts/flock_policy_timing.py [--out PATH] [--rounds 3] [--steps 200]
        python scripts/flock_policy_timing.py --ab --parent-lib PATH [--rounds 3]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

try:  # before gym_flock
    import torch
except ImportError:
    torch = None

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "gym-flock_amd")]

SHAPES = [(512, 100), (4096, 100)]
WIDTHS = (24, 32, 32, 2)
N_TAPS = 4
OUT_DIR = os.path.join(ROOT, "profiles", "flock_policy")


class DevArray:
    """A device buffer of the library for torch.as_tensor (no copy)."""

    def __init__(self, ptr, shape, typestr):
        self.__cuda_array_interface__ = {"shape": tuple(shape), "typestr": typestr, "data": (int(ptr), False), "version": 2}


def time_shape(B, n, n_steps, rounds):
    from gym_flock.vec import VecFlockingRelative
    rs = np.random.RandomState(0)
    ws = [rs.uniform(-0.3, 0.3, size=(WIDTHS[l + 1], WIDTHS[l])).astype(np.float32) for l in range(3)]
    bs = [rs.uniform(-0.3, 0.3, size=(WIDTHS[l + 1],)).astype(np.float32) for l in range(3)]
    v = VecFlockingRelative(B, n)
    v.set_policy(ws, bs, N_TAPS, clip=1.0)
    v.reset_device(seed=0, reject=False, fetch=False)
    x0 = v.get_state()  # (the streams go on from round to round: the draws cost the same)

    tdt = {np.float64: torch.float64, np.float32: torch.float32, np.uint64: torch.int64, np.int32: torch.int32,
           np.uint8: torch.uint8}
    shapes = v.h.policy_shapes(n_steps)
    dev = {k: torch.empty(s, dtype=tdt[d], device="cuda") for k, (s, d) in shapes.items()}
    ptrs = {k: t.data_ptr() for k, t in dev.items()}
    nbytes = sum(t.numel() * t.element_size() for t in dev.values())

    net = torch.nn.Sequential(torch.nn.Linear(24, 32), torch.nn.ReLU(), torch.nn.Linear(32, 32), torch.nn.ReLU(),
                              torch.nn.Linear(32, 2)).cuda()
    with torch.no_grad():
        for lin, w, b in zip([net[0], net[2], net[4]], ws, bs):
            lin.weight.copy_(torch.from_numpy(w))
            lin.bias.copy_(torch.from_numpy(b))
    buf = v.h.device_buffers()
    sv_t = torch.as_tensor(DevArray(buf.state_values, (B, n, 6), "<f4"), device="cuda")
    net_t = torch.as_tensor(DevArray(buf.network, (B, n, n), "<f4"), device="cuda")
    torch.cuda.synchronize()

    def start():
        v.set_state(x0)
        v.compute_helpers()
        v.reset_aggregation()
        v.controller()
        v.sync()

    def host_paced():
        z = torch.zeros((B, n, N_TAPS, 6), dtype=torch.float32, device="cuda")
        z[:, :, 0] = sv_t
        with torch.no_grad():
            u = torch.clamp(net(z.reshape(B, n, 24)), -1.0, 1.0).contiguous()
            torch.cuda.synchronize()
            for _ in range(n_steps):
                v.step(device_ptr=u.data_ptr(), controller=True)
                v.sync()
                zn = torch.empty_like(z)
                zn[:, :, 0] = sv_t
                zn[:, :, 1:] = torch.bmm(net_t, z[:, :, :-1].reshape(B, n, 18)).reshape(B, n, 3, 6)
                z = zn
                u = torch.clamp(net(z.reshape(B, n, 24)), -1.0, 1.0).contiguous()
                torch.cuda.synchronize()

    modes = {}
    for tag, beta in (("b0", 0.0), ("b05", 0.5), ("b1", 1.0)):
        modes["policy_" + tag] = lambda beta=beta: v.policy_steps(n_steps, beta=beta)
    for tag, beta in (("b0", 0.0), ("b05", 0.5), ("b1", 1.0)):
        modes["full_" + tag] = lambda beta=beta: v.policy_steps(n_steps, beta=beta, device_ptrs=ptrs)
    modes["expert"] = lambda: v.expert_steps(n_steps)
    modes["host_paced"] = host_paced
    ts = {k: [] for k in modes}
    for r in range(rounds + 1):  # round 0 warms up
        for name, run in modes.items():
            start()
            t0 = time.perf_counter()
            run()
            v.sync()
            dt = time.perf_counter() - t0
            if r:
                ts[name].append(1e6 * dt / n_steps)
    v.close()
    out = {"n_envs": B, "n_agents": n, "n_steps": n_steps, "widths": list(WIDTHS), "n_taps": N_TAPS,
           "record_bytes_per_step": nbytes // n_steps}
    for name, t in ts.items():
        out[name] = {"us_per_step": statistics.median(t), "min": min(t), "max": max(t), "rounds": len(t)}
    out["host_paced_over_policy_b0"] = out["host_paced"]["us_per_step"] / out["policy_b0"]["us_per_step"]
    out["policy_b0_over_expert"] = out["policy_b0"]["us_per_step"] / out["expert"]["us_per_step"]
    return out


def spread(vals):
    return "%9.2f (%8.2f-%8.2f)" % (statistics.median(vals), min(vals), max(vals))


def verdict(parent, this):
    m = statistics.median(this)
    if m > max(parent):
        return "median ABOVE the parent's spread"
    if m < min(parent):
        return "median below the parent's spread"
    return "median inside the parent's spread"


def ab(parent_lib, rounds, out_path):
    """flock_rollout_timing.py and bench.py's headline, the parent's library and this build's
    alternating (parent first)."""
    timing = {"parent": {}, "this": {}}
    bench = {"parent": [], "this": []}
    for _ in range(rounds):
        for who, lib in (("parent", parent_lib), ("this", None)):
            env = dict(os.environ)
            if lib:
                env["GYMFLOCK_LIB"] = lib
            with tempfile.TemporaryDirectory() as tmp:
                path = os.path.join(tmp, "t.json")
                cmd = ["timeout", "-k", "10", "300", sys.executable, os.path.join(ROOT, "scripts", "flock_rollout_timing.py"),
                       "--out", path, "--repeats", "3"]
                p = subprocess.run(cmd, capture_output=True, env=env)
                if p.returncode != 0:
                    raise SystemExit("flock_rollout_timing.py (%s) failed with %d: %s" % (who, p.returncode, p.stderr.decode()[-2000:]))
                for sh in json.load(open(path))["shapes"]:
                    for mode in ("loop", "rewards", "none", "full_device"):
                        if mode in sh:
                            timing[who].setdefault("%5d x %3d %-11s" % (sh["n_envs"], sh["n_agents"], mode), []).append(
                                sh[mode]["us_per_step"])
            cmd = ["timeout", "-k", "10", "300", sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "200",
                   "--warmup", "20", "--no-cpu-baseline", "--no-other-configs", "--no-controller-line", "--no-packed-line",
                   "--no-host-actions-line", "--no-knn-line"]
            p = subprocess.run(cmd, capture_output=True, env=env)
            if p.returncode != 0:
                raise SystemExit("bench.py (%s) failed with %d: %s" % (who, p.returncode, p.stderr.decode()[-2000:]))
            line = json.loads([ln for ln in p.stdout.decode().splitlines() if ln.startswith("{")][-1])
            bench[who].append(float(line["value"]))
    lines = ["What exists, against the parent commit's build on one MI355X, alternating (parent first), %d runs each." % rounds,
             "scripts/flock_rollout_timing.py --repeats 3 (us per step: median of the runs' figures, their range):"]
    for key in timing["parent"]:
        lines.append("  %s parent %s   this %s   %s" % (key, spread(timing["parent"][key]), spread(timing["this"][key]),
                                                         verdict(timing["parent"][key], timing["this"][key])))
    lines.append("bench.py --gpus 1 --steps 200 --warmup 20, the headline line (agent-steps/s):")
    for who in ("parent", "this"):
        lines.append("  %-6s median %.4e (%.4e-%.4e)" % (who, statistics.median(bench[who]), min(bench[who]), max(bench[who])))
    m = statistics.median(bench["this"])
    lines.append("  this build's median is %s the parent's spread" % (
        "BELOW (slower than)" if m < min(bench["parent"]) else ("above (faster than)" if m > max(bench["parent"]) else "inside")))
    os.makedirs(os.path.dirname(out_path), exist_ok=True)
    with open(out_path, "w") as fh:
        fh.write("\n".join(lines) + "\n")
    print("\n".join(lines))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--ab", action="store_true")
    ap.add_argument("--parent-lib", default=None)
    args = ap.parse_args()
    if args.ab:
        if not args.parent_lib or not os.path.exists(args.parent_lib):
            raise SystemExit("--ab needs --parent-lib: the parent commit's libgymflock.so")
        ab(os.path.abspath(args.parent_lib), args.rounds, args.out or os.path.join(OUT_DIR, "ab_parent_new.txt"))
        return
    if torch is None or not torch.cuda.is_available():
        raise SystemExit("the device-record and host-paced modes need torch with a GPU")
    from gym_flock import _native as nat
    out = {"what": "us per step, host clock to a synchronise; median, min, max over the rounds",
           "runtime": nat.runtime_info(), "shapes": []}
    for B, n in SHAPES:
        out["shapes"].append(time_shape(B, n, args.steps, args.rounds))
        print(json.dumps(out["shapes"][-1]), flush=True)
    path = args.out or os.path.join(OUT_DIR, "flock_policy_timing.json")
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with open(path, "w") as fh:
        json.dump(out, fh, indent=1, default=str)
        fh.write("\n")


if __name__ == "__main__":
    main()
