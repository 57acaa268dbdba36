"""Time per step of collecting recorded multi-episode Shepherding-v0 demonstrations: the fused
call (shep_expert_rollout) against shep_step_expert (the floor: rewards only, no resets) and
against the route a trainer had before it, and the reset on the device against reset() on
the host.

Shapes: 512 and 4096 envs of 10 shepherds + 20 sheep, each in a child process of its own.
Inside it the modes are interleaved and the round repeated --repeats times (at least three),
every mode from the same reset_device(seed=0), one warm-up chunk first, then timed from the
first call until the device is done over 300 steps in chunks of 100:
  a    the route without this call: step(expert=True), obs and adj as float32 into device
       tensors after every step, and VecShepherding.reset() (host draws) every 100 steps;
  s    expert_steps(100), fetching the rewards: the floor;
  b    expert_rollout(100) recording the rewards only, fetched;
  c1   expert_rollout(100) recording obs, adj and actions as float32 into device tensors;
  c10  the same with every=10;
  d1   as c1 with episode_length=100 (every env resets inside the launch at each chunk's end);
  d10  as c10 with episode_length=100.
After the rounds, alone: reset_device(seed) of all envs, reset_device() of 8 envs and reset()
on the host, microseconds per call, the median of --repeats windows.

--parent-lib PATH: also runs scripts/shepherd_timing.py's device figures on that build of the
parent commit's library and on this tree's, alternating, --repeats times each; both series go
into the JSON with whether each of this tree's medians lies inside the parent's own spread.

  python scripts/shepherd_rollout_timing.py [--repeats 3] [--parent-lib PATH] [--out PATH]
Writes profiles/shepherd_rollout/shepherd_rollout_timing.json (or --out). Figures are
recorded, nothing is asserted.
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHUNK, N_CHUNKS, EP = 100, 3, 100
MODES = ("a", "s", "b", "c1", "c10", "d1", "d10")


def child(B, repeats):
    import numpy as np
    import torch  # before gym_flock
    assert torch.cuda.is_available()
    sys.path[:0] = [ROOT, os.path.join(ROOT, "gym-flock_amd")]
    from gym_flock.vec import VecShepherding
    v = VecShepherding(B)
    n = v.n_agents
    tdt = {np.float64: torch.float64, np.uint8: torch.uint8, np.int32: torch.int32, np.float32: torch.float32}
    dev = {}
    for every in (1, 10):
        sh = v.h.rollout_shapes(CHUNK, every, True)
        dev[every] = {k: torch.zeros(sh[k][0], dtype=tdt[sh[k][1]], device="cuda") for k in ("obs", "adj", "actions")}
    t_obs = torch.zeros((B, n, 4), dtype=torch.float32, device="cuda")
    t_adj = torch.zeros((B, n, n), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    ptrs = {e: {k: t.data_ptr() for k, t in d.items()} for e, d in dev.items()}

    def run(mode):
        if mode == "a":
            for _ in range(CHUNK):
                v.step(expert=True)
                v.obs(f32=True, device_ptr=t_obs.data_ptr())
                v.adj(f32=True, device_ptr=t_adj.data_ptr())
            v.reset(seed=0)  # the episode's end, as d1 / d10 reset at each chunk's last step
        elif mode == "s":
            v.expert_steps(CHUNK)
        elif mode == "b":
            v.expert_rollout(CHUNK, record=("rewards",))
        else:
            every = 10 if mode.endswith("10") else 1
            v.expert_rollout(CHUNK, every=every, episode_length=EP if mode[0] == "d" else None, f32=True,
                             device_ptrs=ptrs[every])

    us = {m: [] for m in MODES}
    for _ in range(repeats):
        for m in MODES:
            v.reset_device(seed=0, headings="zero", fetch=False)
            run(m)  # warm-up chunk of this mode
            v.reset_device(seed=0, headings="zero", fetch=False)
            v.sync()
            t0 = time.perf_counter()
            for _ in range(N_CHUNKS):
                run(m)
            v.sync()
            us[m].append(1e6 * (time.perf_counter() - t0) / (CHUNK * N_CHUNKS))

    def window(fn, seconds=0.3):
        fn()
        v.sync()
        k = 1
        while True:
            t0 = time.perf_counter()
            for _ in range(k):
                fn()
            v.sync()
            dt = time.perf_counter() - t0
            if dt >= seconds or k >= 4096:
                return 1e6 * dt / k
            k *= 2

    some = np.arange(8) * (B // 8)
    resets = {"reset_device_all": lambda: v.reset_device(seed=0, headings="zero", fetch=False),
              "reset_device_8_envs": lambda: v.reset_device(envs=some, fetch=False),
              "reset_host": lambda: v.reset(seed=0)}
    reset_us = {k: [window(fn) for _ in range(repeats)] for k, fn in resets.items()}
    res = {"envs": B, "n_shepherds": v.n_shepherds, "n_sheep": v.n_sheep, "steps": CHUNK * N_CHUNKS, "chunk": CHUNK,
           "episode_length": EP, "us_per_step": us, "reset_us_per_call": reset_us,
           "record_bytes_per_step_c1": sum(t.numel() * t.element_size() for t in dev[1].values()) / CHUNK}
    v.close()
    print("RESULT " + json.dumps(res))


def parent_comparison(parent_lib, repeats):
    """scripts/shepherd_timing.py's device figures on the parent's library and on this
    tree's, alternating."""
    series = {"parent": {}, "this": {}}
    script = os.path.join(ROOT, "scripts", "shepherd_timing.py")
    for _ in range(repeats):
        for who in ("parent", "this"):
            env = dict(os.environ)
            env.pop("GYMFLOCK_LIB", None)
            if who == "parent":
                env["GYMFLOCK_LIB"] = os.path.abspath(parent_lib)
            with tempfile.TemporaryDirectory() as d:
                out = os.path.join(d, "t.json")
                p = subprocess.run([sys.executable, script, "--out", out, "--window", "0.3", "--repeats", "3"], env=env,
                                   capture_output=True, timeout=600)
                if p.returncode != 0:
                    sys.stderr.write(p.stderr.decode()[-3000:])
                    raise SystemExit("shepherd_timing.py failed on the %s library (exit %d)" % (who, p.returncode))
                with open(out) as f:
                    dev = json.load(f)["device"]
            for k, r in dev.items():
                series[who].setdefault(k, []).append(r["us_per_step"])
    verdict = {}
    for k, xs in series["parent"].items():
        med = statistics.median(series["this"][k])
        verdict[k] = {"parent_min": min(xs), "parent_max": max(xs), "parent_median": statistics.median(xs),
                      "this_median": med, "this_inside_parent_spread_or_faster": med <= max(xs)}
    return {"us_per_step": series, "verdict": verdict, "runs_each": repeats,
            "method": "shepherd_timing.py --window 0.3 --repeats 3, parent and this tree alternating"}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "shepherd_rollout", "shepherd_rollout_timing.json"))
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--child", type=int, default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        child(a.child, max(a.repeats, 3))
        return
    out = {"modes": {"a": "step(expert=True) + obs/adj float32 to device tensors every step + reset() on the host every 100",
                     "s": "expert_steps(100), rewards fetched (floor)", "b": "expert_rollout(100), rewards only, fetched",
                     "c1": "expert_rollout(100): obs, adj, actions float32 into device tensors, every step",
                     "c10": "c1 with every=10", "d1": "c1 with episode_length=100", "d10": "c10 with episode_length=100"}}
    for B in (512, 4096):
        p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", str(B), "--repeats", str(a.repeats)],
                           capture_output=True, timeout=900)
        if p.returncode != 0:
            sys.stderr.write(p.stderr.decode()[-3000:])
            raise SystemExit("B=%d failed (exit %d)" % (B, p.returncode))
        r = json.loads([ln for ln in p.stdout.decode().splitlines() if ln.startswith("RESULT ")][-1][7:])
        med = {m: statistics.median(x) for m, x in r["us_per_step"].items()}
        r["median_us_per_step"] = med
        r["spread_us_per_step"] = {m: max(x) - min(x) for m, x in r["us_per_step"].items()}
        r["median_reset_us_per_call"] = {k: statistics.median(x) for k, x in r["reset_us_per_call"].items()}
        r["rollout_over_floor_b_over_s"] = med["b"] / med["s"]
        r["old_route_over_fused_a_over_d1"] = med["a"] / med["d1"]
        r["in_launch_resets_us_per_step_d1_minus_c1"] = med["d1"] - med["c1"]
        r["host_reset_over_device_reset"] = (r["median_reset_us_per_call"]["reset_host"]
                                             / r["median_reset_us_per_call"]["reset_device_all"])
        out["B%d" % B] = r
        print("B=%d: median us per step %s; resets us per call %s"
              % (B, json.dumps(med), json.dumps(r["median_reset_us_per_call"])), flush=True)
    if a.parent_lib:
        out["parent_comparison"] = parent_comparison(a.parent_lib, max(a.repeats, 3))
        print(json.dumps(out["parent_comparison"]["verdict"], indent=1), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print("wrote " + a.out)


if __name__ == "__main__":
    main()
