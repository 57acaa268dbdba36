"""Time per step of collecting recorded multi-episode Coverage demonstrations: the fused call
(cov_expert_rollout) against cov_step_expert (the floor: nothing recorded but rewards and done,
no resets) and against the host-paced route on the same library.

Shapes (the two of README's Coverage rows):
  arl  4 robots x 512 envs x max_nodes 1000, CoverageARL maps sampled from an occupancy grid
       (tests/golden/grid_slice10.npy, or GYM_FLOCK_MAPS=path.npy), res 5.0, episode_length 50,
       nearby starts of 20 nodes;
  v0   Coverage-v0 at 200 robots x 512 envs x max_nodes 1000, every env its own map
       (generate_maps(map_seed=8)), episode_length 75, starts anywhere.
Each shape runs in a child process of its own; inside it the modes are interleaved and the
round repeated REPEATS times, every mode from the same reset(seed=0), timed from the first call
until the device is done, over N = 4 episode lengths of steps in chunks of CHUNK:
  s   expert_steps(CHUNK), fetching rewards and done: the floor;
  r   expert_rollout(CHUNK) recording rewards and done only;
  d   the same, also recording actions and the flat row of every step into device tensors;
  e   as d with every=10;
  ra  as r with auto_reset (every env resets at each episode end inside the launch);
  da  as d with auto_reset: recorded multi-episode data, the fused way;
  h   the host-paced route to the same data: step(greedy=True), flat_obs(f32, device_ptr) into
      the same row tensor, reset_envs("done") after every step.
Reported: microseconds per step and mode, the resets made, and the time per reset round that
ra - r implies (every env's workgroup resets in the same iterations, the episodes being of one
length, so a round is one reset of each env that is done).

  python scripts/cov_rollout_timing.py [--repeats 3] [--out PATH]
Writes profiles/cov_rollout/cov_rollout_timing.json (or --out).
"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B, M, CHUNK = 512, 1000, 50
MODES = ("s", "r", "d", "e", "ra", "da", "h")


def child(shape, repeats):
    import numpy as np
    import torch  # before gym_flock
    assert torch.cuda.is_available()
    sys.path[:0] = [ROOT, os.path.join(ROOT, "gym-flock_amd")]
    from gym_flock.vec import VecCoverage
    if shape == "arl":
        R, ep = 4, 50
        grid = np.load(os.environ.get("GYM_FLOCK_MAPS", os.path.join(ROOT, "tests", "golden", "grid_slice10.npy")))
        v = VecCoverage(B, R, max_nodes=M, episode_length=ep, res=5.0, nearby_starts=True)
        v.load_occupancy(grid)
        v.reset(seed=0, new_maps=True, map_seed=100)
    else:
        R, ep = 200, 75
        v = VecCoverage(B, R, max_nodes=M, episode_length=ep)
        v.generate_maps(map_seed=8)
        v.reset(seed=0)
    n_chunks = (4 * ep + CHUNK - 1) // CHUNK
    n = n_chunks * CHUNK
    tdt = {np.float64: torch.float64, np.uint8: torch.uint8, np.int32: torch.int32, np.float32: torch.float32}
    dev = {}
    for every in (1, 10):
        sh = v.h.rollout_shapes(CHUNK, every)
        dev[every] = {k: torch.zeros(sh[k][0], dtype=tdt[sh[k][1]], device="cuda")
                      for k in ("rewards", "done", "actions", "flat_obs")}
    row = torch.zeros((B, 15 * M + 1), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    ptrs = {e: {k: t.data_ptr() for k, t in d.items()} for e, d in dev.items()}
    resets = {}

    def run(mode):
        if mode == "s":
            v.expert_steps(CHUNK)
        elif mode in ("r", "ra"):
            out = v.expert_rollout(CHUNK, auto_reset=mode == "ra")
            if mode == "ra":
                resets["ra"] = resets.get("ra", 0) + int(out["n_resets"].sum())
        elif mode in ("d", "e", "da"):
            v.expert_rollout(CHUNK, every=10 if mode == "e" else 1, device_ptrs=ptrs[10 if mode == "e" else 1],
                             auto_reset=mode == "da")
        else:
            for _ in range(CHUNK):
                v.step(greedy=True)
                v.flat_obs(f32=True, device_ptr=row.data_ptr())
                resets["h"] = resets.get("h", 0) + v.reset_envs("done")[0]

    v.expert_steps(1)  # builds the time matrices and the greedy lists
    us = {m: [] for m in MODES}
    for _ in range(repeats):
        for m in MODES:
            v.reset(seed=0)
            run(m)  # warm-up chunk of this mode
            v.reset(seed=0)
            v.sync()
            resets.pop(m, None)
            t0 = time.perf_counter()
            for _ in range(n_chunks):
                run(m)
            v.sync()
            us[m].append(1e6 * (time.perf_counter() - t0) / n)
    res = {"shape": shape, "robots": R, "envs": B, "max_nodes": M, "episode_length": ep, "steps": n, "chunk": CHUNK,
           "us_per_step": us, "resets_last_round": resets,
           "record_bytes_per_step_d": sum(t.numel() * t.element_size() for t in dev[1].values()) / CHUNK}
    v.close()
    print("RESULT " + json.dumps(res))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cov_rollout", "cov_rollout_timing.json"))
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        child(a.child, a.repeats)
        return
    out = {"modes": {"s": "expert_steps (floor)", "r": "expert_rollout, rewards and done",
                     "d": "r + actions and rows of every step into device tensors", "e": "d with every=10",
                     "ra": "r with auto_reset", "da": "d with auto_reset",
                     "h": "host-paced: step(greedy=True), flat_obs(f32, device_ptr), reset_envs('done') every step"}}
    for shape in ("arl", "v0"):
        p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", shape, "--repeats", str(a.repeats)],
                           capture_output=True, timeout=900)
        if p.returncode != 0:
            sys.stderr.write(p.stderr.decode()[-3000:])
            raise SystemExit("shape %s failed (exit %d)" % (shape, p.returncode))
        r = json.loads([ln for ln in p.stdout.decode().splitlines() if ln.startswith("RESULT ")][-1][7:])
        med = {m: sorted(x)[len(x) // 2] for m, x in r["us_per_step"].items()}
        r["median_us_per_step"] = med
        r["spread_us_per_step"] = {m: max(x) - min(x) for m, x in r["us_per_step"].items()}
        rounds = max(r["resets_last_round"].get("ra", 0) / float(r["envs"]), 1e-9)
        r["us_per_reset_round_ra_minus_r"] = (med["ra"] - med["r"]) * r["steps"] / rounds
        r["host_paced_over_fused_recorded_h_over_da"] = med["h"] / med["da"]
        r["recording_us_per_step_d_minus_r"] = med["d"] - med["r"]
        r["rollout_over_floor_r_over_s"] = med["r"] / med["s"]
        out[shape] = r
        print("%s: median us per step %s" % (shape, json.dumps(med)), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
