"""Time of the flocking reset on the device (fe_reset_device) against the paths it replaces.

Writes profiles/flock_reset/flock_reset_timing.json (or --out): recorded figures, nothing is
asserted. Without --part the script touches no GPU itself: it runs each part as a child
process under its own `timeout` and stops at the first part that fails or runs out of time.
Device figures are host-clock times that end in a stream synchronise, after a warm-up call.

  a  512 envs x N=100, the reference's rejection sampler (env b on RandomState(b)):
       device         one fe_reset_device launch; per-try time = launch time / the slowest
                      env's try count
       dropin         512 sequential FlockingRelativeEnv.reset() in "reference" mode from
                      np.random.seed(b) (one host draw, upload, stats launch and fetch per
                      try, at most reset_max_attempts = 1000 tries), and in "device" mode
       numpy          the NumPy restatement (tests/flock_reset_numpy.py) on one core, measured
                      on the first 128 envs and extrapolated by the batch's try count
  b  256 envs x N=1024 without rejection (the synthetic init): fe_reset_device with
     FE_RESET_NO_REJECT, fe_reset_synthetic, and VecFlockingRelative.reset() /
     .reset_device(reject=False), which both end with compute_helpers
  c  8 of 256 envs at N=100 reset again: one masked fe_reset_device launch (rejection, and
     no-reject) against 8 x fe_set_state_env with host draws (one draw each, and the
     restatement's rejection loop each)

Usage:  python scripts/flock_reset_timing.py [--out PATH] [--repeats 5]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "gym-flock_amd"), os.path.join(ROOT, "tests")]

import flock_reset_numpy as frn  # noqa: E402

PART_TIMEOUT = {"a": 420, "b": 180, "c": 180}  # seconds, each part's own limit


def timed(run, repeats):
    """Median / min / max milliseconds of run() (which ends synchronised), after one warm-up."""
    run()
    ts = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        run()
        ts.append(1e3 * (time.perf_counter() - t0))
    return {"ms": statistics.median(ts), "min_ms": min(ts), "max_ms": max(ts), "repeats": repeats}


def part_a(repeats):
    import gym_flock
    from gym_flock.vec import VecFlockingRelative
    B, n = 512, 100
    out = {"n_envs": B, "n_agents": n}
    v = VecFlockingRelative(B, n)
    res = {}

    def run():
        res["t"], res["s"] = v.h.reset_device(0, max_tries=4096)
    r = timed(run, repeats)
    tries, status = res["t"], res["s"]
    r.update(tries_mean=float(tries.mean()), tries_max=int(tries.max()), tries_min=int(tries.min()),
             tries_total=int(tries.sum()), exhausted=int((status != 0).sum()), max_tries=4096,
             us_per_try_of_slowest_env=1e3 * r["ms"] / int(tries.max()))
    out["device"] = r

    def run_helpers():
        v.reset_device(seed=0, max_tries=4096, fetch=False)
        v.sync()
    out["device_with_compute_helpers"] = timed(run_helpers, repeats)
    v.close()

    class Cfg:
        def getfloat(self, k):
            return {"comm_radius": 0.9, "v_max": 5.0, "dt": 0.01}[k]

        def getint(self, k):
            return n

    import warnings
    for mode in ("device", "reference"):
        env = gym_flock.make("FlockingRelative-v0")
        env.params_from_cfg(Cfg())
        env.reset_mode = mode
        np.random.seed(0)
        env.reset()  # warm-up
        kept = 0
        t0 = time.perf_counter()
        with warnings.catch_warnings(record=True) as w:
            warnings.simplefilter("always")
            for b in range(B):
                np.random.seed(b)
                env.reset()
            kept = len(w)
        dt = time.perf_counter() - t0
        tr = np.minimum(tries, env.reset_max_attempts)
        out["dropin_" + mode] = {"ms": 1e3 * dt, "ms_per_reset": 1e3 * dt / B, "resets": B,
                                 "resets_that_kept_a_rejected_draw": kept,
                                 "us_per_try": 1e6 * dt / int(tr.sum()), "reset_max_attempts": env.reset_max_attempts}
        env.close()

    nb = 128  # measured on envs 0..127, the whole batch extrapolated by its try count
    t0 = time.perf_counter()
    total = 0
    for b in range(nb):
        total += frn.reset_rejection(np.random.RandomState(b), n, max_tries=4096, margins=False)["tries"]
    dt = time.perf_counter() - t0
    assert total == int(tries[:nb].sum())
    out["numpy_one_core"] = {"ms_measured": 1e3 * dt, "envs_measured": nb, "tries_measured": total,
                             "us_per_try": 1e6 * dt / total,
                             "ms_extrapolated_%d_envs" % B: 1e3 * dt / total * int(tries.sum())}
    return out


def part_b(repeats):
    from gym_flock.vec import VecFlockingRelative
    B, n = 256, 1024
    v = VecFlockingRelative(B, n)
    out = {"n_envs": B, "n_agents": n, "state_bytes": B * n * 32}

    def run_device():
        v.h.reset_device(0, reject=False, fetch=False)
        v.sync()

    def run_library():
        v.h.reset_synthetic(0)

    def run_vec_host():
        v.reset(seed=0)
        v.sync()

    def run_vec_device():
        v.reset_device(seed=0, reject=False, fetch=False)
        v.sync()
    out["device_no_reject"] = timed(run_device, repeats)
    out["fe_reset_synthetic"] = timed(run_library, repeats)
    out["vec_reset_host_draws_with_compute_helpers"] = timed(run_vec_host, repeats)
    out["vec_reset_device_with_compute_helpers"] = timed(run_vec_device, repeats)
    v.close()
    return out


def part_c(repeats):
    from gym_flock.init_states import draw_swarm
    from gym_flock.vec import VecFlockingRelative
    B, n = 256, 100
    sel = list(range(5, B, 32))  # 8 envs
    v = VecFlockingRelative(B, n)
    v.reset_device(seed=0, max_tries=4096)
    out = {"n_envs": B, "n_agents": n, "reset_envs": len(sel)}
    res = {}

    def run_masked():
        res["t"], _ = v.h.reset_device(None, sel, max_tries=4096)

    def run_masked_no_reject():
        v.h.reset_device(None, sel, reject=False, fetch=False)
        v.sync()
    rngs = [np.random.RandomState(1000 + b) for b in sel]

    def run_host_single():
        for b, rs in zip(sel, rngs):
            v.h.set_state(draw_swarm(n, np.sqrt(n), 5.0, 5.0, rs), env=b)

    def run_host_rejection():
        k = 0
        for b, rs in zip(sel, rngs):
            r = frn.reset_rejection(rs, n, max_tries=4096, margins=False)
            k += r["tries"]
            v.h.set_state(r["x"], env=b)
        res["host_tries"] = res.get("host_tries", 0) + k
        res["host_runs"] = res.get("host_runs", 0) + 1
    tr = []

    def run_masked_rec():
        run_masked()
        tr.append(int(res["t"][sel].max()))
    r = timed(run_masked_rec, repeats)
    r["slowest_env_tries_per_run"] = tr
    out["device_masked_rejection"] = r
    out["device_masked_no_reject"] = timed(run_masked_no_reject, repeats)
    out["host_single_draw_set_state_env"] = timed(run_host_single, repeats)
    r = timed(run_host_rejection, repeats)
    r["tries_per_run_mean"] = res["host_tries"] / res["host_runs"]
    out["host_rejection_draws_set_state_env"] = r
    v.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "flock_reset", "flock_reset_timing.json"))
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--part", choices=sorted(PART_TIMEOUT), help="run one part in this process (JSON on stdout)")
    a = ap.parse_args()
    if a.part:
        fn = {"a": part_a, "b": part_b, "c": part_c}[a.part]
        print("RESULT " + json.dumps(fn(a.repeats), sort_keys=True))
        return 0
    out, rc = {}, 0
    for part in sorted(PART_TIMEOUT):
        cmd = ["timeout", "-k", "10", str(PART_TIMEOUT[part]), sys.executable, os.path.abspath(__file__),
               "--part", part, "--repeats", str(a.repeats)]
        p = subprocess.run(cmd, stdout=subprocess.PIPE, universal_newlines=True)
        if p.returncode != 0:  # nothing more is started on the device after a failure
            out[part] = {"failed": p.returncode}
            rc = 1
            break
        line = [ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")][-1]
        out[part] = json.loads(line[len("RESULT "):])
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps(out, indent=1, sort_keys=True))
    return rc


if __name__ == "__main__":
    sys.exit(main())
