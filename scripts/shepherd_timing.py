"""Per-step time of Shepherding-v0 on the device and of the two NumPy forms on one core.

Writes profiles/shepherd/shepherd_timing.json (or --out): recorded figures, nothing is
asserted. Device figures are host-clock windows that end in a stream synchronise, every
shape warmed up first, the median of --repeats windows of at least --window seconds each:

  dropin_B1            ShepherdingEnv.step(u): one launch, the state, observation,
                       adjacency and reward brought to the host, per call
  resident_B{512,4096} VecShepherding.step(resident=True), one launch per step
  rollout_B{512,4096}  VecShepherding.expert_steps(100), 100 closed-loop steps per launch
                       (controller + step; the observation written once per launch)

CPU figures (this process, one core): the loop restatement (tests/shepherding_numpy.py)
and a whole-array NumPy step in the reference's operation order, per env and step,
measured on a few envs; a batch of B envs costs B times that on one core.

Usage:  python scripts/shepherd_timing.py [--out PATH] [--window 0.5] [--repeats 5]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "gym-flock_amd"), os.path.join(ROOT, "tests")]

import shepherding_numpy as sn  # noqa: E402


def numpy_step(x, u, ns, dt=0.01, scale=5.0, comm_r2=4.0, goal_r=None):
    """One env's step, observation, adjacency and reward on whole arrays, in the
    reference's operation order (shepherding.py:80-185)."""
    n = len(x)
    goal_r = sn.goal_region_radius(n) if goal_r is None else goal_r
    w = np.where(np.arange(n) < ns, sn.W_SHEPHERD, sn.W_SHEEP).reshape(1, n, 1)

    def pairs(x):
        d = x[:, None, :2] - x[None, :, :2]
        return d[:, :, 0] * d[:, :, 0] + d[:, :, 1] * d[:, :, 1], d

    r2, d = pairs(x)
    r2[r2 > 2] = np.inf
    np.fill_diagonal(r2, np.inf)
    rep = np.sum(w * (d / r2[:, :, None]), axis=1)
    full = np.vstack((u * scale, rep[ns:]))
    c, s = np.cos(x[:, 2]), np.sin(x[:, 2])
    v = full[:, 0] * c + full[:, 1] * s
    om = full[:, 0] * (-s / sn.D_OFFSET) + full[:, 1] * (c / sn.D_OFFSET)
    v[ns:] = v[ns:] / 2 + 0.5
    new = np.empty_like(x)
    new[:, 0] = x[:, 0] + v * c * dt
    new[:, 1] = x[:, 1] + v * s * dt
    new[:, 2] = x[:, 2] + om * dt
    r2, _ = pairs(new)
    np.fill_diagonal(r2, np.inf)
    adj = (r2 < comm_r2).astype(float) / np.sqrt(r2)
    rew = np.sum(np.sqrt(new[ns:, 0] * new[ns:, 0] + new[ns:, 1] * new[ns:, 1]) < goal_r) / (n - ns)
    return new, adj, rew


def windows(run, per_call, window, repeats):
    """Median seconds per step over `repeats` windows of >= `window` seconds; run(k) does k
    calls and ends synchronised; per_call: steps per call."""
    run(3)
    k = 1
    while True:
        t0 = time.perf_counter()
        run(k)
        dt = time.perf_counter() - t0
        if dt >= window:
            break
        k = max(k + 1, int(k * min(10.0, 1.3 * window / max(dt, 1e-6))))
    ts = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        run(k)
        ts.append((time.perf_counter() - t0) / (k * per_call))
    return {"us_per_step": 1e6 * statistics.median(ts), "min_us": 1e6 * min(ts), "max_us": 1e6 * max(ts),
            "calls_per_window": k, "steps_per_call": per_call, "windows": repeats}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "shepherd", "shepherd_timing.json"))
    ap.add_argument("--window", type=float, default=0.5)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--cpu-only", action="store_true", help="rehearsal: the NumPy figures only")
    a = ap.parse_args()
    ns, nsheep = 10, 20
    n = ns + nsheep
    out = {"n_shepherds": ns, "n_sheep": nsheep, "window_seconds": a.window, "device": {}, "cpu_one_core": {}}

    rs = np.random.RandomState(0)
    u1 = rs.uniform(-2, 2, size=(ns, 2)).astype(np.float32)
    if not a.cpu_only:
        import gym_flock
        from gym_flock.vec import VecShepherding
        env = gym_flock.make("Shepherding-v0")
        env.seed(0)
        env.reset()

        def run_env(k):
            for _ in range(k):
                env.step(u1)
        out["device"]["dropin_B1"] = dict(windows(run_env, 1, a.window, a.repeats), n_envs=1)
        env.close()
        for B in (512, 4096):
            v = VecShepherding(B)
            x0 = v.reset(seed=1)
            v.step(rs.uniform(-2, 2, size=(B, ns, 2)).astype(np.float32))

            def run_resident(k):
                for _ in range(k):
                    v.step(resident=True)
                v.sync()
            r = dict(windows(run_resident, 1, a.window, a.repeats), n_envs=B)
            r["env_steps_per_second"] = B / (r["us_per_step"] * 1e-6)
            out["device"]["resident_B%d" % B] = r
            v.set_state(x0)

            def run_rollout(k):
                for _ in range(k):
                    v.expert_steps(100, fetch=False)
                v.sync()
            r = dict(windows(run_rollout, 100, a.window, a.repeats), n_envs=B)
            r["env_steps_per_second"] = B / (r["us_per_step"] * 1e-6)
            out["device"]["rollout_B%d" % B] = r
            v.close()

    # one core: per env and step, on 4 envs' states
    from gym_flock.init_states import draw_shepherding
    r_max = np.sqrt(n)
    xs = []
    for b in range(4):
        x = np.zeros((n, 3))
        x[:, :2] = draw_shepherding(n, r_max, np.array([-3 * r_max, 0]), np.random.RandomState(b))
        x[:, 2] = np.random.RandomState(100 + b).uniform(-np.pi, np.pi, size=n)
        xs.append(x)
    new, adj, rew = numpy_step(xs[0], u1, ns)
    want = sn.step(xs[0], u1, ns)[0]
    assert np.array_equal(new, want) and np.array_equal(adj, sn.observe(want, ns)[1]) and rew == sn.observe(want, ns)[2]

    def run_restatement(k):
        for i in range(k):
            xn = sn.step(xs[i % 4], u1, ns)[0]
            sn.observe(xn, ns)

    def run_numpy(k):
        for i in range(k):
            numpy_step(xs[i % 4], u1, ns)
    for name, fn in (("restatement_loops", run_restatement), ("numpy_whole_array", run_numpy)):
        r = windows(fn, 1, a.window, a.repeats)
        r = {"us_per_env_step": r["us_per_step"], "min_us": r["min_us"], "max_us": r["max_us"]}
        for B in (1, 512, 4096):
            r["us_per_step_B%d_extrapolated" % B] = B * r["us_per_env_step"]
        out["cpu_one_core"][name] = r

    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps(out, indent=1, sort_keys=True))


if __name__ == "__main__":
    main()
