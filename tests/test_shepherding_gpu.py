"""Shepherding-v0 on the device (gym-flock_amd/csrc/shepherd.hip) against the reference's
recorded episodes (tests/golden/shepherding_ep*.npz) and the NumPy restatement
(tests/shepherding_numpy.py). Needs an MI355X.

What contains no device trigonometry is compared bit for bit: the adjacency, the reward,
the sheep rows of the control, and the controller's branch choice (the recorder keeps every
tested angle at least 1e-9 rad from its threshold). The integrated state and the
controller's output are compared under the teacher-forced tolerance rtol = 1e-12, atol =
1e-12 * max(1, max|u|) over the full (N,2) control u: OpenCL-class double sin / cos are
within 4 ulp (9e-16 relative), which in the worst term, theta += w dt, is about
|u| / d * 9e-16 * dt = 3e-17 |u|; the tolerance leaves more than three decades over that.
"""
import ctypes
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import GOLDEN, ROOT

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import shepherding_numpy as sn  # noqa: E402

pytestmark = pytest.mark.gpu

nat = pytest.importorskip("gym_flock._native")
from gym_flock.vec import VecShepherding  # noqa: E402

RTOL = 1e-12
SEEN = {}  # the largest errors seen, for profiles/shepherd/parity.txt


def atol(u):
    return 1e-12 * max(1.0, float(np.abs(u).max()))


def check_close(got, want, u, what):
    err = float(np.abs(got - want).max())
    SEEN[what] = max(SEEN.get(what, 0.0), err)
    SEEN[what + " / atol"] = max(SEEN.get(what + " / atol", 0.0), err / atol(u))
    np.testing.assert_allclose(got, want, rtol=RTOL, atol=atol(u), err_msg=what)


def restate(x, u, ns, **kw):
    """The restatement's results for one state and action."""
    new, full = sn.step(x, u, ns, **kw)
    ctrl, rows, gap = sn.controller(x, ns)
    return dict(new=new, full=full, ctrl=ctrl, rows=rows, gap=gap)


@pytest.fixture(scope="module", params=[0, 1])
def ep(request):
    """A recorded episode, the restatement of each of its 61 states, and the device's
    results for the 61 states loaded as one batch of 61 envs."""
    f = np.load(os.path.join(GOLDEN, "shepherding_ep%d.npz" % request.param))
    ns, x = int(f["n_shepherds"]), f["x"]
    u = np.concatenate([f["u"], np.zeros_like(f["u"][:1])])  # the last state takes a zero action
    ref = [restate(x[t], u[t], ns) for t in range(61)]
    v = VecShepherding(61)
    v.set_state(x)
    dev = dict(obs=v.obs(), adj=v.adj(), rew=v.rewards(), ctrl=v.controller())
    v.step(u)
    dev.update(new=v.get_state(), full=v.controls(), new_obs=v.obs(), new_adj=v.adj(), new_rew=v.rewards())
    v.close()
    return dict(f=f, ns=ns, x=x, u=u, ref=ref, dev=dev)


def test_same_state_adjacency_and_reward_are_bit_exact(ep):
    f, dev, ns = ep["f"], ep["dev"], ep["ns"]
    for k, t in enumerate(f["adj_steps"]):
        np.testing.assert_array_equal(dev["adj"][t], f["adj"][k], err_msg="adjacency, state %d" % t)
    np.testing.assert_array_equal(dev["rew"], np.concatenate([[f["reward0"]], f["reward"]]))
    for t in range(61):
        obs, adj, rew = sn.observe(ep["x"][t], ns)
        np.testing.assert_array_equal(dev["obs"][t], obs)
        np.testing.assert_array_equal(dev["adj"][t], adj)
        assert dev["rew"][t] == rew
        # the observation of the stepped state: of the device's own new state, bit for bit
        obs, adj, rew = sn.observe(dev["new"][t], ns)
        np.testing.assert_array_equal(dev["new_obs"][t], obs)
        np.testing.assert_array_equal(dev["new_adj"][t], adj)
        assert dev["new_rew"][t] == rew


def test_same_state_sheep_controls_are_bit_exact(ep):
    ns = ep["ns"]
    for t in range(61):
        np.testing.assert_array_equal(ep["dev"]["full"][t], ep["ref"][t]["full"], err_msg="control, state %d" % t)
    assert np.abs(ep["dev"]["full"][:, ns:]).max() > 0


def test_same_state_controller_branch_choice_is_exact(ep):
    ns = ep["ns"]
    for t in range(61):
        assert ep["ref"][t]["gap"] >= 1e-9
        rows = sn.rows_of(ep["dev"]["ctrl"][t], ep["x"][t][:ns, 2])
        np.testing.assert_array_equal(rows, ep["ref"][t]["rows"], err_msg="state %d" % t)
        np.testing.assert_array_equal(rows, sn.rows_of(ep["f"]["controller"][t], ep["x"][t][:ns, 2]))


def test_teacher_forced_step_and_controller_match_the_reference(ep):
    f = ep["f"]
    for t in range(61):
        full = ep["ref"][t]["full"]
        if t < 60:
            check_close(ep["dev"]["new"][t], f["x"][t + 1], full, "teacher-forced state")
        check_close(ep["dev"]["new"][t], ep["ref"][t]["new"], full, "teacher-forced state")
        check_close(ep["dev"]["ctrl"][t], f["controller"][t], full, "controller output")


def _random_batch(B, ns, nsheep, seed):
    """States dense enough for pairs inside sqrt(2) and 2, headings all round, float32 actions."""
    rs = np.random.RandomState(seed)
    n = ns + nsheep
    x = np.empty((B, n, 3))
    x[..., :2] = rs.uniform(-1.0, 1.0, size=(B, n, 2)) * max(1.0, 0.9 * np.sqrt(n))
    x[..., 2] = rs.uniform(-np.pi, np.pi, size=(B, n))
    return x, rs.uniform(-2, 2, size=(B, ns, 2)).astype(np.float32)


# B = 5 leaves the last workgroup partly empty; N = 64 and 65 straddle the switch from a
# wave per env to a workgroup per env
SHAPES = [(1, 10, 20), (3, 10, 20), (5, 10, 20), (2, 1, 1), (3, 24, 40), (2, 25, 40), (2, 100, 100)]


@pytest.mark.parametrize("B,ns,nsheep", SHAPES)
def test_shapes_against_the_restatement(B, ns, nsheep):
    n = ns + nsheep
    x, u = _random_batch(B, ns, nsheep, 100 + n + B)
    v = VecShepherding(B, ns, nsheep)
    v.set_state(x)
    ctrl = v.controller()
    v.step(u)
    new, full, obs, adj, rew = v.get_state(), v.controls(), v.obs(), v.adj(), v.rewards()
    # three closed-loop steps in one launch equal three step(controller()) calls
    v.set_state(x)
    rews = v.expert_steps(3)
    roll = v.get_state()
    v.set_state(x)
    for t in range(3):
        v.step(v.controller())
        np.testing.assert_array_equal(v.rewards(), rews[t])
    np.testing.assert_array_equal(v.get_state(), roll)
    v.close()
    gr = sn.goal_region_radius(n)
    for b in range(B):
        ref = restate(x[b], u[b], ns)
        assert ref["gap"] >= 1e-9 and sn.pair_gap(x[b]) >= 1e-9
        np.testing.assert_array_equal(full[b], ref["full"])
        check_close(new[b], ref["new"], ref["full"], "shapes: state")
        check_close(ctrl[b], ref["ctrl"], ref["full"], "shapes: controller output")
        np.testing.assert_array_equal(sn.rows_of(ctrl[b], x[b][:ns, 2]), ref["rows"])
        o, a, r = sn.observe(new[b], ns, goal_radius=gr)
        np.testing.assert_array_equal(obs[b], o)
        np.testing.assert_array_equal(adj[b], a)
        assert rew[b] == r
        if n > 2:
            assert np.count_nonzero(a) > 0 and np.abs(ref["full"][ns:]).max() > 0


@pytest.mark.parametrize("ns,nsheep,inside", [(10, 20, (5, 10, 20)), (100, 100, (37, 50, 100))])
def test_reward_counts_sheep_inside_the_goal_circle(ns, nsheep, inside):
    """Sheep inside, outside and astride the goal circle, 1e-6 from its edge."""
    n = ns + nsheep
    R = sn.goal_region_radius(n)
    rs = np.random.RandomState(7)
    x, _ = _random_batch(3, ns, nsheep, 8)
    for b, k in enumerate(inside):
        ang = rs.uniform(0, 2 * np.pi, size=nsheep)
        rad = np.where(np.arange(nsheep) < k, R - 1e-6, R + 1e-6)
        if b == 0:
            rad = np.where(np.arange(nsheep) < k, rs.uniform(0, R - 1e-6, size=nsheep), rs.uniform(R + 1e-6, 3 * R, size=nsheep))
        perm = rs.permutation(nsheep)
        x[b, ns:, 0], x[b, ns:, 1] = (rad * np.cos(ang))[perm], (rad * np.sin(ang))[perm]
        x[b, :ns, :2] *= 0.1  # shepherds near the centre do not count
    v =VecShepherding(3, ns, nsheep)
    v.set_state(x)
    rew = v.rewards()
    v.close()
    for b, k in enumerate(inside):
        assert sn.goal_gap(x[b], ns) >= 0.9e-6
        assert rew[b] == sn.observe(x[b], ns)[2] == k / nsheep


def test_radius_comparisons_are_strict():
    """r2 > 2 drops a pair from the repulsion and r2 < 4 keeps it in the graph, both strict:
    a pair at exactly sqrt(2) repels, a pair at exactly 2 is not adjacent."""
    up, down = np.nextafter(1.0, 2.0), np.nextafter(2.0, 0.0)
    far = [100.0, 100.0, 0.3]
    x = np.array([[far, [0, 0, 0.1], [1, 1, 0.2], [2, 0, 0.3]],        # r2 = 2, 4, 2 exactly
                  [far, [0, 0, 0.1], [1, up, 0.2], [down, 0, 0.3]]])   # just over 2, just under 4
    assert 1.0 * 1.0 + up * up > 2.0 and down * down < 4.0
    v = VecShepherding(2, 1, 3)
    v.set_state(x)
    adj = v.adj()
    v.step(np.zeros((2, 1, 2), np.float32))
    full = v.controls()
    v.close()
    for b in range(2):
        np.testing.assert_array_equal(adj[b], sn.observe(x[b], 1)[1])
        np.testing.assert_array_equal(full[b, 1:], sn.sheep_control(x[b], 1))
    assert adj[0, 1, 3] == 0.0 and adj[0, 1, 2] == 1.0 / np.sqrt(2.0) and adj[1, 1, 3] == 1.0 / np.sqrt(down * down)
    assert np.all(full[0, 1] == [0.15 * 0.5 * (-1.0 / 2.0)] * 2)  # sheep 1 is pushed by sheep 2 only
    assert np.all(full[1, 1] == 0.0)                               # and by nobody once it is past sqrt(2)


def test_shepherd_branch_quirk_is_reproduced():
    """:253 on the device: a shepherd dead ahead is tested only when exactly one of the two
    states has an exactly-zero component (the states of tests/test_shepherding_cpu.py)."""
    base = np.array([[-5.0, 0.25, 0.5], [-3.0, 0.25, 0.7], [-9.0, 3.0, 0.3], [-9.0, -3.0, 0.2]])
    x = np.stack([base, base, base])
    x[0, 0, 2] = 1e-300           # generic
    x[1, 0, 2] = 0.0              # shepherd 0 has a zero, shepherd 1 none
    x[2, 0, 2] = x[2, 1, 2] = 0.0  # both have one
    v = VecShepherding(3, 2, 2)
    v.set_state(x)
    ctrl = v.controller()
    v.close()
    rows = np.array([sn.rows_of(ctrl[b], x[b, :2, 2]) for b in range(3)])
    np.testing.assert_array_equal(rows, [sn.controller(x[b], 2)[1] for b in range(3)])
    np.testing.assert_array_equal(rows[:, 0], [2, 1, 2])


def hip_runtime():
    nat.load()
    with open("/proc/self/maps") as f:
        paths = {ln.split()[-1] for ln in f if "libamdhip64.so" in ln}
    assert paths, "libamdhip64 is not mapped after loading libgymflock"
    hip = ctypes.CDLL(sorted(paths)[0])
    hip.hipMalloc.argtypes = [ctypes.POINTER(ctypes.c_void_p), ctypes.c_size_t]
    hip.hipFree.argtypes = [ctypes.c_void_p]
    hip.hipMemcpy.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int]
    return hip


def hmalloc(hip, n):
    p = ctypes.c_void_p()
    assert hip.hipMalloc(ctypes.byref(p), n) == 0
    return p.value


def test_action_precisions_and_sources():
    """float32 and float64 actions give NumPy's two products; resident and device-pointer
    actions equal host actions bit for bit."""
    hip = hip_runtime()
    B, ns = 3, 10
    x, u32 = _random_batch(B, ns, 20, 55)
    u64 = u32.astype(np.float64)
    v = VecShepherding(B)
    got = {}
    for name, u in (("f32", u32), ("f64", u64)):
        v.set_state(x)
        v.step(u)
        got[name] = (v.controls(), v.get_state())
        v.set_state(x)
        v.step(resident=True)
        np.testing.assert_array_equal(v.get_state(), got[name][1])
        np.testing.assert_array_equal(v.controls(), got[name][0])
        d = hmalloc(hip, u.nbytes)
        try:
            assert hip.hipMemcpy(d, u.ctypes.data, u.nbytes, 1) == 0
            v.set_state(x)
            v.step(device_ptr=d, f64=name == "f64")
            np.testing.assert_array_equal(v.get_state(), got[name][1])
            np.testing.assert_array_equal(v.controls(), got[name][0])
        finally:
            v.sync()
            hip.hipFree(d)
    v.close()
    np.testing.assert_array_equal(got["f32"][0][:, :ns], (u32 * np.float32(5.0)).astype(np.float64))
    np.testing.assert_array_equal(got["f64"][0][:, :ns], u64 * 5.0)
    assert np.any(got["f32"][0][:, :ns] != got["f64"][0][:, :ns])
    assert np.any(got["f32"][1] != got["f64"][1])


def test_calls_out_of_order_are_state_errors():
    h = nat.ShepherdHandle(2, 3, 1)
    for call in (lambda: h.step(np.zeros((1, 2, 2), np.float32)), h.observe, h.controller, lambda: h.step_expert(2),
                 h.get_state, h.obs):
        with pytest.raises(nat.GymFlockError) as e:
            call()
        assert e.value.code == nat.GF_ESTATE
    h.set_state(np.ones((1, 5, 3)))
    with pytest.raises(nat.GymFlockError) as e:
        h.step(None, nat.SHEP_U_RESIDENT)
    assert e.value.code == nat.GF_ESTATE and "resident" in str(e.value)
    h.close()


def test_rollout_equals_stepping_the_controller():
    """expert_steps(20) equals 20 calls of step(controller()) bit for bit: states and every
    reward (envs centred on the goal, so the rewards move)."""
    B = 5
    v = VecShepherding(B)
    x = v.reset(seed=11)
    x[..., 0] -= v.goal_offset[0]
    x[..., :2] *= 1.4  # some sheep inside the goal circle, some outside
    x[..., 2] = np.random.RandomState(12).uniform(-np.pi, np.pi, size=x.shape[:2])
    v.set_state(x)
    rews = v.expert_steps(20)
    roll, adj, obs = v.get_state(), v.adj(), v.obs()
    v.set_state(x)
    for t in range(20):
        v.step(v.controller())
        np.testing.assert_array_equal(v.rewards(), rews[t], err_msg="rewards, step %d" % t)
    np.testing.assert_array_equal(v.get_state(), roll)
    np.testing.assert_array_equal(v.adj(), adj)
    np.testing.assert_array_equal(v.obs(), obs)
    v.set_state(x)
    v.step(expert=True)  # the fused single step is the first of them
    assert np.array_equal(v.rewards(), rews[0])
    v.close()
    assert len(np.unique(rews)) >= 2 and rews.max() > 0


def test_free_running_rollout_stays_within_the_recorded_sensitivity():
    """Against the controller-driven episode over its 60 steps: the free-running states stay
    within 100 x free_run_sensitivity (a factor of ten for device trig at up to 4 ulp plus
    the roundings the one-ulp nudge does not model, a factor of ten of margin); the rewards
    equal the recorded ones exactly."""
    f = np.load(os.path.join(GOLDEN, "shepherding_ep0.npz"))
    assert str(f["policy"]) == "controller"
    bound = 100.0 * float(f["free_run_sensitivity"])
    v = VecShepherding(1)
    v.set_state(f["x"][:1])
    worst = 0.0
    for t in range(60):
        r = v.expert_steps(1)
        assert r[0, 0] == f["reward"][t]
        worst = max(worst, float(np.abs(v.get_state()[0] - f["x"][t + 1]).max()))
    last = v.get_state()
    v.set_state(f["x"][:1])
    r = v.expert_steps(60)
    np.testing.assert_array_equal(r[:, 0], f["reward"])
    np.testing.assert_array_equal(v.get_state(), last)  # one launch of 60 = 60 launches of one
    v.close()
    SEEN["free-running deviation over 60 steps"] = worst
    SEEN["free-running bound (100 x free_run_sensitivity)"] = bound
    print("free-running deviation %.3g, bound %.3g" % (worst, bound))
    assert worst <= bound


def test_drop_in_env_follows_the_recorded_episode():
    import gym_flock
    f = np.load(os.path.join(GOLDEN, "shepherding_ep1.npz"))
    env = gym_flock.make("Shepherding-v0")
    env.seed(int(f["seed"]))
    obs, adj = env.reset()
    np.testing.assert_array_equal(env.x, f["x"][0])
    np.testing.assert_array_equal(obs, np.hstack((f["x"][0], env.agent_identities)))
    np.testing.assert_array_equal(adj, f["adj"][0])
    check_close(env.controller(), f["controller"][0], f["controller"][0], "drop-in: controller output")
    for t in range(10):
        full = sn.step(f["x"][t], f["u"][t], 10)[1]
        (obs, adj), r, done, info = env.step(f["u"][t])
        check_close(env.x, f["x"][t + 1], full, "drop-in: state")
        assert obs.shape == (30, 4) and adj.shape == (30, 30) and obs.dtype == adj.dtype == np.float64
        np.testing.assert_array_equal(obs[:, :3], env.x)
        assert r == f["reward"][t] and isinstance(r, float) and done is False and info == {}
    np.testing.assert_array_equal(adj, sn.observe(env.x, 10)[1])
    env.x = f["x"][20].copy()  # a state assigned by the caller is what the next step starts from
    env.step(f["u"][20])
    check_close(env.x, f["x"][21], sn.step(f["x"][20], f["u"][20], 10)[1], "drop-in: state")
    env.close()


def test_float32_getters_write_device_memory():
    """The float32 observation, adjacency and rewards written into caller-owned device
    memory equal the host float64 results cast to float32 (a torch tensor as the
    destination: the torch-first child process below)."""
    hip = hip_runtime()
    B, ns, nsheep = 3, 10, 20
    x, _ = _random_batch(B, ns, nsheep, 77)
    v = VecShepherding(B)
    v.set_state(x)
    want = dict(obs=v.obs(), adj=v.adj(), rewards=v.rewards())
    for got, arr in zip(v.outputs(), want.values()):  # the three in one copy
        np.testing.assert_array_equal(got, arr)
    for name, arr in want.items():
        np.testing.assert_array_equal(getattr(v, name)(f32=True), arr.astype(np.float32))
        for f32 in (True, False):
            got = np.empty(arr.shape, np.float32 if f32 else np.float64)
            d = hmalloc(hip, got.nbytes)
            try:
                assert getattr(v, name)(f32=f32, device_ptr=d) is None
                v.sync()
                assert hip.hipMemcpy(got.ctypes.data, d, got.nbytes, 2) == 0
            finally:
                hip.hipFree(d)
            np.testing.assert_array_equal(got, arr.astype(got.dtype))
    v.close()


_TORCH_FIRST = r"""
import json, sys
import numpy as np
import torch
assert torch.cuda.is_available()
sys.path[:0] = [{root!r}, {pkg!r}]
from gym_flock.vec import VecShepherding
v = VecShepherding(4)
v.reset(seed=3)
v.step(np.random.RandomState(9).uniform(-2, 2, size=(4, 10, 2)).astype(np.float32))
obs, adj = v.obs(), v.adj()
t_obs = torch.empty((4, 30, 4), dtype=torch.float32, device="cuda")
t_adj = torch.empty((4, 30, 30), dtype=torch.float32, device="cuda")
torch.cuda.synchronize()
v.obs(f32=True, device_ptr=t_obs.data_ptr())
v.adj(f32=True, device_ptr=t_adj.data_ptr())
v.sync()
out = dict(obs_ok=bool(np.array_equal(t_obs.cpu().numpy(), obs.astype(np.float32))),
           adj_ok=bool(np.array_equal(t_adj.cpu().numpy(), adj.astype(np.float32))),
           edges=int(np.count_nonzero(adj)))
v.close()
print("RESULT " + json.dumps(out))
"""


def test_float32_getters_write_a_torch_tensor():
    """torch imported before gym_flock, in a child process: this one stays
    torch-free."""
    code = _TORCH_FIRST.format(root=ROOT, pkg=os.path.join(ROOT, "gym-flock_amd"))
    p = subprocess.run([sys.executable, "-c", code], capture_output=True, timeout=240)
    assert p.returncode == 0, p.stderr.decode()[-3000:]
    line = [ln for ln in p.stdout.decode().splitlines() if ln.startswith("RESULT ")][-1]
    out = json.loads(line[len("RESULT "):])
    assert out["obs_ok"] and out["adj_ok"] and out["edges"] > 0, out


def test_zz_report_the_largest_errors_seen():
    """The figures behind profiles/shepherd/parity.txt (written where GYMFLOCK_PARITY_OUT names a file)."""
    lines = ["%-50s %.3e" % (k, v) for k, v in sorted(SEEN.items())]
    print("\n".join(lines))
    path = os.environ.get("GYMFLOCK_PARITY_OUT")
    if path:
        with open(path, "w") as fh:
            fh.write("\n".join(lines) + "\n")
