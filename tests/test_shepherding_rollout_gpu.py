"""Shepherding-v0's recorded expert rollouts across episode ends (shep_expert_rollout,
gym-flock_amd/csrc/shepherd_rollout.hip). Needs an MI355X.

The launch is compared bit for bit with a second handle paced from the host: controller()
and step(expert=True) per step, the getters, and reset_device(envs=due) when an env's
episode step count reaches the episode length. Both run the same device code on the same
states, so nothing is compared under a tolerance except the reference's recorded episodes
(tests/golden/shepherding_episodes.npz), whose states carry NumPy's cos / sin.
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import GOLDEN, ROOT

pytestmark = pytest.mark.gpu

nat = pytest.importorskip("gym_flock._native")
from gym_flock.vec import VecShepherding  # noqa: E402

SHAPES = [(5, 10, 20), (4, 4, 60), (3, 3, 62), (2, 40, 160)]
ALL = ("obs", "adj", "actions", "rewards", "done", "n_resets")


def start(B, ns, nsheep, seed=40):
    """A batch reset on the device, with random headings so every controller row occurs."""
    v = VecShepherding(B, ns, nsheep)
    x = v.reset_device(seed=seed)
    x[..., 2] = np.random.RandomState(seed).uniform(-np.pi, np.pi, size=x.shape[:2])
    x[..., 0] -= v.goal_offset[0] * 0.9  # near the goal circle: the rewards move
    v.set_state(x)
    return v


def final(v):
    keys, pos = v.h.get_rng()
    return dict(x=v.get_state(), obs=v.obs(), adj=v.adj(), rewards=v.rewards(), controls=v.controls(), keys=keys,
                pos=pos, count=v.h.episode_steps())


def host_paced(v, n, L, every=1):
    """The contract's loop on handle v; the records as expert_rollout returns them."""
    B = v.n_envs
    rec = dict(obs=[], adj=[], actions=[], rewards=[], done=[], n_resets=np.zeros(B, np.int32))
    for t in range(n):
        rec["actions"].append(v.controller())
        v.step(expert=True)
        rec["rewards"].append(v.rewards())
        due = v.h.episode_steps() >= L if L > 0 else np.zeros(B, bool)
        rec["done"].append(due)
        if due.any():
            v.reset_device(envs=due, fetch=False)
            rec["n_resets"] += due
        if (t + 1) % every == 0:
            rec["obs"].append(v.obs())
            rec["adj"].append(v.adj())
    return {k: np.array(a) for k, a in rec.items()}


def same(got, want, what):
    assert sorted(got) == sorted(want), what
    for k in want:
        assert got[k].shape == want[k].shape, "%s: %s %s != %s" % (what, k, got[k].shape, want[k].shape)
        np.testing.assert_array_equal(got[k], want[k], err_msg="%s: %s" % (what, k))


@pytest.mark.parametrize("B,ns,nsheep", SHAPES)
def test_one_launch_equals_the_host_paced_twin(B, ns, nsheep):
    """24 steps with episodes of 7: resets at t = 6, 13, 20, away from the launch's ends."""
    v, w = start(B, ns, nsheep), start(B, ns, nsheep)
    np.testing.assert_array_equal(v.get_state(), w.get_state())
    got = v.expert_rollout(24, record=ALL, every=1, episode_length=7)
    want = host_paced(w, 24, 7)
    same(got, want, "records")
    np.testing.assert_array_equal(got["n_resets"], 3)
    np.testing.assert_array_equal(np.nonzero(got["done"][:, 0])[0], [6, 13, 20])
    same(final(v), final(w), "final")
    np.testing.assert_array_equal(final(v)["count"], 3)
    assert np.abs(got["actions"]).max() > 0 and np.count_nonzero(got["adj"]) > 0
    # every later call agrees too
    v.step(expert=True)
    w.step(expert=True)
    same(final(v), final(w), "a step later")
    v.close()
    w.close()


def test_launches_chain_and_honour_the_count():
    B, L = 5, 7
    v = start(B, 10, 20)
    whole = v.expert_rollout(14, record=ALL, episode_length=L)
    end = final(v)
    np.testing.assert_array_equal(whole["n_resets"], 2)
    for first in (5, 7):  # 7: the first launch ends on a done step, its reset inside it
        w = start(B, 10, 20)
        a = w.expert_rollout(first, record=ALL, episode_length=L)
        np.testing.assert_array_equal(w.h.episode_steps(), first % L)
        if first == 7:
            assert a["done"][-1].all() and np.all(a["n_resets"] == 1)
            np.testing.assert_array_equal(a["obs"][-1], w.obs())  # the reset state's observation
        b = w.expert_rollout(14 - first, record=ALL, episode_length=L)
        for k in ALL[:-1]:
            np.testing.assert_array_equal(np.concatenate([a[k], b[k]]), whole[k], err_msg="%d + %d: %s" % (first, 14 - first, k))
        np.testing.assert_array_equal(a["n_resets"] + b["n_resets"], whole["n_resets"])
        same(final(w), end, "%d + %d" % (first, 14 - first))
        w.close()
    # plain steps count: three of them, then a rollout whose first reset comes after 4 more
    w, u = start(B, 10, 20), start(B, 10, 20)
    for t in range(3):
        for h in (w, u):
            h.step(h.controller())
    np.testing.assert_array_equal(w.h.episode_steps(), 3)
    got = w.expert_rollout(6, record=ALL, episode_length=L)
    np.testing.assert_array_equal(np.nonzero(got["done"][:, 0])[0], [3])
    same(got, host_paced(u, 6, L), "after plain steps")
    same(final(w), final(u), "after plain steps, final")
    np.testing.assert_array_equal(w.h.episode_steps(), 2)
    # a count already past the length (the episode length shrank): the first step is done
    got = w.expert_rollout(2, record=("done",), episode_length=2)
    np.testing.assert_array_equal(got["done"], [[True] * B, [False] * B])
    w.close()
    u.close()
    # every fourth row
    w = start(B, 10, 20)
    got = w.expert_rollout(12, record=ALL, every=4, episode_length=L)
    w.close()
    w = start(B, 10, 20)
    each = w.expert_rollout(12, record=ALL, every=1, episode_length=L)
    w.close()
    v.close()
    assert got["obs"].shape == (3, B, 30, 4) and got["adj"].shape == (3, B, 30, 30)
    for k in ALL:
        np.testing.assert_array_equal(got[k], each[k][3::4] if k in ("obs", "adj") else each[k], err_msg=k)


@pytest.mark.parametrize("B,ns,nsheep", [(5, 10, 20), (3, 3, 62)])
def test_without_episodes_it_is_expert_steps_with_records(B, ns, nsheep):
    v, w = start(B, ns, nsheep), start(B, ns, nsheep)
    got = v.expert_rollout(9, record=ALL, episode_length=0)
    rews = w.expert_steps(9)
    np.testing.assert_array_equal(got["rewards"], rews)
    assert not got["done"].any() and not got["n_resets"].any()
    same(final(v), final(w), "final")
    np.testing.assert_array_equal(final(v)["count"], 9)
    np.testing.assert_array_equal(got["obs"][-1], v.obs())
    np.testing.assert_array_equal(got["adj"][-1], v.adj())
    assert len(np.unique(rews)) >= 2
    # a handle without streams rolls out too, as long as no episode ends
    u = VecShepherding(B, ns, nsheep)
    u.set_state(w.get_state())
    w.expert_steps(3)
    assert u.expert_rollout(3, record=("n_resets",))["n_resets"].sum() == 0
    np.testing.assert_array_equal(u.get_state(), w.get_state())
    for h in (v, w, u):
        h.close()


def test_float32_and_null_records():
    B = 5
    v, w = start(B, 10, 20), start(B, 10, 20)
    f64 = v.expert_rollout(10, record=ALL, every=5, episode_length=4)
    f32 = w.expert_rollout(10, record=ALL, every=5, episode_length=4, f32=True)
    for k in ALL:
        assert f32[k].dtype == (np.float32 if k in ("obs", "adj", "actions") else f64[k].dtype)
        np.testing.assert_array_equal(f32[k], f64[k].astype(f32[k].dtype), err_msg=k)
    same(final(v), final(w), "final")
    # NULL members are skipped: any subset gives the same arrays, none gives none
    for names in (("actions",), ("adj", "done"), ()):
        u = start(B, 10, 20)
        got = u.expert_rollout(10, record=names, every=5, episode_length=4)
        assert sorted(got) == sorted(names)
        for k in names:
            np.testing.assert_array_equal(got[k], f64[k], err_msg=k)
        assert u.expert_rollout(10, fetch=False, episode_length=4) is None
        u.close()
    v.close()
    w.close()


def test_refusals_leave_the_handle_usable():
    import ctypes
    B = 3
    v = VecShepherding(B)
    h = v.h
    reset = (v.r_max, v.goal_offset)

    def refused(code, call):
        with pytest.raises(nat.GymFlockError) as e:
            call()
        assert e.value.code == code, str(e.value)

    refused(nat.GF_ESTATE, lambda: h.expert_rollout(4))  # no state
    v.set_state(np.random.RandomState(0).uniform(-3, 3, size=(B, 30, 3)))
    refused(nat.GF_ESTATE, lambda: h.expert_rollout(4, episode_length=2, reset=reset))  # no streams
    h.set_rng(np.random.RandomState(1), env=0)
    refused(nat.GF_ESTATE, lambda: h.expert_rollout(4, episode_length=2, reset=reset))  # not all of them
    h.set_rng([np.random.RandomState(b) for b in range(B)])
    for n, every in ((0, 1), (-3, 1), (4, 0), (4, -1), (4, 3), (4, 8)):
        refused(nat.GF_EINVAL, lambda: h.expert_rollout(n, every=every))
    refused(nat.GF_EINVAL, lambda: h.expert_rollout(4, episode_length=-1, reset=reset))
    refused(nat.GF_EINVAL, lambda: h.expert_rollout(4, episode_length=2))  # null reset config
    for bad in (0.0, -2.0, np.inf, np.nan):
        refused(nat.GF_EINVAL, lambda: h.expert_rollout(4, episode_length=2, reset=(bad, v.goal_offset)))
    refused(nat.GF_EINVAL, lambda: h.expert_rollout(4, flags=0x1))
    refused(nat.GF_EINVAL, lambda: h.expert_rollout(4, flags=0x10 | nat.SHEP_REC_F32))
    assert nat.load().shep_expert_rollout(None, 4, 1, 0, None, None, 0) == nat.GF_EINVAL
    assert nat.load().shep_get_episode_steps(h.h, None) == nat.GF_EINVAL
    np.testing.assert_array_equal(h.episode_steps(), 0)  # nothing ran
    assert nat.load().shep_expert_rollout(h.h, 4, 2, 0, None, None, 0) == nat.GF_OK  # records may be NULL
    v.sync()
    np.testing.assert_array_equal(h.episode_steps(), 4)
    got = v.expert_rollout(4, record=ALL, episode_length=3)
    np.testing.assert_array_equal(got["n_resets"], 2)  # counts 4 >= 3: the first step ends an episode
    np.testing.assert_array_equal(got["done"][:, 0], [True, False, False, True])
    v.close()


_TORCH_FIRST = r"""
import json, sys
import numpy as np
import torch
assert torch.cuda.is_available()
sys.path[:0] = [{root!r}, {pkg!r}]
from gym_flock.vec import VecShepherding
B, n, every, L = 5, 12, 3, 5
def start():
    v = VecShepherding(B)
    x = v.reset_device(seed=8)
    x[..., 2] = np.random.RandomState(8).uniform(-3, 3, size=x.shape[:2])
    v.set_state(x)
    return v
v = start()
host = v.expert_rollout(n, record=("obs", "adj", "actions", "rewards", "done", "n_resets"), every=every,
                        episode_length=L, f32=True)
end = v.get_state()
v.close()
v = start()
tdt = dict(float32=torch.float32, float64=torch.float64, uint8=torch.uint8, int32=torch.int32)
ok, guards_ok, tens = dict(), True, dict()
for name, (shape, dtype) in v.h.rollout_shapes(n, every, True).items():
    # a guard row before and after the record, every element poisoned
    t = torch.full((shape[0] + 2,) + tuple(shape[1:]), 77, dtype=tdt[np.dtype(dtype).name], device="cuda")
    tens[name] = t
torch.cuda.synchronize()
assert v.expert_rollout(n, every=every, episode_length=L, f32=True,
                        device_ptrs=dict((k, t[1:].data_ptr()) for k, t in tens.items())) is None
v.sync()
for name, t in tens.items():
    a = t.cpu().numpy()
    guards_ok = guards_ok and bool(np.all(a[0] == 77) and np.all(a[-1] == 77))
    ok[name] = bool(np.array_equal(a[1:-1], host[name].astype(a.dtype)))
poison_left = int(sum(np.count_nonzero(t.cpu().numpy()[1:-1] == 77) for k, t in tens.items() if k in ("obs", "actions")))
out = dict(ok=ok, guards_ok=guards_ok, poison_left=poison_left, state_ok=bool(np.array_equal(v.get_state(), end)),
           resets=host["n_resets"].tolist(), edges=int(np.count_nonzero(host["adj"])))
v.close()
print("RESULT " + json.dumps(out))
"""


def test_device_records_fill_torch_tensors_and_nothing_else():
    """The records written into torch tensors (torch imported first, in a child process, as
    INTEGRATION.md has it) equal the host ones; poisoned tensors are fully overwritten and
    the guard rows before and after them are not touched."""
    code = _TORCH_FIRST.format(root=ROOT, pkg=os.path.join(ROOT, "gym-flock_amd"))
    p = subprocess.run([sys.executable, "-c", code], capture_output=True, timeout=240)
    assert p.returncode == 0, p.stderr.decode()[-3000:]
    line = [ln for ln in p.stdout.decode().splitlines() if ln.startswith("RESULT ")][-1]
    out = json.loads(line[len("RESULT "):])
    assert all(out["ok"].values()) and len(out["ok"]) == 6, out
    assert out["guards_ok"] and out["poison_left"] == 0 and out["state_ok"], out
    assert out["resets"] == [2] * 5 and out["edges"] > 0, out


def test_the_references_episodes():
    """seed(s); reset(); three episodes of 20 controller() steps, each followed by a
    reset(), recorded from the reference: the device run reproduces the stream positions
    and the final key exactly, every reward exactly (the recorder's guards keep a one-ulp
    trig difference from flipping one), and the states within 100 x free_run_sensitivity,
    the margin and reasoning of test_free_running_rollout_stays_within_the_recorded_
    sensitivity (tests/test_shepherding_gpu.py)."""
    f = np.load(os.path.join(GOLDEN, "shepherding_episodes.npz"))
    L = int(f["episode_length"])
    bound = 100.0 * float(f["free_run_sensitivity"])
    v = VecShepherding(1, int(f["n_shepherds"]), int(f["n_sheep"]))
    assert v.r_max == float(f["r_max"]) and np.array_equal(v.goal_offset, f["goal_offset"])
    v.h.set_rng([np.random.RandomState(int(f["seed"]))])
    x = v.reset_device()
    assert v.h.get_rng(0)[1] == f["pos"][0]
    assert v.rewards()[0] == f["reward0"][0]
    worst = float(np.abs(x[0] - f["x0"][0]).max())
    got = v.expert_rollout(60, record=("obs", "rewards", "done", "n_resets"), episode_length=L)
    np.testing.assert_array_equal(got["rewards"][:, 0], f["reward"])
    np.testing.assert_array_equal(np.nonzero(got["done"][:, 0])[0], [19, 39, 59])
    assert got["n_resets"][0] == 3
    for t in range(60):
        want = f["x0"][(t + 1) // L] if (t + 1) % L == 0 else f["x"][t]
        worst = max(worst, float(np.abs(got["obs"][t, 0, :, :3] - want).max()))
    key, pos = v.h.get_rng(0)
    assert pos == f["final_pos"] == f["pos"][3]
    np.testing.assert_array_equal(key, f["final_key"])
    assert v.rewards()[0] == f["reward0"][3]
    v.close()
    print("deviation over three episodes %.3g, bound %.3g" % (worst, bound))
    assert worst <= bound
