"""bench.py's plain run and `--dump-outputs DIR`: a plain run carries the headline only
(what `--full` adds is absent), `--steps` is the number of timed steps, and the arrays
written are the timed path's outputs after its last step. On the CPU: the sampling of
dump_outputs against a stand-in env. On an MI355X: a small run checked against the oracle
stepped warmup + steps times from the same seeded inputs."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

import bench

FULL_ONLY = ("cpu_baseline", "step_with_controller", "packed_network", "host_actions", "flocking_v0_knn7",
             "coverage_config4", "n8192_config5", "dropin", "dropin_coverage")


class FakeEnv:
    """The getters dump_outputs calls, over fixed arrays."""

    def __init__(self, B, N):
        rs = np.random.RandomState(1)
        self.n_envs, self.n_agents = B, N
        self.x = rs.randn(B, N, 4)
        self.sv = rs.randn(B, N, 6).astype(np.float32)
        self.net = rs.rand(B, N, N).astype(np.float32)
        self.rew = rs.randn(B)

    def get_state(self):
        return self.x

    def state_values(self):
        return self.sv

    def rewards(self):
        return self.rew

    def network(self, env):
        return self.net[env]


def test_dump_outputs_whole_and_sampled(tmp_path, monkeypatch):
    env = FakeEnv(6, 16)
    info = bench.dump_outputs(env, str(tmp_path / "a"))
    got = {k: np.load(str(tmp_path / "a" / (k + ".npy"))) for k in info}
    np.testing.assert_array_equal(got["x"], env.x)
    np.testing.assert_array_equal(got["state_values"], env.sv)
    np.testing.assert_array_equal(got["rewards"], env.rew)
    np.testing.assert_array_equal(got["network_sample"], env.net)  # every env fits
    assert got["x"].dtype == np.float64 and got["network_sample"].dtype == np.float32
    # a share that holds 2 envs' networks: 2 whole envs, ascending, the same from call to call
    monkeypatch.setattr(bench, "DUMP_NETWORK_BYTES", 2 * 4 * 16 * 16)
    bench.dump_outputs(env, str(tmp_path / "b"))
    bench.dump_outputs(env, str(tmp_path / "c"))
    nb, nc = (np.load(str(tmp_path / d / "network_sample.npy")) for d in "bc")
    np.testing.assert_array_equal(nb, nc)
    envs = [int(np.nonzero((env.net == n).all(axis=(1, 2)))[0][0]) for n in nb]
    assert len(envs) == 2 and envs == sorted(set(envs))
    # one env's network over the share: seeded rows of env 0
    monkeypatch.setattr(bench, "DUMP_NETWORK_BYTES", 5 * 4 * 16)
    bench.dump_outputs(env, str(tmp_path / "d"))
    nd = np.load(str(tmp_path / "d" / "network_sample.npy"))
    assert nd.shape == (5, 16)
    rows = [int(np.nonzero((env.net[0] == r).all(axis=1))[0][0]) for r in nd]
    assert rows == sorted(set(rows))
    # any other array over its share: a seeded sample of its leading axis
    monkeypatch.setattr(bench, "DUMP_ARRAY_BYTES", 3 * 16 * 4 * 8)
    info = bench.dump_outputs(env, str(tmp_path / "e"))
    xe = np.load(str(tmp_path / "e" / "x.npy"))
    assert xe.shape == (3, 16, 4) and "sample" in info["x"]
    assert all((env.x == a).all(axis=(1, 2)).any() for a in xe)


@pytest.mark.gpu
def test_plain_run_dumps_last_step_outputs(tmp_path):
    from gym_flock.init_states import synthetic_batch
    from oracle import flocking as orc
    B, N, K, W = 4, 64, 3, 2
    out = str(tmp_path / "dump")
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(K), "--warmup",
                        str(W), "--n-agents", str(N), "--n-envs", str(B), "--clock-warmup-ms", "1",
                        "--dump-outputs", out], capture_output=True, timeout=120)
    assert p.returncode == 0, p.stderr.decode()[-2000:]
    lines = p.stdout.decode().strip().splitlines()
    assert len(lines) == 1
    d = json.loads(lines[0])
    assert d["steps"] == K and d["warmup"] == W and d["unit"] == "agent-steps/s" and d["dtype"] == "f64"
    assert d["higher_is_better"] is True and d["ms_per_step"] > 0
    assert d["value"] == pytest.approx(B * N / (d["ms_per_step"] * 1e-3), rel=1e-9)
    assert not [k for k in FULL_ONLY if k in d]
    assert sorted(os.listdir(out)) == ["network_sample.npy", "rewards.npy", "state_values.npy", "x.npy"]
    got = {k: np.load(os.path.join(out, k + ".npy")) for k in d["dumped_outputs"]}
    assert sum(a.nbytes for a in got.values()) <= 64 << 20
    x = synthetic_batch(B, N, 0)
    u = np.random.RandomState(1234).uniform(-1, 1, size=(B, N, 2)).astype(np.float32)
    for b in range(B):
        for _ in range(W + K):
            ref = orc.step(x[b], u[b])
            x[b] = ref["x"]
        np.testing.assert_array_equal(got["x"][b], ref["x"])
        np.testing.assert_array_equal(got["network_sample"][b], ref["network"].astype(np.float32))
        np.testing.assert_allclose(got["state_values"][b], ref["state_values"], rtol=1e-5, atol=1e-8)
        np.testing.assert_allclose(got["rewards"][b], ref["reward"], rtol=1e-12)
