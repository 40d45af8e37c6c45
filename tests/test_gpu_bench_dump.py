"""A plain bench.py run on one MI355X with `--dump-outputs`: the line carries
the headline keys and none of what `--full` adds, and the dumped arrays are
the env's outputs after the last timed step — bit for bit those of the same
seeded env stepped eagerly here through the warmup, alignment and timed
steps with the bench's action sequence (each graph reads the sequence from
its start). The settle loop's pass count depends on the clock, so this also
holds the run to the same inputs whatever that count was."""
import json
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

import bench

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parents[1]
DEV = "cuda:0"


def test_plain_run_dumps_the_last_timed_step(tmp_path):
    from gsmarl_amd import EnvConfig, GpuBatchEnv
    B, N, K, W = 300, 3, 20, 5
    r = subprocess.run([sys.executable, "-u", str(ROOT / "bench.py"), "--gpus", "1", "--steps", str(K),
                        "--warmup", str(W), "--config", "c2", "--n-envs", str(B), "--dump-outputs", str(tmp_path)],
                       capture_output=True, text=True, timeout=100, cwd=str(ROOT))
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    d = json.loads(lines[0])
    assert d["steps"] == K and d["warmup"] == W and d["unit"] == "agent-steps/s" and d["dtype"] == "f32"
    assert d["higher_is_better"] is True and d["metric"] == bench.METRIC
    # ms_per_step is the time of one timed step (the line rounds it to 1e-5 ms)
    assert d["ms_per_step"] == pytest.approx(B * N / d["value"] * 1e3, abs=1e-5)
    assert d["roofline"] is None and d["cpu_baseline"] is None and "graph_device_us" not in d["timed_region"]
    assert d["timed_region"]["settle_steps"] >= 200 and d["timed_region"]["episode_boundaries"] == 1

    cfg = EnvConfig(seed=1234, scenario="navigation", n_agents=N, n_envs=B)
    EL = cfg.episode_length
    gen = torch.Generator(device=DEV)
    gen.manual_seed(1000)
    actions = torch.randint(0, 5, (EL, B, N), dtype=torch.int32, device=DEV, generator=gen)
    env = GpuBatchEnv(cfg, DEV)
    env.reset(seed=cfg.seed, sync_edges=False)
    for n in (W, bench.align_steps(W, K, EL), K):
        for t in range(n):
            env.step(actions[t], sync_edges=False)
    torch.cuda.synchronize()
    want = env.outputs()
    assert sorted(p.name for p in tmp_path.iterdir()) == sorted(f"{k}.npy" for k in want)
    assert int(want["edge_ptr"][B]) > 0 and float(want["node_feat"].abs().max()) > 0
    for k, t in want.items():
        a = np.load(tmp_path / f"{k}.npy")
        assert a.dtype in (np.float32, np.float64), k
        assert a.shape == tuple(t.shape), k
        assert np.array_equal(a, t.cpu().numpy().astype(a.dtype)), k
    env.close()
