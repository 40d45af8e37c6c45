"""Measure minibatch assembly from a GraphRolloutBuffer: the torch composition
(graph_batch + gnn.env_csr + gnn.csr_transpose) against graph_batch_csr(check=
False) (gsm_graph_batch_ptr + gsm_graph_batch_gather), in one process, the two
alternating, K samples drawn over all slots and envs; and the GAE loop of
compute_returns against its one-launch kernel (gsm_gae). Shapes: 24 agents x
8192 envs with K = 8192, and 3 agents x 4096 envs (K = 4096); GAE at T = 100.
One JSON line, also written to profiles/graph_batch.json (or $GRAPH_BATCH_OUT).

Algorithmic bytes of the two assembly launches, per sample of E nodes and n
entries: read E*28 (node rows) + 12 n (src is searched, dst, edge_attr), write
E*28 + E*8 (row_ptr) + 12 n (col, edge_attr, t_edge); the index and offset
words (a few per sample) are not counted. GAE: reward and value read once,
returns written once (12 bytes per element and slot; done is 1 byte per env).
Shares are of the 8 TB/s HBM peak; they are shares of a whole call (launches,
allocations and host synchronisations included: a trainer waits for them too),
not of a kernel's own time. The GAE arrays at the large shape (3 x 79 MB) fit the
256 MiB Infinity Cache and are re-read call after call, so its rate is no HBM
rate."""
import json
import os
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "gs-marl_amd"))
import torch  # noqa: E402

from gsmarl_amd import EnvConfig, GpuBatchEnv, GraphRolloutBuffer, gnn  # noqa: E402

DEV = "cuda:0"
T_SLOTS = int(os.environ.get("GB_SLOTS", 4))      # stored slots the samples are drawn from (T_SLOTS + 1)
T_GAE = int(os.environ.get("GB_GAE_T", 100))
ROUNDS = int(os.environ.get("GB_ROUNDS", 10))
REPS = int(os.environ.get("GB_REPS", 10))


def timed_pair(old, new, rounds=ROUNDS, reps=REPS):
    """Median over rounds of the mean wall time of reps calls, the two
    alternating round by round; each window ends in a device synchronise."""
    for _ in range(3):
        old()
        new()
    torch.cuda.synchronize()
    a, b = [], []
    for _ in range(rounds):
        for fn, dst in ((old, a), (new, b)):
            t0 = time.perf_counter()
            for _ in range(reps):
                fn()
            torch.cuda.synchronize()
            dst.append((time.perf_counter() - t0) / reps)
    return sorted(a)[len(a) // 2], sorted(b)[len(b) // 2]


def assembly(n_agents, n_envs, K):
    env = GpuBatchEnv(EnvConfig(n_agents=n_agents, n_envs=n_envs, seed=1), DEV)
    buf = GraphRolloutBuffer(env, episode_length=T_SLOTS)
    buf.reset(seed=1)
    g = torch.Generator(device=DEV).manual_seed(0)
    for _ in range(T_SLOTS):
        buf.insert(torch.randint(0, 5, (env.B, env.N), dtype=torch.int32, device=DEV, generator=g))
    t_idx = torch.randint(0, T_SLOTS + 1, (K,), device=DEV, generator=g)
    b_idx = torch.randint(0, n_envs, (K,), device=DEV, generator=g)
    E = env.E

    def old():
        gb = buf.graph_batch(t_idx, b_idx)
        row_ptr = gnn.env_csr(gb["edge_index"], K * E)
        col = gb["edge_index"][1].to(torch.int32)
        return gb, row_ptr, col, gnn.csr_transpose(row_ptr, col)

    def new():
        return buf.graph_batch_csr(t_idx, b_idx, check=False)

    # the outputs being timed are the same ones
    gb, row_ptr, col, tr = old()
    c = new()
    assert int(c["status"].item()) == 0
    for x, y in ((c["row_ptr"], row_ptr), (c["col"], col), (c["transpose"][1], tr[1]), (c["transpose"][2], tr[2]),
                 (c["edge_attr"].view(torch.int32), gb["edge_attr"].view(torch.int32)),
                 (c["node_feat"].view(torch.int32), gb["node_feat"].view(torch.int32))):
        assert torch.equal(x, y)
    nE = col.numel()
    old_s, new_s = timed_pair(old, new)
    bytes_ = K * (E * 28 + E * 28 + E * 8) + 24 * nE
    ach = bytes_ / new_s / 1e9
    env.close()
    return {
        "buffer": f"{n_agents} agents x {n_envs} envs, {T_SLOTS + 1} slots", "samples": K, "nodes": K * E,
        "entries": nE, "torch_graph_batch_env_csr_csr_transpose_us": round(old_s * 1e6, 1),
        "graph_batch_csr_us": round(new_s * 1e6, 1), "speedup": round(old_s / new_s, 2),
        "algorithmic_bytes": int(bytes_), "achieved_GBs": round(ach, 1), "frac_of_8TBs": round(ach / 8000, 4),
    }


def gae(n_agents, n_envs, T):
    env = GpuBatchEnv(EnvConfig(n_agents=n_agents, n_envs=n_envs, seed=1, episode_length=25), DEV)
    buf = GraphRolloutBuffer(env, episode_length=T, edges_per_env=1)     # only rewards and dones matter here
    g = torch.Generator(device=DEV).manual_seed(0)
    buf.reward.normal_(generator=g)
    buf.done.copy_(torch.rand(T + 1, n_envs, device=DEV, generator=g) < 0.04)
    v = torch.randn(T + 1, n_envs, n_agents, device=DEV, generator=g)
    a, b = buf.compute_returns(v), buf.compute_returns(v, kernel=True)
    assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    old_s, new_s = timed_pair(lambda: buf.compute_returns(v), lambda: buf.compute_returns(v, kernel=True))
    bytes_ = T * n_envs * n_agents * 12 + (T + 1) * n_envs * (n_agents * 4 + 1)
    ach = bytes_ / new_s / 1e9
    env.close()
    return {
        "shape": f"T = {T}, {n_envs} envs x {n_agents} agents", "torch_loop_us": round(old_s * 1e6, 1),
        "gsm_gae_us": round(new_s * 1e6, 1), "speedup": round(old_s / new_s, 1),
        "algorithmic_bytes": int(bytes_), "achieved_GBs": round(ach, 1), "frac_of_8TBs": round(ach / 8000, 4),
        "note": "repeated calls on the same arrays: what fits the 256 MiB Infinity Cache is re-read from it",
    }


line = json.dumps({
    "op": "minibatch assembly (gsm_graph_batch_ptr + gsm_graph_batch_gather) and GAE (gsm_gae) against the torch "
          "paths they stand in for",
    "assembly_24x8192": assembly(24, 8192, 8192),
    "assembly_3x4096": assembly(3, 4096, 4096),
    "gae_24x8192": gae(24, 8192, T_GAE),
    "gae_3x4096": gae(3, 4096, T_GAE),
    "timing": f"host clock around {REPS} calls ending in a device synchronise, median of {ROUNDS} rounds, old and "
              "new alternating round by round after 3 warm-up calls of each; every call includes its own host "
              "synchronisations (torch path: two; graph_batch_csr(check=False): one; GAE: none)",
})
print(line)
dst = Path(os.environ.get("GRAPH_BATCH_OUT") or ROOT / "profiles" / "graph_batch.json")
dst.parent.mkdir(parents=True, exist_ok=True)
dst.write_text(line + "\n")
