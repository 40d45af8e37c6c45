"""Measure the fused first GNN layer (gsm_env_conv: TransformerConv(7, C,
heads) straight from the env-form graph) against the path it replaces, in one
process: gnn.env_csr + TransformerConv.forward under no_grad (four Linear(7,
HC) GEMMs + gsm_attn_aggregate). Shapes: 24 agents x 8192 envs (H) and 3 x
4096; layouts: after a reset, and roll_states.crowd (every entity of an env
inside a few contact distances: long rows). One JSON line per case, all of them
written to profiles/env_conv.json (or $ENV_CONV_OUT).

Algorithmic bytes, n = B*E nodes, nE entries, R output rows an env:
  fused     node table 28 n, entries 12 nE (row, col, distance), edge_ptr
            8 (B+1), out 4 HC B R, row_ptr_out 8 (n+1) when asked for; the
            weights (at most 8 KB) are not counted
  composed  env_csr: rows 4 nE read (and widened), counts and offsets 16 n;
            four projections: 4 x (28 n read + 4 HC n written); aggregation:
            q, k, v, skip read and out written 5 x 4 HC n, row_ptr 8 n, col and
            distance 8 nE (tools/bench_gnn.py)
"""
import json
import os
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "gs-marl_amd"))
sys.path.insert(0, str(ROOT / "tests"))
import torch  # noqa: E402

import roll_states  # noqa: E402
from gsmarl_amd import EnvConfig, GpuBatchEnv, gnn  # noqa: E402

DEV = "cuda:0"
heads, C = int(os.environ.get("GNN_HEADS", 3)), int(os.environ.get("GNN_C", 16))
HC = heads * C
REPS = int(os.environ.get("ENV_CONV_REPS", 50))


def timed(fn, reps):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps


def case(N, B, layout):
    env = GpuBatchEnv(EnvConfig(n_agents=N, n_envs=B, seed=1), DEV)
    env.reset(seed=1)
    if layout == "crowd":
        st = roll_states.crowd(N, N, B)
        env.set_state({k: torch.from_numpy(st[k]) for k in ("pos", "vel", "step_count")})
    out = env.observe()
    E, n = env.E, B * env.E
    nE = int(out["edge_ptr"][-1])
    torch.manual_seed(0)
    conv = gnn.TransformerConv(7, C, heads=heads).to(DEV)
    w, w_e = (t.detach() for t in gnn.pack_conv_params(conv))
    x = out["node_feat"].reshape(n, 7)
    ea = out["edge_attr"].reshape(-1, 1)
    args = (out["node_feat"], out["edge_ptr"], out["edge_index"], out["edge_attr"], w, w_e, heads)

    def composed():
        ptr = gnn.env_csr(out["edge_index"], n)
        return conv(x, ptr, out["edge_index"][1], ea)

    ptr = gnn.env_csr(out["edge_index"], n)
    col = out["edge_index"][1].contiguous()
    with torch.no_grad():
        t_all = timed(lambda: gnn.env_conv(*args, E, True, check=False), REPS)
        t_ptr = timed(lambda: gnn.env_conv(*args, E, True, row_ptr=True, check=False), REPS)
        t_agents = timed(lambda: gnn.env_conv(*args, N, True, check=False), REPS)
        t_method = timed(lambda: conv.forward_env(out), REPS)
        t_comp = timed(composed, REPS)
        t_fwd = timed(lambda: conv(x, ptr, col, ea), REPS)
        t_csr = timed(lambda: gnn.env_csr(out["edge_index"], n), REPS)
    base = 28 * n + 12 * nE + 8 * (B + 1)
    b_all, b_agents = base + 4 * HC * n, base + 4 * HC * B * N
    b_comp = 4 * nE + 16 * n + 4 * (28 * n + 4 * HC * n) + 5 * 4 * HC * n + 8 * n + 8 * nE
    env.close()

    def tbs(nbytes, ms):
        return round(nbytes / (ms * 1e-3) / 1e12, 3)

    return {
        "op": "gsm_env_conv (fused TransformerConv(7, C, heads) on the env-form graph)",
        "shape": f"{N} agents x {B} envs", "layout": layout, "nodes": n, "entries": nE,
        "mean_row": round(nE / n, 2), "heads": heads, "channels": C,
        "fused_all_rows_us": round(t_all * 1e3, 1), "fused_all_rows_with_row_ptr_us": round(t_ptr * 1e3, 1),
        "fused_agent_rows_us": round(t_agents * 1e3, 1),
        "forward_env_checked_us": round(t_method * 1e3, 1),
        "composed_env_csr_plus_forward_us": round(t_comp * 1e3, 1),
        "composed_forward_only_us": round(t_fwd * 1e3, 1), "env_csr_us": round(t_csr * 1e3, 1),
        "speedup_all_rows": round(t_comp / t_all, 2), "speedup_agent_rows": round(t_comp / t_agents, 2),
        "fused_all_rows_bytes": b_all, "fused_agent_rows_bytes": b_agents, "composed_bytes": b_comp,
        "fused_all_rows_TBs": tbs(b_all, t_all), "fused_agent_rows_TBs": tbs(b_agents, t_agents),
        "composed_TBs": tbs(b_comp, t_comp),
        "timing": f"torch.cuda events around {REPS} calls after 3 warm-up calls, one stream, one process; fused = "
                  "gnn.env_conv(check=False) (output and status allocations included); forward_env_checked adds "
                  "the status read (one host synchronisation a call)",
    }


lines = []
for N, B in ((24, 8192), (3, 4096)):
    for layout in ("reset", "crowd"):
        lines.append(json.dumps(case(N, B, layout)))
        print(lines[-1], flush=True)
dst = Path(os.environ.get("ENV_CONV_OUT") or ROOT / "profiles" / "env_conv.json")
dst.parent.mkdir(parents=True, exist_ok=True)
dst.write_text("\n".join(lines) + "\n")
