"""Measure the training path of the fused first GNN layer: forward plus
backward of one TransformerConv(7, C, heads) on an env-form graph, three ways
in one process, the three alternating round by round:

  fused     gnn.env_conv_autograd (gsm_env_conv_fwd + gsm_env_conv_bwd): no
            [n, HC] tensor in either direction
  composed  gnn.env_csr + TransformerConv(kernel_backward=True).forward with the
            transposed graph prebuilt: four Linear(7, HC) GEMMs and their
            backward around gsm_attn_aggregate_fwd / gsm_attn_aggregate_bwd
  torch     gnn.env_conv_ref + autograd (what forward_env runs without the flag)

Shapes: 24 agents x 8192 envs and 3 x 4096; layouts: after a reset, and
roll_states.crowd (long rows). Every path gets gradients for the parameters
only and the same grad_out. One JSON line per case, written to
profiles/env_conv_backward.json (or $ENV_CONV_BWD_OUT). $ENV_CONV_BWD_CASES
selects cases ("24x8192:reset,3x4096:crowd"), $ENV_CONV_BWD_PATHS the paths.

Algorithmic bytes, n = B*E nodes, nE entries, H heads (weights, dw and the
workgroup partials, at most a few MB, are not counted):
  fused     forward: node table 28 n, entries 12 nE, edge_ptr 8 (B+1), out
            4 HC n and lse 4 H n written; backward: the same graph reads, plus
            the columns a second time (source pass, 4 nE; the searches hit
            cache), grad_out and out 8 HC n, lse 4 H n, a_ij and ds_ij written
            and read back 16 H nE (L2-resident by design, counted anyway)
  composed  forward as tools/bench_env_conv.py counts it plus lse 4 H n;
            backward: the aggregation's (tools/bench_gnn.py: g, q, k, v, out,
            skip read, dq, dk, dv written: 9 x 4 HC n; a, ds 16 H nE; graph and
            transposed graph 8 n + 8 nE + 8 n + 8 nE) and the four Linear
            backwards (4 x (4 HC n + 28 n) read)
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
REPS = int(os.environ.get("ENV_CONV_BWD_REPS", 20))
ROUNDS = int(os.environ.get("ENV_CONV_BWD_ROUNDS", 3))
PATHS = os.environ.get("ENV_CONV_BWD_PATHS", "fused,composed,torch").split(",")
CASES = os.environ.get("ENV_CONV_BWD_CASES", "24x8192:reset,24x8192:crowd,3x4096:reset,3x4096:crowd").split(",")


def timed(fn, reps):
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
    conv = gnn.TransformerConv(7, C, heads=heads, kernel_backward=True).to(DEV)
    params = list(conv.parameters())
    go = torch.randn(B, E, HC, device=DEV)
    x = out["node_feat"].reshape(n, 7)
    ea = out["edge_attr"].reshape(-1, 1)
    col = out["edge_index"][1].contiguous()
    tr = gnn.csr_transpose(gnn.env_csr(out["edge_index"], n), col)

    def grads(y):
        return torch.autograd.grad(y, params, go)

    def fused():
        w, w_e = gnn.pack_conv_params(conv)
        y, _ = gnn.env_conv_autograd(out["node_feat"], out["edge_ptr"], out["edge_index"], out["edge_attr"], w, w_e,
                                     heads, E, True, check=False)
        return grads(y)

    def composed():
        ptr = gnn.env_csr(out["edge_index"], n)
        return grads(conv(x, ptr, col, ea, transpose=tr).view(B, E, HC))

    def torch_path():
        w, w_e = gnn.pack_conv_params(conv)
        return grads(gnn.env_conv_ref(out["node_feat"], out["edge_ptr"], out["edge_index"], out["edge_attr"], w, w_e,
                                      heads, E, True))

    fns = {"fused": fused, "composed": composed, "torch": torch_path}
    # the torch path runs for tens of ms at the large shapes: fewer calls of it
    reps = {"fused": REPS, "composed": REPS, "torch": max(2, REPS // 5)}
    ms = {k: [] for k in PATHS}
    for k in PATHS:                                          # warm-up: allocator, hipBLASLt heuristics
        for _ in range(3):
            fns[k]()
    for _ in range(ROUNDS):
        for k in PATHS:
            ms[k].append(timed(fns[k], reps[k]))
    env.close()
    H = heads
    graph = 28 * n + 12 * nE + 8 * (B + 1)
    b_fused = (graph + 4 * HC * n + 4 * H * n) + (graph + 4 * nE + 8 * HC * n + 4 * H * n + 16 * H * nE)
    b_comp_f = 4 * nE + 16 * n + 4 * (28 * n + 4 * HC * n) + 5 * 4 * HC * n + 8 * n + 8 * nE + 4 * H * n
    b_comp_b = 9 * 4 * HC * n + 16 * H * nE + 16 * n + 16 * nE + 4 * (4 * HC * n + 28 * n)
    res = {
        "op": "TransformerConv(7, C, heads) on the env-form graph, forward + backward (parameter gradients)",
        "shape": f"{N} agents x {B} envs", "layout": layout, "nodes": n, "entries": nE, "mean_row": round(nE / n, 2),
        "heads": heads, "channels": C, "fused_bytes": b_fused, "composed_bytes": b_comp_f + b_comp_b,
    }
    for k in PATHS:
        best = min(ms[k])
        res[f"{k}_ms_rounds"] = [round(t, 4) for t in ms[k]]
        res[f"{k}_ms"] = round(best, 4)
    if "fused" in ms and "composed" in ms:
        res["speedup_vs_composed"] = round(min(ms["composed"]) / min(ms["fused"]), 2)
        res["fused_TBs"] = round(b_fused / (min(ms["fused"]) * 1e-3) / 1e12, 3)
        res["composed_TBs"] = round((b_comp_f + b_comp_b) / (min(ms["composed"]) * 1e-3) / 1e12, 3)
    if "fused" in ms and "torch" in ms:
        res["speedup_vs_torch"] = round(min(ms["torch"]) / min(ms["fused"]), 2)
    res["timing"] = (f"torch.cuda events around {REPS} calls ({max(2, REPS // 5)} of the torch path) after 3 warm-up "
                     f"calls, {ROUNDS} rounds alternating the paths in one process on one stream; *_ms is the best "
                     "round, every round is listed; allocations (outputs, workspace) included, no status read")
    return res


lines = []
for spec in CASES:
    shape, layout = spec.split(":")
    N, B = (int(v) for v in shape.split("x"))
    lines.append(json.dumps(case(N, B, layout)))
    print(lines[-1], flush=True)
dst = Path(os.environ.get("ENV_CONV_BWD_OUT") or ROOT / "profiles" / "env_conv_backward.json")
dst.parent.mkdir(parents=True, exist_ok=True)
dst.write_text("\n".join(lines) + "\n")
