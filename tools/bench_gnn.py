"""Measure gsm_attn_aggregate (the GNN message-passing kernel) on the env's
own graph at the headline size (24 agents x 8192 envs: 589,824 nodes), and
the torch formulation of the same op for comparison. One JSON line for the
forward, then one for forward + backward (gnn.attn_aggregate_autograd with the
transposed graph prebuilt and built each call, against autograd of the torch
formulation in the same process), which is also written to
profiles/gnn_backward.json (or $GNN_BWD_OUT).

Algorithmic bytes per launch: q, skip and out rows once per node (3 x 4HC),
k and v rows once per node (each row is gathered by its ~2.5 neighbours, which
sit in the same env, so one HBM read), row_ptr (8) per node, col + edge
weight (8) per edge.

Forward + backward adds: the forward's lse (4H per node); the target kernel
reads q, g, out, skip, k, v rows and lse once per node (6 x 4HC + 4H),
row_ptr (8), col + edge weight (8) per edge, and writes dq (4HC), a_ij and
ds_ij (2 x 4H per edge) and dedge_w (4 per edge); the source kernel reads
t_ptr (8) and the q, g rows once per node (2 x 4HC; gathered by the entries of
the same env), t_edge + t_tgt (8) and a_ij, ds_ij (2 x 4H) per edge, and writes
dk, dv (2 x 4HC). The dw_e partials (at most 2048 x HC) are not counted."""
import json
import os
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "gs-marl_amd"))
import torch  # noqa: E402

from gsmarl_amd import EnvConfig, GpuBatchEnv, gnn  # noqa: E402

DEV = "cuda:0"
heads, C = int(os.environ.get("GNN_HEADS", 3)), int(os.environ.get("GNN_C", 16))
B = int(os.environ.get("GNN_B", 8192))
env = GpuBatchEnv(EnvConfig(n_agents=24, n_envs=B, seed=1), DEV)
out = env.reset(seed=1)
n = env.B * env.E
ptr = gnn.env_csr(out["edge_index"], n)
col = out["edge_index"][1].contiguous()
ew = out["edge_attr"].contiguous()
nE = col.numel()
HC = heads * C
g = torch.Generator(device=DEV).manual_seed(0)
q, k, v, sk = (torch.randn(n, HC, device=DEV, generator=g) for _ in range(4))
we = torch.randn(HC, device=DEV, generator=g)


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


kern_ms = timed(lambda: gnn.attn_aggregate(q, k, v, ptr, col, ew, we, sk, heads), 100)
ref_ms = timed(lambda: gnn.attn_aggregate_ref(q, k, v, ptr, col, ew, we, sk, heads), 10)
bytes_ = n * (3 * 4 * HC + 2 * 4 * HC + 8) + nE * 8
ach = bytes_ / (kern_ms * 1e-3) / 1e9
print(json.dumps({
    "op": "gsm_attn_aggregate (TransformerConv edge softmax + aggregation)",
    "graph": f"env graph, 24 agents x {B} envs: {n} nodes, {nE} edges",
    "heads": heads, "channels": C, "kernel_us": round(kern_ms * 1e3, 2),
    "torch_formulation_us": round(ref_ms * 1e3, 1), "speedup_vs_torch": round(ref_ms / kern_ms, 1),
    "algorithmic_bytes": int(bytes_), "achieved_GBs": round(ach, 1), "frac_of_8TBs": round(ach / 8000, 4),
    "timing": "torch.cuda events around 100 launches on the current stream (the kernel's stream)",
}))

# forward + backward
gr = torch.randn(n, HC, device=DEV, generator=g)
ins = [t.clone().requires_grad_(True) for t in (q, k, v, ew, we, sk)]


def fb_kernel(transpose):
    out_ = gnn.attn_aggregate_autograd(ins[0], ins[1], ins[2], ptr, col, ins[3], ins[4], ins[5], heads,
                                       transpose=transpose)
    return torch.autograd.grad(out_, ins, gr)


def fb_torch():
    out_ = gnn.attn_aggregate_ref(ins[0], ins[1], ins[2], ptr, col, ins[3], ins[4], ins[5], heads)
    return torch.autograd.grad(out_, ins, gr)


tr = gnn.csr_transpose(ptr, col)
pre_ms = timed(lambda: fb_kernel(tr), 50)
each_ms = timed(lambda: fb_kernel(None), 20)
tr_ms = timed(lambda: gnn.csr_transpose(ptr, col), 20)
torch_ms = timed(fb_torch, 5)
H = heads
fb_bytes = n * (20 * HC + 8 + 4 * H) + nE * 8 + n * (44 * HC + 4 * H + 16) + nE * (20 + 16 * H)
fb_ach = fb_bytes / (pre_ms * 1e-3) / 1e9
line = json.dumps({
    "op": "attn_aggregate_autograd forward + backward (gsm_attn_aggregate_fwd + gsm_attn_aggregate_bwd)",
    "graph": f"env graph, 24 agents x {B} envs: {n} nodes, {nE} edges",
    "heads": heads, "channels": C,
    "kernel_fwd_bwd_prebuilt_transpose_us": round(pre_ms * 1e3, 1),
    "kernel_fwd_bwd_transpose_each_call_us": round(each_ms * 1e3, 1),
    "csr_transpose_us": round(tr_ms * 1e3, 1),
    "torch_formulation_fwd_bwd_us": round(torch_ms * 1e3, 1),
    "speedup_vs_torch_prebuilt": round(torch_ms / pre_ms, 1),
    "speedup_vs_torch_each_call": round(torch_ms / each_ms, 1),
    "algorithmic_bytes": int(fb_bytes), "achieved_GBs": round(fb_ach, 1), "frac_of_8TBs": round(fb_ach / 8000, 4),
    "timing": "torch.cuda events around 50 / 20 / 5 forward+backward calls after 3 warm-up calls, one stream; "
              "gradients of q, k, v, edge_w, w_e and skip by torch.autograd.grad (no .grad accumulation)",
})
print(line)
dst = Path(os.environ.get("GNN_BWD_OUT") or ROOT / "profiles" / "gnn_backward.json")
dst.parent.mkdir(parents=True, exist_ok=True)
dst.write_text(line + "\n")
env.close()
