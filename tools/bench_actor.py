"""Measure the fused actor head (gsmarl_amd.policy.ActorHead: gsm_actor_sample,
gsm_actor_eval, gsm_actor_eval_bwd) against the composed torch head it
replaces, in one process on one GPU.

Default: at R = 24 x 8192 and 3 x 4096 rows, 48 features, hidden 64, 5 actions
  act       fused ActorHead.act against Linear, ReLU, Linear, log_softmax,
            exp, multinomial, gather under no_grad
  evaluate  ActorHead(kernel_backward=True).evaluate + backward against
            autograd of the torch formulation (actor_logits_ref /
            actor_dist_ref), gradients for the parameters and x
three alternating repeats each (fused, composed, fused, ...), torch.cuda events
around REPS calls after 3 warm-up calls. One JSON line per shape, written to
profiles/actor_head.json (or $ACTOR_OUT).

--loop: the closed loop of a runner's step, TransformerConv(7, 16, heads=3)
on the env-form graph (gsm_env_conv, agent rows) + act + env.step, run eagerly
and as one torch.cuda.graph whose draw counter lives on the device and is
advanced by an add_ inside the graph. Written to profiles/actor_loop.json.

Algorithmic bytes of act: R rows x (4 in_features read + 8 written: action and
logp); the weights (13.6 KB) are not counted."""
import json
import os
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "gs-marl_amd"))
import torch  # noqa: E402

from gsmarl_amd import ActorHead, EnvConfig, GpuBatchEnv, gnn, policy  # noqa: E402

DEV = "cuda:0"
F, HID, A = 48, 64, 5
REPS = int(os.environ.get("ACTOR_REPS", 200))
SHAPES = ((24, 8192), (3, 4096))


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
    return a.elapsed_time(b) / reps * 1e3          # microseconds a call


def alternate(fused, composed, reps, n=3):
    f, c = [], []
    for _ in range(n):
        f.append(round(timed(fused, reps), 1))
        c.append(round(timed(composed, reps), 1))
    return f, c


def summary(f, c):
    med = lambda v: sorted(v)[len(v) // 2]
    return {"fused_us": f, "composed_us": c, "fused_median_us": med(f), "composed_median_us": med(c),
            "speedup_of_medians": round(med(c) / med(f), 2),
            "fused_faster_beyond_spread": max(f) < min(c)}


def case(N, B):
    torch.manual_seed(0)
    head = ActorHead(F, HID, A, kernel_backward=True).to(DEV)
    x = torch.randn(B, N, F, device=DEV)
    R = B * N
    draw = [0]

    def fused_act():
        draw[0] += 1
        return head.act(x, 1, draw=draw[0])

    def composed_act():
        with torch.no_grad():
            logp_all = torch.log_softmax(head.lin2(torch.relu(head.lin1(x))), -1).view(R, A)
            a = torch.multinomial(logp_all.exp(), 1)
            return a.view(B, N), logp_all.gather(1, a).view(B, N)

    act = alternate(fused_act, composed_act, REPS)
    actions, _ = head.act(x, 1)
    g_logp, g_ent = torch.randn(B, N, device=DEV), torch.randn(B, N, device=DEV)
    xg = x.clone().requires_grad_()

    def backward_of(logp, ent):
        for p in head.parameters():
            p.grad = None
        xg.grad = None
        torch.autograd.backward((logp, ent), (g_logp, g_ent))

    def fused_eval():
        backward_of(*head.evaluate(xg, actions))

    def composed_eval():
        logp_all, ent = policy.actor_dist_ref(head.logits(xg))
        backward_of(logp_all.gather(-1, actions.long()[..., None])[..., 0], ent)

    ev = alternate(fused_eval, composed_eval, max(REPS // 4, 10))
    nbytes = R * (4 * F + 8)
    s_act = summary(*act)
    return {"op": "ActorHead (gsm_actor_sample / gsm_actor_eval + gsm_actor_eval_bwd)",
            "shape": f"{N} agents x {B} envs", "rows": R, "in_features": F, "hidden": HID, "n_actions": A,
            "act": s_act, "evaluate_backward": summary(*ev), "act_bytes": nbytes,
            "act_fused_TBs": round(nbytes / (s_act["fused_median_us"] * 1e-6) / 1e12, 3),
            "act_fused_TFLOPs": round(2 * R * (F * HID + HID * A) / (s_act["fused_median_us"] * 1e-6) / 1e12, 2),
            "timing": f"torch.cuda events around {REPS} calls (evaluate: {max(REPS // 4, 10)}) after 3 warm-up calls, "
                      "three alternating repeats, one stream, one process; output allocations included"}


def loop(N, B, steps=200):
    env = GpuBatchEnv(EnvConfig(n_agents=N, n_envs=B, seed=1), DEV)
    env.reset(seed=1, sync_edges=False)
    torch.manual_seed(0)
    conv = gnn.TransformerConv(7, 16, heads=3).to(DEV)
    head = ActorHead(F, HID, A).to(DEV)
    w, w_e = (t.detach() for t in gnn.pack_conv_params(conv))
    t = env.t
    counter = torch.zeros(1, dtype=torch.int64, device=DEV)

    def step():
        with torch.no_grad():
            feats, _ = gnn.env_conv(t["node_feat"], t["edge_ptr"], t["edge_index"], t["edge_attr"], w, w_e, 3, N, True,
                                    check=False)
            actions, _ = head.act(feats, 1, draw_counter=counter)
            counter.add_(1)
            env.step(actions, sync_edges=False)

    eager = [round(timed(step, steps), 1) for _ in range(3)]
    side = torch.cuda.Stream(device=DEV)
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step()
    torch.cuda.current_stream().wait_stream(side)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        step()
    graph = [round(timed(g.replay, steps), 1) for _ in range(3)]
    torch.cuda.synchronize()
    res = {"op": "closed loop: gsm_env_conv (agent rows) + gsm_actor_sample + counter add_ + env.step",
           "shape": f"{N} agents x {B} envs", "eager_us_per_step": eager, "graph_us_per_step": graph,
           "draws_taken": int(counter.item()),
           "timing": f"torch.cuda events around {steps} steps after 3 warm-up steps, three repeats"}
    del g
    env.close()
    return res


if __name__ == "__main__":
    run, name = (loop, "actor_loop.json") if "--loop" in sys.argv[1:] else (case, "actor_head.json")
    lines = []
    for N, B in SHAPES:
        lines.append(json.dumps(run(N, B)))
        print(lines[-1], flush=True)
    dst = Path(os.environ.get("ACTOR_OUT") or ROOT / "profiles" / name)
    dst.parent.mkdir(parents=True, exist_ok=True)
    dst.write_text("\n".join(lines) + "\n")
