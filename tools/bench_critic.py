"""Measure the fused critic head (gsmarl_amd.policy.CriticHead: gsm_critic_eval,
gsm_critic_eval_bwd) against the composed torch critic it replaces, in one
process on one GPU.

At R = 24 x 8192 and 3 x 4096 rows, 48 features, hidden 64, 2 heads
  forward           fused CriticHead.forward with denorm under no_grad against
                    mean over agents, expand, cat, Linear, ReLU, Linear,
                    denormalise, head-major copy under no_grad
  forward_backward  CriticHead(kernel_backward=True).forward + backward against
                    autograd of the same composition, gradients for the
                    parameters and x
three alternating repeats each (fused, composed, fused, ...), torch.cuda events
around REPS calls after 3 warm-up calls. Before timing, the two forms' values
and gradients are compared at the timed size. One JSON line per shape, written
to profiles/critic_head.json (or $CRITIC_OUT).

Algorithmic bytes of forward: R rows x (4 in_features read + 4 n_out written);
the weights (25.6 KB) are not counted."""
import json
import os
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "gs-marl_amd"))
import torch  # noqa: E402

from gsmarl_amd import CriticHead  # noqa: E402

DEV = "cuda:0"
F, HID, O = 48, 64, 2
REPS = int(os.environ.get("CRITIC_REPS", 200))
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


def composed_values(head, x, denorm=None):
    """The critic as a user would chain it in torch."""
    B, N, _ = x.shape
    pool = x.mean(1, keepdim=True).expand(B, N, F)
    v = head.lin2(torch.relu(head.lin1(torch.cat([pool, x], -1))))
    if denorm is not None:
        v = v * denorm[:, 1] + denorm[:, 0]
    return v.permute(2, 0, 1).contiguous()


def case(N, B):
    torch.manual_seed(0)
    head = CriticHead(F, HID, O, kernel_backward=True).to(DEV)
    x = torch.randn(B, N, F, device=DEV)
    denorm = torch.tensor([[0.5, 3.0], [-2.0, 0.25]], device=DEV)
    g = torch.randn(O, B, N, device=DEV)
    xg = x.clone().requires_grad_()
    R = B * N

    def fused_fwd():
        with torch.no_grad():
            return head(x, denorm=denorm)

    def composed_fwd():
        with torch.no_grad():
            return composed_values(head, x, denorm)

    def backward_of(v):
        for p in head.parameters():
            p.grad = None
        xg.grad = None
        v.backward(g)

    def fused_train():
        backward_of(head(xg))

    def composed_train():
        backward_of(composed_values(head, xg))

    # the same results first (fp32 against fp32: reordered sums only)
    diff = {"values": float((fused_fwd() - composed_fwd()).abs().max())}
    fused_train()
    got = [p.grad.clone() for p in head.parameters()] + [xg.grad.clone()]
    composed_train()
    want = [p.grad for p in head.parameters()] + [xg.grad]
    for name, a, b in zip(("dw1", "db1", "dw2", "db2", "dx"), got, want):
        diff[name] = float(((a - b).abs() / (1 + b.abs())).max())
    assert diff["values"] <= 1e-4 and max(diff.values()) <= 1e-3, diff

    fwd = summary(*alternate(fused_fwd, composed_fwd, REPS))
    train = summary(*alternate(fused_train, composed_train, max(REPS // 4, 10)))
    nbytes = R * 4 * (F + O)
    return {"op": "CriticHead (gsm_critic_eval / gsm_critic_eval + gsm_critic_eval_bwd)",
            "shape": f"{N} agents x {B} envs", "rows": R, "in_features": F, "hidden": HID, "n_out": O,
            "forward": fwd, "forward_backward": train, "fused_vs_composed_max_diff": diff, "forward_bytes": nbytes,
            "forward_fused_TBs": round(nbytes / (fwd["fused_median_us"] * 1e-6) / 1e12, 3),
            "forward_fused_TFLOPs": round(2 * (R * (F * HID + HID * O) + B * F * HID) /
                                          (fwd["fused_median_us"] * 1e-6) / 1e12, 2),
            "timing": f"torch.cuda events around {REPS} calls (forward_backward: {max(REPS // 4, 10)}) after 3 "
                      "warm-up calls, three alternating repeats, one stream, one process; output allocations "
                      "included"}


if __name__ == "__main__":
    lines = []
    for N, B in SHAPES:
        lines.append(json.dumps(case(N, B)))
        print(lines[-1], flush=True)
    dst = Path(os.environ.get("CRITIC_OUT") or ROOT / "profiles" / "critic_head.json")
    dst.parent.mkdir(parents=True, exist_ok=True)
    dst.write_text("\n".join(lines) + "\n")
