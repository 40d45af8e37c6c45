"""Measure the fused PPO / Lagrangian loss (gsmarl_amd.loss.PPOLagrangianLoss:
gsm_ppo_loss, two launches, the backward a multiplication) against the torch
restatement under autograd (gsmarl_amd.loss.ppo_loss_ref, the loss as a user
would write it), in one process on one GPU.

At R = 24 x 8192 and 3 x 4096 rows, two heads, with a weight
  forward_backward  loss = f(logp, ent, values, ...); loss.backward(), with
                    gradients for logp, ent and values
  forward           the same loss under no_grad
three alternating repeats each (fused, composed, fused, ...), torch.cuda events
around REPS calls after 3 warm-up calls. Before timing, the two forms' loss,
statistics and gradients are compared at the timed size. One JSON line per
shape, written to profiles/ppo_loss.json (or $PPO_LOSS_OUT).

Algorithmic bytes of forward_backward: R rows x 4 B x (3 + 4 n_out + 1 read, 2 +
n_out written and, scaled in place, read and written once more)."""
import json
import os
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "gs-marl_amd"))
import torch  # noqa: E402

from gsmarl_amd import LagrangeMultiplier, PPOLagrangianLoss  # noqa: E402
from gsmarl_amd.loss import ppo_loss_ref  # noqa: E402

DEV = "cuda:0"
O = 2
REPS = int(os.environ.get("PPO_LOSS_REPS", 1000))
SHAPES = ((24, 8192), (3, 4096))
COEF = dict(clip=0.2, value_clip=0.2, ent_coef=0.01, value_coef=1.0)


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
    g = torch.Generator(device=DEV).manual_seed(0)
    rn = lambda *s: torch.randn(*s, device=DEV, generator=g)
    logp_old = -(0.1 + 2.0 * torch.rand(B, N, device=DEV, generator=g))
    logp = (logp_old + 0.25 * rn(B, N)).requires_grad_()
    ent = (1.6 * torch.rand(B, N, device=DEV, generator=g)).requires_grad_()
    v_old = rn(O, B, N)
    values = (v_old + 0.2 * rn(O, B, N)).requires_grad_()
    ret, adv = v_old + rn(O, B, N), rn(O, B, N)
    weight = (torch.rand(B, N, device=DEV, generator=g) < 0.9).float()
    lam = LagrangeMultiplier(0.5, lr=0.05, cost_limit=1.0).to(DEV)
    fused_mod = PPOLagrangianLoss(COEF["clip"], COEF["value_clip"], COEF["ent_coef"], COEF["value_coef"])
    leaves = (logp, ent, values)
    rest = (logp_old, adv, v_old, ret, weight, None, lam.lam)
    R = B * N

    def fused_loss():
        return fused_mod(*leaves, *rest)

    def composed_loss():
        return ppo_loss_ref(*leaves, *rest, **COEF)[0]

    def train(loss_fn):
        def run():
            for x in leaves:
                x.grad = None
            loss_fn().backward()
        return run

    def fwd(loss_fn):
        def run():
            with torch.no_grad():
                return loss_fn()
        return run

    # the same results first (fp32 against fp32: reordered sums and torch's exp only)
    train(fused_loss)()
    got = [x.grad.clone() for x in leaves]
    stats = fused_mod.stats.clone()
    train(composed_loss)()
    want = [x.grad for x in leaves]
    W = float(stats[7])
    diff = {"loss": abs(float(fwd(fused_loss)()) - float(fwd(composed_loss)())),
            "stats": float((stats - ppo_loss_ref(*(x.detach() for x in leaves), *rest, **COEF)[1]).abs()[:7].max())}
    flips = 0
    for name, a, b in zip(("g_logp", "g_ent", "g_values"), got, want):
        flipped = (a == 0) != (b == 0)          # a row on a branch point that the two fp32 forms decide differently
        flips += int(flipped.sum())
        err = (a - b).abs() * W / (1 + b.abs() * W)                             # per row, in units of w_r / W
        diff[name] = float(torch.where(flipped, torch.zeros_like(err), err).max())
    assert int(fused_mod.status.item()) == 0 and max(diff.values()) <= 1e-4 and flips <= 3, (diff, flips)
    diff["rows_decided_differently"] = flips

    train_t = summary(*alternate(train(fused_loss), train(composed_loss), REPS))
    fwd_t = summary(*alternate(fwd(fused_loss), fwd(composed_loss), REPS))
    nbytes = R * 4 * ((3 + 4 * O + 1) + 3 * (2 + O))
    return {"op": "PPOLagrangianLoss (gsm_ppo_loss) against ppo_loss_ref under autograd",
            "shape": f"{N} agents x {B} envs", "rows": R, "n_out": O, "forward_backward": train_t, "forward": fwd_t,
            "fused_vs_composed_max_diff": diff, "forward_backward_bytes": nbytes,
            "forward_backward_fused_TBs": round(nbytes / (train_t["fused_median_us"] * 1e-6) / 1e12, 3),
            "timing": f"torch.cuda events around {REPS} calls after 3 warm-up calls, three alternating repeats, "
                      "one stream, one process; output allocations, the status word's fill and autograd's "
                      "bookkeeping included"}


if __name__ == "__main__":
    lines = []
    for N, B in SHAPES:
        lines.append(json.dumps(case(N, B)))
        print(lines[-1], flush=True)
    dst = Path(os.environ.get("PPO_LOSS_OUT") or ROOT / "profiles" / "ppo_loss.json")
    dst.parent.mkdir(parents=True, exist_ok=True)
    dst.write_text("\n".join(lines) + "\n")
