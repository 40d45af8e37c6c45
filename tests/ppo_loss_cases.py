"""Synthetic inputs of the PPO loss tests (test_ppo_loss_ref.py on the CPU,
test_gpu_ppo_loss.py on the GPU). Helpers only. A case is drawn once, in fp32
on the CPU, from its own seed; the spreads are chosen so that every case has
rows on both sides of every branch of the loss: ``logp - logp_old`` ~ 0.25
randn puts roughly four rows in ten outside the clip range, ``v - v_old`` ~
0.2 randn roughly three value rows in ten past the value clip.
test_ppo_loss_ref.py holds every case to the share conditions."""
import functools

import torch

import train_chain as tc
from gsmarl_amd import loss as L

LAM = tc.COST_MULT
COEF = dict(clip=tc.CLIP, value_clip=tc.VCLIP, ent_coef=tc.ENT_COEF, value_coef=1.0)
# the capped grid of gsm_ppo_loss as built: 256 workgroups of 256 threads, four rows a thread
MAX_BLOCKS, THREADS, ROWS_PER_THREAD = 256, 256, 4
# rows of the case past one pass of the capped grid: every workgroup takes a second item (2 * 256 - 1 full
# rounds of 256 threads and two more items), so all 256 partials are written and every workgroup loops
B_CAPPED = ((2 * MAX_BLOCKS - 1) * THREADS + 2) * ROWS_PER_THREAD // 3

CASES = {
    "r3": dict(B=1, N=3),                                   # one item, the scalar path (R % 4 != 0)
    "r12": dict(B=4, N=3),                                  # three items, 16-byte loads
    "r765": dict(B=255, N=3),                               # around the workgroup edge of 256 * 4 rows: scalar,
    "r768": dict(B=256, N=3),                               # 16-byte loads,
    "r771": dict(B=257, N=3),                               # scalar
    "r1023": dict(B=341, N=3),                              # one short of a full workgroup
    "r1026": dict(B=342, N=3),                              # a second workgroup of one item
    "capped": dict(B=B_CAPPED, N=3),                        # past one pass of the capped grid
    "ragged24": dict(B=37, N=24, ragged=True),              # n_valid, weights in {0, 0.5, 1}, NaN in masked rows
    "nout1": dict(B=100, N=3, n_out=1),
}
# one seed per case; test_ppo_loss_ref.py holds each to the share conditions (of three or twelve rows not
# every draw has a row outside the clip range, a clipped value row in both heads and no undecided row)
SEEDS = dict({name: 100 + i for i, name in enumerate(CASES)}, r3=151, r12=150)
TENSORS = ("logp", "ent", "values", "logp_old", "adv", "v_old", "ret")


@functools.lru_cache(maxsize=None)
def inputs(case):
    """The fp32 CPU inputs of a case: the seven tensors and, for a ragged
    case, ``n_valid`` [B] (0 and N among the counts), ``weight`` [B, N] in {0,
    0.5, 1} and NaN in every input wherever the row is masked (in ``weight``
    only past ``n_valid``). Drawn once and left unchanged."""
    spec = CASES[case]
    B, N, n_out = spec["B"], spec["N"], spec.get("n_out", 2)
    g = torch.Generator().manual_seed(SEEDS[case])
    rn = lambda *s: torch.randn(*s, generator=g)
    logp_old = -(0.1 + 2.0 * torch.rand(B, N, generator=g))
    logp = logp_old + 0.25 * rn(B, N)
    ent = 1.6 * torch.rand(B, N, generator=g)
    v_old = rn(n_out, B, N)
    values = v_old + 0.2 * rn(n_out, B, N)
    ret = v_old + rn(n_out, B, N)
    adv = rn(n_out, B, N)
    d = dict(logp=logp, ent=ent, values=values, logp_old=logp_old, adv=adv, v_old=v_old, ret=ret, n_valid=None,
             weight=None)
    if spec.get("ragged"):
        n_valid = torch.randint(0, N + 1, (B,), generator=g, dtype=torch.int32)
        n_valid[0], n_valid[1] = 0, N
        weight = torch.randint(0, 3, (B, N), generator=g).to(torch.float32) * 0.5
        valid = torch.arange(N)[None, :] < n_valid[:, None]
        off = ~(valid & (weight > 0))
        nan = torch.tensor(float("nan"))
        for k in ("logp", "ent", "logp_old"):
            d[k] = torch.where(off, nan, d[k])
        for k in ("values", "adv", "v_old", "ret"):
            d[k] = torch.where(off[None], nan, d[k])
        d.update(n_valid=n_valid, weight=torch.where(valid, weight, nan))
    return d


def ref64(d, weight, keep=None, lam=LAM):
    """The fp64 restatement on the fp32 inputs ``d`` with ``weight``: ``(loss, stats)``."""
    t = [d[k].double() for k in TENSORS]
    return L.ppo_loss_ref(*t, weight.double() if weight is not None else None, d["n_valid"],
                          lam if t[2].shape[0] == 2 else None, keep=keep, **COEF)


def decide(d):
    """``(weight [B, N] fp64, share of undecided rows, share of weighted rows
    with the ratio outside the clip range, clipped value rows per head)`` from
    the fp64 restatement alone: the case's own weight without the rows within
    ``train_chain.EDGE`` of a branch point (``train_chain.undecided``)."""
    keep = {}
    ref64(d, d["weight"], keep)
    w0 = keep["w"]
    on = w0 > 0
    z = torch.zeros((), dtype=torch.float64)
    data = dict(v_old=torch.where(on[None], d["v_old"].double(), z), ret=torch.where(on[None], d["ret"].double(), z))
    und = tc.undecided(dict(ratio=keep["ratio"], v=keep["v"]), data) & on
    weight = w0 * (~und).to(w0.dtype)
    live = weight > 0
    r = keep["ratio"]
    outside = ((r < 1.0 - tc.CLIP) | (r > 1.0 + tc.CLIP)) & live
    clipped = ((keep["v"] - data["v_old"]).abs() > tc.VCLIP) & live[None]
    n = max(int(on.sum()), 1)
    return weight, float(und.sum()) / n, float(outside.sum()) / max(int(live.sum()), 1), clipped.sum((1, 2)).tolist()
