"""Cases of the optimizer step (gsm_adam_step, gsmarl_amd.optim) for
test_optim_ref.py (CPU) and test_gpu_optim.py / test_gpu_guard_optim.py (GPU),
and the error scales both hold a result to. Helpers only.

A case is a list of tensors with gradients, moments, a step count and the
hyper-parameters, drawn on the CPU from the case's seed. The sizes are the
edges of the kernel's mapping (an item of 4 elements, a wave of 64 items, a
chunk of 1024 elements) and the chain's real shapes (6144 = 64 x 96, 336 = 48
x 7, 2304 = 48 x 48); LOOP is a tensor of more chunks than the grid cap, so
every workgroup loops; MANY has more tensors than one launch's table."""
import math

import torch

from gsmarl_amd.optim import clipped_adam_ref

CHUNK, CAP, TABLE = 1024, 1024, 32           # kOptChunk, kOptMaxBlocks (gsm_adam.hip), kOptTable (gsm_internal.h)
SIZES = [1, 5, 63, 64, 65, 255, 256, 257, 1023, 1025, 6144, 336, 2304]
LOOP = CHUNK * CAP + 1025                    # 1026 chunks
MANY = [SIZES[i % len(SIZES)] for i in range(TABLE + 8)]
MANY[5] = 0                                  # a tensor of no elements is legal and skipped
LR, BETAS, EPS = 7e-4, (0.9, 0.999), 1e-5
U = 2.0 ** -24

# name: sizes, gradient scale, step count before the call, warmed moments, max_norm, what the case must show
CASES = {
    "clipped":   dict(sizes=SIZES, scale=1.0, t=0, warm=False, max_norm=0.5, want="clip"),
    "unclipped": dict(sizes=SIZES, scale=1e-2, t=1, warm=True, max_norm=10.0, want="one"),
    "noclip":    dict(sizes=SIZES, scale=1e2, t=9, warm=True, max_norm=None, want="one"),
    "t999":      dict(sizes=SIZES, scale=1e-1, t=999, warm=True, max_norm=0.5, want="clip"),
    "t9999":     dict(sizes=SIZES, scale=1e1, t=9999, warm=True, max_norm=10.0, want="clip"),
    "zero":      dict(sizes=SIZES, scale=0.0, t=0, warm=False, max_norm=10.0, want="zero"),
    "nan":       dict(sizes=SIZES, scale=1.0, t=9, warm=True, max_norm=10.0, want="skip", poison=float("nan")),
    "inf":       dict(sizes=SIZES, scale=1.0, t=9, warm=True, max_norm=None, want="skip", poison=float("inf")),
    "huge":      dict(sizes=SIZES[:8], scale=1e20, t=1, warm=True, max_norm=10.0, want="clip"),
    "frozen":    dict(sizes=SIZES, scale=1.0, t=1, warm=True, max_norm=0.5, want="clip", frozen=3),
    "many":      dict(sizes=MANY, scale=1e-1, t=9, warm=True, max_norm=10.0, want="clip"),
    "capped":    dict(sizes=[5, 1023, LOOP, 64], scale=1e-2, t=9, warm=True, max_norm=10.0, want="clip"),
}
SMALL = [c for c in CASES if c != "capped"]       # the cases a CPU test steps in fp64 many times
PARITY = [c for c in CASES if CASES[c]["want"] != "skip"]


def make(name, dtype=torch.float32, device="cpu"):
    """The state of case ``name`` before the call: dict(p, g, m, v: lists, an
    entry of ``g`` None for the frozen parameter; t; max_norm). Drawn in fp32
    and then cast, so every dtype starts from the same fp32 values."""
    c = CASES[name]
    gen = torch.Generator().manual_seed(1000 + list(CASES).index(name))
    rn = lambda n: torch.randn(n, generator=gen)
    p, g, m, v = [], [], [], []
    for i, n in enumerate(c["sizes"]):
        p.append(rn(n))
        if c["scale"] >= 1e20:                    # squares overflow fp32, every element (no small draw)
            g.append(c["scale"] * (1.0 + torch.rand(n, generator=gen)) * torch.sign(rn(n)))
        else:
            g.append(c["scale"] * rn(n))
        s = c["scale"] if 0 < c["scale"] < 1e20 else 1.0
        m.append(0.1 * s * rn(n) if c["warm"] else torch.zeros(n))
        v.append((0.5 * s * rn(n)) ** 2 if c["warm"] else torch.zeros(n))
    if "poison" in c:
        g[10][4097] = c["poison"]                 # one element of one gradient, in the fifth chunk of the 6144
    if "frozen" in c:
        g[c["frozen"]] = None
    cast = lambda ts: [t.to(device=device, dtype=dtype) if t is not None else None for t in ts]
    return dict(p=cast(p), g=cast(g), m=cast(m), v=cast(v), t=c["t"], max_norm=c["max_norm"])


def active(st):
    """The indices with a gradient."""
    return [i for i, g in enumerate(st["g"]) if g is not None]


def ref_step(st, dtype, lr=LR):
    """``clipped_adam_ref`` in ``dtype`` from the state ``st`` (cast from what
    it holds) over the tensors with a gradient. ``lr``: a float or a tensor.
    Returns dict(p, m, v: lists over ``active(st)``; step; stats)."""
    idx = active(st)
    to = lambda ts: [ts[i].to(dtype) for i in idx]
    p, m, v, step, stats = clipped_adam_ref(to(st["p"]), to(st["g"]), to(st["m"]), to(st["v"]), st["t"], lr, BETAS,
                                            EPS, st["max_norm"])
    return dict(p=p, m=m, v=v, step=step, stats=stats)


def _ratio(diff, scale):
    """max diff / scale; where the scale is 0 the difference has to be 0."""
    r = torch.where(scale > 0, diff / torch.where(scale > 0, scale, torch.ones_like(scale)),
                    torch.where(diff > 0, torch.full_like(diff, math.inf), torch.zeros_like(diff)))
    return float(r.max()) if r.numel() else 0.0


def ratios(st, got, lr=LR):
    """The errors of ``got`` (dict(p, m, v): lists over ``active(st)``, what an
    fp32 form made of the fp32 state ``st``) against ``clipped_adam_ref`` in
    fp64 from the same state, in units of 2^-24 times the scales

        a = |g| coef,  sm = beta1 |m| + (1 - beta1) a,  sv = beta2 v + (1 - beta2) a^2
        m: sm      v: sv      p: step_size sm / denom64, after 2^-24 |p64| is taken off

    (every term non-negative: nothing cancels). Returns (rm, rv, rp, ref64);
    the state must not be a skipped one."""
    ref = ref_step(st, torch.float64, lr)
    assert float(ref["stats"][3]) == 0.0
    idx = active(st)
    coef = ref["stats"][1]
    b1, b2 = BETAS
    t = st["t"] + 1
    lr64 = float(lr.double().reshape(-1)[0]) if torch.is_tensor(lr) else float(lr)
    step_size, bc2_sqrt = lr64 / (1.0 - b1 ** t), math.sqrt(1.0 - b2 ** t)
    rm = rv = rp = 0.0
    for k, i in enumerate(idx):
        dev = ref["p"][k].device
        a = st["g"][i].to(dev, torch.float64).abs() * coef
        sm = b1 * st["m"][i].to(dev, torch.float64).abs() + (1.0 - b1) * a
        sv = b2 * st["v"][i].to(dev, torch.float64) + (1.0 - b2) * a * a
        denom = ref["v"][k].sqrt() / bc2_sqrt + EPS
        d = lambda x, y: (x.to(dev, torch.float64) - y).abs()
        rm = max(rm, _ratio(d(got["m"][k], ref["m"][k]), U * sm))
        rv = max(rv, _ratio(d(got["v"][k], ref["v"][k]), U * sv))
        over = (d(got["p"][k], ref["p"][k]) - U * ref["p"][k].abs()).clamp(min=0.0)
        rp = max(rp, _ratio(over, U * step_size * sm / denom))
    return rm, rv, rp, ref


def pow2_above(x):
    return 2.0 ** math.ceil(math.log2(x))


# Km, Kv, Kp of the GPU tests: 4 x the largest ratio of the fp32 torch restatement on the cases above
# (test_optim_ref.py measures them and holds 4 x measured, rounded up to a power of two, to these)
KM, KV, KP = 16.0, 32.0, 32.0
