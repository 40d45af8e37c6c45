"""Bit-level A/B of two builds of libgsm.so on the heads and GNN entry points.

Runs a fixed, seeded list of calls through the library ``GSM_LIB_PATH`` names
(the product library without it) and prints one JSON object
``{case: {output: sha256 of its bytes}}``. Run it once per library, in separate
processes; a refactor leaves the two objects equal key for key:

    GSM_LIB_PATH=.../lib/ablate/parent.so python tools/ab_bits.py > a.json
    python tools/ab_bits.py > b.json

The shapes are the smallest that reach every path of the actor and critic
heads (partial tiles, a second tile, the grid caps, strided rows), of the
attention aggregation and of the fused first layer (both lane widths, more
than 128 partials, the recompute form). Needs a GPU.
"""
from __future__ import annotations

import hashlib
import itertools
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "gs-marl_amd"))
from gsmarl_amd import _lib, gnn  # noqa: E402

DEV = torch.device("cuda:0")
F32 = dict(dtype=torch.float32, device=DEV)
OUT = {}
P, S = _lib.ptr, _lib.stream


def sha(t):
    return None if t is None else hashlib.sha256(t.detach().contiguous().cpu().numpy().tobytes()).hexdigest()


def record(case, **outs):
    assert case not in OUT, case
    OUT[case] = {k: sha(v) for k, v in outs.items()}


def rand(gen, *shape, scale=1.0):
    return (torch.randn(*shape, generator=gen) * scale).to(DEV)


def mlp_weights(gen, cols, hidden, n_out):
    kw = hidden if hidden else cols
    w1 = rand(gen, hidden, cols, scale=0.3) if hidden else None
    b1 = rand(gen, hidden, scale=0.3) if hidden else None
    return w1, b1, rand(gen, n_out, kw, scale=0.3), rand(gen, n_out, scale=0.3)


def call(name, *args):
    lib = _lib.load()
    _lib.check(lib, getattr(lib, name)(*args), None, name)


# ------------------------------------------------------------------ actor
def actor_sample(x, stride, w, B, N, F, H, A, det, counter, want):
    acts = torch.empty(B, N, dtype=torch.int32, device=DEV)
    logp = torch.empty(B, N, **F32)
    ent = torch.empty(B, N, **F32) if want else None
    lout = torch.empty(B, N, A, **F32) if want else None
    st = torch.zeros(1, dtype=torch.int32, device=DEV)
    call("gsm_actor_sample", P(x), stride, *map(P, w), B, N, F, H, A, 1234567, 5, 3, P(counter),
         _lib.ACTOR_DETERMINISTIC if det else 0, P(acts), P(logp), P(ent), P(lout), P(st), S(DEV))
    return dict(actions=acts, logp=logp, entropy=ent, logits=lout, status=st)


def actor_eval(x, stride, w, B, N, F, H, A, acts):
    logp, ent = torch.empty(B, N, **F32), torch.empty(B, N, **F32)
    st = torch.zeros(1, dtype=torch.int32, device=DEV)
    call("gsm_actor_eval", P(x), stride, *map(P, w), B, N, F, H, A, P(acts), P(logp), P(ent), P(st), S(DEV))
    return dict(logp=logp, entropy=ent, status=st)


def actor_bwd(x, stride, w, B, N, F, H, A, acts, g_logp, g_ent, want_dx):
    work = torch.empty(_lib.work_floats("gsm_actor_backward_work_floats", F, H, A), **F32)
    d = [torch.empty_like(t) if t is not None else None for t in w]
    dx = torch.empty(B, N, F, **F32) if want_dx else None
    st = torch.zeros(1, dtype=torch.int32, device=DEV)
    call("gsm_actor_eval_bwd", P(g_logp), P(g_ent), P(x), stride, *map(P, w), B, N, F, H, A, P(acts), P(work),
         *map(P, d), P(dx), P(st), S(DEV))
    return dict(dw1=d[0], db1=d[1], dw2=d[2], db2=d[3], dx=dx, status=st)


def actor_cases():
    counter = torch.tensor([7], dtype=torch.int64, device=DEV)
    for (F, H, A), (B, N) in itertools.product([(4, 0, 2), (48, 16, 5), (52, 32, 5), (128, 64, 8)], [(7, 3), (43, 3)]):
        gen = torch.Generator().manual_seed(1000 + F + B)
        tag = f"actor/{F}-{H}-{A}/{B}x{N}"
        w, x = mlp_weights(gen, F, H, A), rand(gen, B, N, F)
        s = actor_sample(x, F, w, B, N, F, H, A, False, counter, False)
        record(tag + "/sample", **s)
        record(tag + "/deterministic", **actor_sample(x, F, w, B, N, F, H, A, True, None, True))
        record(tag + "/eval", **actor_eval(x, F, w, B, N, F, H, A, s["actions"]))
        gl, ge = rand(gen, B, N), rand(gen, B, N)
        for ent, dx in itertools.product((True, False), (True, False)):
            record(f"{tag}/bwd/ent{int(ent)}-dx{int(dx)}",
                   **actor_bwd(x, F, w, B, N, F, H, A, s["actions"], gl, ge if ent else None, dx))
    # x a slice of wider rows: the row stride is greater than in_features
    gen = torch.Generator().manual_seed(11)
    F, H, A, B, N = 48, 16, 5, 43, 3
    w, wide = mlp_weights(gen, F, H, A), rand(gen, B, N, F + 16)
    x = wide[..., 8:8 + F]
    assert x.data_ptr() % 16 == 0
    s = actor_sample(x, F + 16, w, B, N, F, H, A, False, None, True)
    record("actor/strided/sample", **s)
    record("actor/strided/bwd", **actor_bwd(x, F + 16, w, B, N, F, H, A, s["actions"], rand(gen, B, N),
                                            rand(gen, B, N), True))
    # past the grid caps: a workgroup takes a second tile
    F, H, A, N = 52, 32, 5, 24
    w = mlp_weights(gen, F, H, A)
    for B, bwd in ((2731, True), (10923, False)):
        x = rand(gen, B, N, F)
        s = actor_sample(x, F, w, B, N, F, H, A, False, None, True)
        record(f"actor/capped/{B}x{N}/sample", **s)
        if bwd:
            record(f"actor/capped/{B}x{N}/bwd", **actor_bwd(x, F, w, B, N, F, H, A, s["actions"], rand(gen, B, N),
                                                            rand(gen, B, N), True))


# ------------------------------------------------------------------ critic
def critic_eval(x, w, n_valid, denorm, B, N, F, H, O):
    values = torch.empty(O, B, N, **F32)
    st = torch.zeros(1, dtype=torch.int32, device=DEV)
    call("gsm_critic_eval", P(x), F, P(n_valid), *map(P, w), P(denorm), B, N, F, H, O, P(values), P(st), S(DEV))
    return dict(values=values, status=st)


def critic_bwd(g, x, w, n_valid, B, N, F, H, O, want_dx):
    work = torch.empty(_lib.work_floats("gsm_critic_backward_work_floats", F, H, O), **F32)
    d = [torch.empty_like(t) for t in w]
    dx = torch.empty(B, N, F, **F32) if want_dx else None
    st = torch.zeros(1, dtype=torch.int32, device=DEV)
    call("gsm_critic_eval_bwd", P(g), P(x), F, P(n_valid), *map(P, w), B, N, F, H, O, P(work), *map(P, d), P(dx),
         P(st), S(DEV))
    return dict(dw1=d[0], db1=d[1], dw2=d[2], db2=d[3], dx=dx, status=st)


def critic_cases():
    shapes = [(7, 3), (5, 96), (3, 128), (300, 1)]
    for (F, H, O), (B, N) in itertools.product([(4, 16, 1), (52, 32, 2), (64, 64, 2)], shapes + [(2561, 24)]):
        big = B == 2561
        if big and H != 32:
            continue
        gen = torch.Generator().manual_seed(2000 + F + B)
        tag = f"critic/{F}-{H}-{O}/{B}x{N}"
        w, x, g = mlp_weights(gen, 2 * F, H, O), rand(gen, B, N, F), rand(gen, O, B, N)
        nv = torch.randint(0, N + 1, (B,), generator=gen).to(torch.int32)
        nv[0], nv[-1] = 0, N
        denorm = rand(gen, 2 * O).abs() + 0.5
        for name, n_valid in (("all", None), ("ragged", nv.to(DEV))):
            if not big:
                record(f"{tag}/{name}/eval", **critic_eval(x, w, n_valid, None, B, N, F, H, O))
                record(f"{tag}/{name}/eval-denorm", **critic_eval(x, w, n_valid, denorm, B, N, F, H, O))
                record(f"{tag}/{name}/bwd", **critic_bwd(g, x, w, n_valid, B, N, F, H, O, False))
            record(f"{tag}/{name}/bwd-dx", **critic_bwd(g, x, w, n_valid, B, N, F, H, O, True))


# ------------------------------------------------------------------ attention
def symmetric_graph(rng, n, deg=4):
    """A random symmetric graph as CSR with ascending columns: (row_ptr int64 [n+1], col int32)."""
    a = rng.integers(0, n, n * deg // 2)
    b = rng.integers(0, n, n * deg // 2)
    keep = a != b
    pairs = np.unique(np.concatenate([np.stack([a[keep], b[keep]], 1), np.stack([b[keep], a[keep]], 1)]), axis=0)
    ptr = np.zeros(n + 1, np.int64)
    np.cumsum(np.bincount(pairs[:, 0], minlength=n), out=ptr[1:])
    return torch.from_numpy(ptr).to(DEV), torch.from_numpy(pairs[:, 1].astype(np.int32)).to(DEV)


def attention_cases():
    for (heads, C), n in itertools.product([(3, 16), (3, 1)], (2100, 10)):
        rng = np.random.default_rng(3000 + n + C)
        gen = torch.Generator().manual_seed(3000 + n + C)
        HC = heads * C
        ptr, col = symmetric_graph(rng, n)
        q, k, v, skip, go = (rand(gen, n, HC) for _ in range(5))
        ew, we = rand(gen, col.numel()).abs(), rand(gen, HC)
        for edge in (True, False):
            tag = f"attn/{heads}x{C}/n{n}/edge{int(edge)}"
            e = dict(edge_w=ew, w_e=we) if edge else {}
            record(tag + "/fwd", out=gnn.attn_aggregate(q, k, v, ptr, col, skip=skip, heads=heads, **e))
            leaves = [t.clone().requires_grad_(True) for t in ((q, k, v, skip) + ((ew, we) if edge else ()))]
            ee = dict(edge_w=leaves[4], w_e=leaves[5]) if edge else {}
            out = gnn.attn_aggregate_autograd(*leaves[:3], ptr, col, skip=leaves[3], heads=heads, **ee)
            out.backward(go)
            names = ("dq", "dk", "dv", "dskip", "dedge_w", "dw_e")
            record(tag + "/fwd-bwd", out=out, **{m: t.grad for m, t in zip(names, leaves)})


# ------------------------------------------------------------------ fused first layer
def env_graph(rng, B, E, deg=4):
    """B symmetric env graphs of E entities in env form: (node_feat, edge_ptr, edge_index, edge_attr)."""
    rows, cols, ptr = [], [], [0]
    for b in range(B):
        a, c = rng.integers(0, E, E * deg // 2), rng.integers(0, E, E * deg // 2)
        keep = a != c
        pairs = np.unique(np.concatenate([np.stack([a[keep], c[keep]], 1), np.stack([c[keep], a[keep]], 1)]), axis=0)
        rows.append(pairs[:, 0] + b * E)
        cols.append(pairs[:, 1] + b * E)
        ptr.append(ptr[-1] + len(pairs))
    ei = torch.from_numpy(np.stack([np.concatenate(rows), np.concatenate(cols)]).astype(np.int32)).to(DEV)
    attr = torch.from_numpy(rng.random(ei.shape[1]).astype(np.float32)).to(DEV)
    feat = torch.from_numpy(rng.standard_normal((B, E, 7)).astype(np.float32)).to(DEV)
    return feat, torch.tensor(ptr, dtype=torch.int64, device=DEV), ei, attr


def env_conv_cases():
    # (entities, heads, channels, rows_out, envs): 288 entities take the recompute form
    shapes = [(27, 3, 16, 27, 300), (27, 3, 16, 5, 3), (6, 3, 1, 6, 300), (6, 3, 1, 3, 3), (288, 3, 8, 288, 2)]
    for (E, heads, C, R, B), skip, edge in itertools.product(shapes, (True, False), (True, False)):
        rng = np.random.default_rng(4000 + E + B)
        gen = torch.Generator().manual_seed(4000 + E + B)
        HC = heads * C
        feat, ptr, ei, attr = env_graph(rng, B, E)
        w, w_e, go = rand(gen, 4 if skip else 3, HC, 8, scale=0.5), (rand(gen, HC) if edge else None), rand(gen, B, R, HC)
        tag = f"env_conv/E{E}-{heads}x{C}-R{R}/B{B}/skip{int(skip)}-edge{int(edge)}"
        out, rp = gnn.env_conv(feat, ptr, ei, attr, w, w_e, heads, R, skip, row_ptr=True)
        record(tag + "/fwd", out=out, row_ptr=rp)
        wl = w.clone().requires_grad_(True)
        wel = w_e.clone().requires_grad_(True) if edge else None
        out = gnn.env_conv_autograd(feat, ptr, ei, attr, wl, wel, heads, R, skip)
        out.backward(go)
        record(tag + "/fwd-bwd", out=out, dw=wl.grad, dw_e=wel.grad if edge else None)


if __name__ == "__main__":
    actor_cases()
    critic_cases()
    attention_cases()
    env_conv_cases()
    torch.cuda.synchronize()
    print(f"library: {_lib.LIB_PATH}", file=sys.stderr)
    print(json.dumps(OUT, sort_keys=True))
