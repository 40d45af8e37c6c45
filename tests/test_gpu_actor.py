"""The actor head on the GPU (gsm_actor_sample / gsm_actor_eval /
gsm_actor_eval_bwd behind gsmarl_amd.policy.ActorHead) against the fp64 torch
restatements and the Philox oracle.

Bounds: logits err / (1 + |ref|) <= 2e-5 (the bound of test_gpu_env_conv.py);
logp and entropy within 2e-5 * (1 + |ref|); weight gradients and dx within
2e-5 * (1 + sum |terms|) (the form of test_gpu_env_conv_backward.py). Actions:
every row whose u lies further than 1e-5 from every value of the fp64 CDF of
the kernel's own logits must carry exactly the reference action, and at most
0.5 % of the rows may be closer than that."""
import ctypes as C

import numpy as np
import pytest
import torch

from gsmarl_amd import ActorHead, EnvConfig, GpuBatchEnv, _lib, policy
from gsmarl_amd.gnn import TransformerConv
from oracle import philox

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BOUND = 2e-5
SEED = 0x5EED_0000_0000_0011

SHAPES = [(7, 3), (333, 6), (1366, 3), (171, 24)]
HEADS = [(4, 0, 2), (48, 64, 5), (128, 64, 8), (48, 16, 5), (52, 32, 5)]
ids_h = [f"in{f}-h{h}-a{a}" for f, h, a in HEADS]
ids_s = [f"B{b}-N{n}" for b, n in SHAPES]


def make_head(F, hidden, A, seed=0, **kw):
    torch.manual_seed(seed)
    head = ActorHead(F, hidden, A, **kw).to(DEV)
    with torch.no_grad():
        head.lin2.weight.mul_(3.0)      # logits a few units apart: a distribution that is not flat
        head.lin2.bias.uniform_(-1.0, 1.0)
    return head


def make_x(B, N, F, seed=1):
    g = torch.Generator(device=DEV).manual_seed(seed)
    if F == 52:                          # a view of wider rows: row stride 64
        return torch.randn(B, N, 64, device=DEV, generator=g)[:, :, :F]
    return torch.randn(B, N, F, device=DEV, generator=g)


def w64(head):
    return [t.detach().double() if t is not None else None for t in head._weights()]


def oracle_u(B, N, seed, env_base=0, draw=0):
    i = np.arange(N, dtype=np.uint64)[None, :]
    b = (np.arange(B, dtype=np.uint64)[:, None] + np.uint64(env_base)) & np.uint64(0xFFFFFFFF)
    x0 = philox.philox4x32_10(i, np.uint64(draw & 0xFFFFFFFF), b, 3, seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF)[0]
    return philox.u01_f32(x0)


def bits(t):
    return t.contiguous().view(torch.int32)


def ev(head, x, actions):
    """evaluate with no gradient wanted: the gsm_actor_eval launch."""
    with torch.no_grad():
        return head.evaluate(x, actions)


@pytest.mark.parametrize("B,N", SHAPES, ids=ids_s)
@pytest.mark.parametrize("F,hidden,A", HEADS, ids=ids_h)
def test_sample_against_fp64_and_oracle(F, hidden, A, B, N):
    head, x = make_head(F, hidden, A), make_x(B, N, F)
    draw, env_base = 99, 5
    act, logp, ent, lout = head.act(x, SEED, env_base=env_base, draw=draw, entropy=True, logits=True)
    assert int(head.status.item()) == 0
    assert act.dtype == torch.int32 and act.shape == (B, N) and lout.shape == (B, N, A)
    # logits
    ref_l = policy.actor_logits_ref(x.double(), *w64(head))
    e = float(((lout.double() - ref_l).abs() / (1 + ref_l.abs())).max())
    print(f"logits worst err/(1+|ref|) = {e:.3e}")
    assert e <= BOUND
    # actions: the inverse CDF of the kernel's own logits in fp64, u from the oracle
    u = oracle_u(B, N, SEED, env_base, draw).astype(np.float64)
    l64 = lout.double().cpu().numpy()
    p = np.exp(l64 - l64.max(-1, keepdims=True))
    cdf = np.cumsum(p, -1) / p.sum(-1, keepdims=True)
    want = np.minimum((u[..., None] >= cdf).sum(-1), A - 1)
    decided = np.abs(u[..., None] - cdf).min(-1) > 1e-5
    got = act.cpu().numpy()
    assert got.min() >= 0 and got.max() < A
    assert np.array_equal(got[decided], want[decided])
    share = 1.0 - decided.mean()
    print(f"rows not decided by the fp64 CDF: {share:.4%}")
    assert share <= 0.005
    # logp of the chosen action and the entropy
    ref_lp_all, ref_ent = policy.actor_dist_ref(ref_l)
    ref_lp = ref_lp_all.gather(-1, act.long()[..., None])[..., 0]
    e_lp = float(((logp.double() - ref_lp).abs() / (1 + ref_lp.abs())).max())
    e_en = float(((ent.double() - ref_ent).abs() / (1 + ref_ent.abs())).max())
    print(f"logp {e_lp:.3e}  entropy {e_en:.3e}")
    assert e_lp <= BOUND and e_en <= BOUND
    # the same bits from evaluate: the PPO ratio is exactly 1
    lp2, en2 = ev(head, x, act)
    assert torch.equal(bits(lp2), bits(logp)) and torch.equal(bits(en2), bits(ent))
    # deterministic mode: the first argmax of the returned logits, and again the same bits
    dact, dlogp, dl = head.act(x, SEED, deterministic=True, logits=True)
    assert torch.equal(dl, lout)
    first = (lout == lout.max(-1, keepdim=True)[0]).int().argmax(-1)   # of a 0/1 row: its first 1
    assert torch.equal(dact.long(), first)
    assert torch.equal(bits(ev(head, x, dact)[0]), bits(dlogp))


def test_sample_past_one_grid_of_tiles():
    """More tiles than the forward's grid has workgroups (2048 x 128 rows): a
    workgroup loops over tiles; the rows past the first round are checked like
    the others."""
    B, N, F, A = 90_000, 3, 4, 2
    head, x = make_head(F, 0, A), make_x(B, N, F)
    act, logp, lout = head.act(x, SEED, logits=True)
    ref_l = policy.actor_logits_ref(x.double(), *w64(head))
    assert float(((lout.double() - ref_l).abs() / (1 + ref_l.abs())).max()) <= BOUND
    ref = policy.actor_sample_ref(lout.double(), torch.from_numpy(oracle_u(B, N, SEED)).to(DEV))
    assert float((ref != act).float().mean()) <= 0.005
    assert torch.equal(bits(ev(head, x, act)[0]), bits(logp))


def test_sharding_is_a_slice_of_the_full_batch():
    B, N = 333, 6
    head, x = make_head(48, 64, 5), make_x(B, N, 48)
    full = head.act(x, SEED, draw=2, entropy=True, logits=True)
    for b0, b1 in ((0, 100), (100, 101), (129, 333)):
        part = head.act(x[b0:b1], SEED, env_base=b0, draw=2, entropy=True, logits=True)
        for f, p in zip(full, part):
            assert torch.equal(bits(f[b0:b1]), bits(p)), (b0, b1)


def test_repeatability_draw_seed_and_counter():
    B, N = 171, 24
    head, x = make_head(48, 16, 5), make_x(B, N, 48)
    a0, lp0 = head.act(x, SEED, draw=3)
    a1, lp1 = head.act(x, SEED, draw=3)
    assert torch.equal(a0, a1) and torch.equal(bits(lp0), bits(lp1))
    assert not torch.equal(a0, head.act(x, SEED, draw=4)[0])
    assert not torch.equal(a0, head.act(x, SEED + 1, draw=3)[0])
    c = torch.tensor([3], dtype=torch.int64, device=DEV)
    a2, lp2 = head.act(x, SEED, draw_counter=c)
    assert torch.equal(a0, a2) and torch.equal(bits(lp0), bits(lp2))
    a3, _ = head.act(x, SEED, draw=1, draw_counter=c - 1)   # the two add up
    assert torch.equal(a0, a3)
    # the torch formulation (use_kernel=False) samples by the same rule from the same draws
    slow = ActorHead(48, 16, 5, use_kernel=False).to(DEV)
    slow.load_state_dict(head.state_dict())
    a4, lp4 = slow.act(x, SEED, draw=3)
    assert float((a4 != a0).float().mean()) <= 0.005
    same = a4 == a0
    assert float((lp4 - lp0).abs()[same].max()) <= 1e-4


def _bwd(head, x, actions, g_logp, g_ent, want_dx=True, fill=float("nan")):
    """gsm_actor_eval_bwd called directly; returns (dw1, db1, dw2, db2, dx, status)."""
    lib = _lib.load()
    B, N, F = x.shape
    xk, stride = policy._rows(x)
    w1, b1, w2, b2 = head._weights()
    n = C.c_int64()
    assert lib.gsm_actor_backward_work_floats(F, head.hidden, head.n_actions, C.byref(n)) == 0
    work = torch.full((n.value,), fill, dtype=torch.float32, device=DEV)
    new = lambda t: torch.full_like(t, fill) if t is not None else None
    dw1, db1, dw2, db2 = new(w1), new(b1), new(w2), new(b2)
    dx = torch.full((B, N, F), fill, dtype=torch.float32, device=DEV) if want_dx else None
    status = torch.zeros(1, dtype=torch.int32, device=DEV)
    P = policy._ptr
    rc = lib.gsm_actor_eval_bwd(P(g_logp), P(g_ent), P(xk) if B else None, stride, P(w1), P(b1), P(w2), P(b2), B, N, F,
                                head.hidden, head.n_actions, P(actions), P(work), P(dw1), P(db1), P(dw2), P(db2),
                                P(dx) if B else None, P(status), policy._stream(torch.device(DEV)))
    assert rc == 0, _lib.last_error(lib)
    return dw1, db1, dw2, db2, dx, status


def _ref_bwd(head, x, actions, g_logp, g_ent):
    """fp64 autograd of the reference, and sum |terms| of every gradient entry."""
    xd = x.double().reshape(-1, x.shape[-1]).requires_grad_()
    ws = [t.clone().requires_grad_() if t is not None else None for t in w64(head)]
    w1, b1, w2, b2 = ws
    a = actions.reshape(-1).long()
    gl = g_logp.double().reshape(-1)
    ge = g_ent.double().reshape(-1) if g_ent is not None else None
    h = torch.relu(xd @ w1.t() + b1) if w1 is not None else xd
    lp_all, H = policy.actor_dist_ref(h @ w2.t() + b2)
    loss = (lp_all.gather(-1, a[:, None])[:, 0] * gl).sum() + ((H * ge).sum() if ge is not None else 0.0)
    names = [n for n, t in zip(("dw1", "db1", "dw2", "db2"), ws) if t is not None] + ["dx"]
    grads = dict(zip(names, torch.autograd.grad(loss, [t for t in ws if t is not None] + [xd])))
    with torch.no_grad():
        p = lp_all.exp()
        onehot = torch.nn.functional.one_hot(a, w2.shape[0]).double()
        dl = gl[:, None].abs() * (onehot + p)
        if ge is not None:
            dl = dl + ge[:, None].abs() * p * (lp_all.abs() + H[:, None].abs())
        scale = {"db2": 1 + dl.sum(0), "dw2": 1 + dl.t() @ h.abs()}
        dh = dl @ w2.abs()
        if w1 is not None:
            dh = dh * (h > 0)
            scale.update(dw1=1 + dh.t() @ xd.abs(), db1=1 + dh.sum(0), dx=1 + dh @ w1.abs())
        else:
            scale["dx"] = 1 + dh
    return grads, scale


BWD_SHAPES = [(7, 3), (1366, 3), (171, 24)]


@pytest.mark.parametrize("B,N", BWD_SHAPES, ids=[f"B{b}-N{n}" for b, n in BWD_SHAPES])
@pytest.mark.parametrize("F,hidden,A", HEADS, ids=ids_h)
def test_backward_against_fp64_autograd(F, hidden, A, B, N):
    head, x = make_head(F, hidden, A), make_x(B, N, F)
    g = torch.Generator(device=DEV).manual_seed(3)
    actions = torch.randint(0, A, (B, N), device=DEV, generator=g, dtype=torch.int32)
    g_logp = torch.randn(B, N, device=DEV, generator=g)
    g_ent = torch.randn(B, N, device=DEV, generator=g)
    got = dict(zip(("dw1", "db1", "dw2", "db2", "dx", "status"), _bwd(head, x, actions, g_logp, g_ent)))
    assert int(got["status"].item()) == 0
    ref, scale = _ref_bwd(head, x, actions, g_logp, g_ent)
    for name, r in ref.items():
        e = float(((got[name].double().reshape(r.shape) - r).abs() / scale[name]).max())
        print(f"{name}: worst err / (1 + sum|terms|) = {e:.3e}")
        assert e <= BOUND, name
    # bitwise reproducible
    again = _bwd(head, x, actions, g_logp, g_ent)
    for a, b in zip(again[:5], (got[k] for k in ("dw1", "db1", "dw2", "db2", "dx"))):
        assert (a is None and b is None) or torch.equal(bits(a), bits(b))
    # g_ent = NULL (zeros) and dx = NULL (not wanted)
    no = dict(zip(("dw1", "db1", "dw2", "db2", "dx"), _bwd(head, x, actions, g_logp, None, want_dx=False)))
    assert no["dx"] is None
    ref0, scale0 = _ref_bwd(head, x, actions, g_logp, None)
    for name in ("dw1", "db1", "dw2", "db2"):
        if name in ref0:
            assert float(((no[name].double() - ref0[name]).abs() / scale0[name]).max()) <= BOUND, name


def test_backward_past_one_grid_of_tiles():
    """More tiles than the backward's capped grid (512 x 128 rows): the
    workgroups accumulate several tiles before they write their partial."""
    B, N, F, hidden, A = 22_000, 3, 48, 16, 5
    head, x = make_head(F, hidden, A), make_x(B, N, F)
    g = torch.Generator(device=DEV).manual_seed(4)
    actions = torch.randint(0, A, (B, N), device=DEV, generator=g, dtype=torch.int32)
    g_logp = torch.randn(B, N, device=DEV, generator=g)
    g_ent = torch.randn(B, N, device=DEV, generator=g)
    got = dict(zip(("dw1", "db1", "dw2", "db2", "dx"), _bwd(head, x, actions, g_logp, g_ent)))
    ref, scale = _ref_bwd(head, x, actions, g_logp, g_ent)
    for name, r in ref.items():
        assert float(((got[name].double().reshape(r.shape) - r).abs() / scale[name]).max()) <= BOUND, name


def test_backward_of_no_envs_is_zeros():
    for F, hidden, A in ((48, 64, 5), (4, 0, 2)):
        head = make_head(F, hidden, A)
        x = torch.zeros(0, 3, F, device=DEV)
        empty = torch.zeros(0, 3, device=DEV)
        dw1, db1, dw2, db2, _, _ = _bwd(head, x, empty.int(), empty, empty)
        for t in (dw1, db1, dw2, db2):
            assert t is None or (t == 0).all()


@pytest.mark.parametrize("F,hidden,A", [(48, 64, 5), (4, 0, 2), (52, 32, 5)])
def test_module_backward_puts_the_kernel_gradients_on_the_parameters(F, hidden, A):
    B, N = 333, 6
    head, x = make_head(F, hidden, A, kernel_backward=True), make_x(B, N, F)
    x = x.requires_grad_()
    g = torch.Generator(device=DEV).manual_seed(5)
    actions = torch.randint(0, A, (B, N), device=DEV, generator=g, dtype=torch.int32)
    g_logp = torch.randn(B, N, device=DEV, generator=g)
    g_ent = torch.randn(B, N, device=DEV, generator=g)
    logp, ent = head.evaluate(x, actions)
    assert logp.grad_fn is not None and "ActorEval" in type(logp.grad_fn).__name__
    ((logp * g_logp).sum() + (ent * g_ent).sum()).backward()
    dw1, db1, dw2, db2, dx, _ = _bwd(head, x.detach(), actions, g_logp, g_ent)
    assert torch.equal(bits(head.lin2.weight.grad), bits(dw2)) and torch.equal(bits(head.lin2.bias.grad), bits(db2))
    if hidden:
        assert torch.equal(bits(head.lin1.weight.grad), bits(dw1))
        assert torch.equal(bits(head.lin1.bias.grad), bits(db1))
    assert torch.equal(bits(x.grad), bits(dx))
    # without kernel_backward the torch formulation trains, to the same gradients within the bound
    slow = make_head(F, hidden, A)
    slow.load_state_dict(head.state_dict())
    lp, en = slow.evaluate(x.detach(), actions)
    assert "ActorEval" not in type(lp.grad_fn).__name__
    ((lp * g_logp).sum() + (en * g_ent).sum()).backward()
    assert torch.allclose(slow.lin2.weight.grad, dw2, rtol=1e-3, atol=1e-3)


def test_gradient_reaches_the_conv_through_forward_env():
    B, N = 64, 3
    env = GpuBatchEnv(EnvConfig(n_envs=B, n_agents=N, seed=3), DEV)
    out = env.reset(seed=3)
    torch.manual_seed(0)
    conv = TransformerConv(7, 16, heads=2, kernel_backward=True).to(DEV)
    head = make_head(32, 16, 5, kernel_backward=True)
    feats = conv.forward_env(out, rows="agents", n_agents=N)
    assert feats.shape == (B, N, 32) and feats.requires_grad
    with torch.no_grad():
        actions, logp0 = head.act(feats.detach(), SEED)
    logp, ent = head.evaluate(feats, actions)
    assert torch.equal(bits(logp.detach()), bits(logp0))
    (logp.sum() + 0.01 * ent.sum()).backward()
    for lin in (conv.lin_query, conv.lin_key, conv.lin_value, conv.lin_skip):
        assert lin.weight.grad is not None and torch.isfinite(lin.weight.grad).all()
        assert float(lin.weight.grad.abs().sum()) > 0
    assert float(head.lin1.weight.grad.abs().sum()) > 0
    env.close()


def test_status_nonfinite_row_and_bad_action():
    B, N = 333, 6
    head, x = make_head(48, 64, 5), make_x(B, N, 48)
    clean = head.act(x, SEED, entropy=True, logits=True)
    assert int(head.status.item()) == 0
    bad = x.clone()
    bad[100, 2, 7] = float("nan")
    got = head.act(bad, SEED, entropy=True, logits=True)
    assert int(head.status.item()) == _lib.ACTOR_NONFINITE
    assert int(got[0][100, 2]) == 0 and torch.isnan(got[1][100, 2])
    keep = torch.ones(B, N, dtype=torch.bool, device=DEV)
    keep[100, 2] = False
    for c, g in zip(clean, got):
        assert torch.equal(bits(c)[keep], bits(g)[keep])
    lp, _ = ev(head, bad, clean[0])
    assert int(head.status.item()) == _lib.ACTOR_NONFINITE and torch.isnan(lp[100, 2])
    assert torch.equal(bits(lp)[keep], bits(clean[1])[keep])
    actions = clean[0].clone()
    actions[5, 1] = 7
    lp, en = ev(head, x, actions)
    assert int(head.status.item()) == _lib.ACTOR_BAD_ACTION
    assert torch.isnan(lp[5, 1]) and int(torch.isnan(lp).sum()) == 1
    assert torch.equal(bits(en), bits(clean[2]))


def test_captured_act_counter_and_step_replay():
    """act(draw_counter=c), c.add_(1) and env.step recorded into one
    torch.cuda.graph: each replay draws with the counter's current value, so
    three replays equal eager steps with draws d, d+1, d+2 from the same state."""
    B, N, d = 300, 6, 7
    head = make_head(4, 16, 5)

    def fresh():
        env = GpuBatchEnv(EnvConfig(n_envs=B, n_agents=N, seed=9), DEV)
        env.reset(seed=9, sync_edges=False)
        return env, env.t["node_feat"][:, :N, :4]

    def snap(env, actions):
        return {"actions": actions.clone()} | {k: env.t[k].clone() for k in ("node_feat", "reward", "cost", "done",
                                                                             "edge_ptr")}

    env, x = fresh()
    c = torch.tensor([d], dtype=torch.int64, device=DEV)
    side = torch.cuda.Stream(device=DEV)
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        head.act(x, SEED, draw_counter=c)            # warm the kernels; no step, no advance
    torch.cuda.current_stream().wait_stream(side)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        actions, _ = head.act(x, SEED, draw_counter=c)
        c.add_(1)
        env.step(actions, sync_edges=False)          # recorded, not run
    replays = []
    for _ in range(3):
        g.replay()
        replays.append(snap(env, actions))
    torch.cuda.synchronize()
    assert int(c.item()) == d + 3
    del g
    env.close()
    env, x = fresh()
    for t in range(3):
        a, _ = head.act(x, SEED, draw=d + t)
        env.step(a, sync_edges=False)
        want = snap(env, a)
        for k, v in want.items():
            assert torch.equal(replays[t][k], v), (t, k)
    env.close()
    assert not torch.equal(replays[0]["actions"], replays[1]["actions"])
    assert not torch.equal(replays[1]["actions"], replays[2]["actions"])
    assert not torch.equal(replays[0]["actions"], replays[2]["actions"])
