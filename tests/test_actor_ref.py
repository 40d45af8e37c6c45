"""The actor head without a GPU: the torch restatements of gsmarl_amd.policy
against numpy in fp64 and against autograd, the draw's counter convention
against the Philox oracle, and the host-side argument checks of the three
library entry points."""
import ctypes as C

import numpy as np
import pytest
import torch

from gsmarl_amd import ActorHead, _lib, policy
from oracle import philox

TAG = 3


def oracle_u(B, N, seed, env_base=0, draw=0):
    """u [B, N] by the documented convention: counter (agent, draw, env_base + env, 3)."""
    i = np.arange(N, dtype=np.uint64)[None, :]
    b = (np.arange(B, dtype=np.uint64)[:, None] + np.uint64(env_base)) & np.uint64(0xFFFFFFFF)
    x0 = philox.philox4x32_10(i, np.uint64(draw & 0xFFFFFFFF), b, TAG, seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF)[0]
    return philox.u01_f32(x0)


def numpy_inverse_cdf(logits64, u):
    p = np.exp(logits64 - logits64.max(-1, keepdims=True))
    cdf = np.cumsum(p, -1) / p.sum(-1, keepdims=True)
    act = (u.astype(np.float64)[..., None] >= cdf).sum(-1)
    return np.minimum(act, logits64.shape[-1] - 1), cdf


@pytest.mark.parametrize("env_base,draw", [(0, 0), (5, 0), (5, 99), (2 ** 32 - 2, 1)])
def test_uniform_ref_is_the_oracles_counter_convention(env_base, draw):
    B, N, seed = 9, 4, 0x1234_5678_9ABC_DEF1
    u = policy.actor_uniform_ref(B, N, seed, env_base, draw).numpy()
    assert np.array_equal(u, oracle_u(B, N, seed, env_base, draw))
    ut = policy.actor_uniform_ref(B, N, seed, env_base, torch.tensor([draw], dtype=torch.int64)).numpy()
    assert np.array_equal(u, ut)
    assert u.min() >= 0.0 and u.max() < 1.0


@pytest.mark.parametrize("sigma", [0.5, 2.0, 6.0])
@pytest.mark.parametrize("env_base", [0, 5])
def test_sampling_rule_against_numpy_inverse_cdf(sigma, env_base):
    B, N, A, seed = 400, 6, 5, 11
    g = torch.Generator().manual_seed(int(sigma * 10) + env_base)
    logits = (torch.randn(B, N, A, generator=g) * sigma)
    u = oracle_u(B, N, seed, env_base, draw=1)
    got = policy.actor_sample_ref(logits, torch.from_numpy(u)).numpy()
    want, cdf = numpy_inverse_cdf(logits.double().numpy(), u)
    decided = np.abs(u.astype(np.float64)[..., None] - cdf).min(-1) > 1e-5
    assert got.dtype == np.int32 and got.min() >= 0 and got.max() < A
    assert np.array_equal(got[decided], want[decided])
    assert 1.0 - decided.mean() <= 0.005
    # in fp64 the rule is the inverse CDF on every decided row as well
    got64 = policy.actor_sample_ref(logits.double(), torch.from_numpy(u)).numpy()
    assert np.array_equal(got64[decided], want[decided])


def test_sampling_rule_edges():
    l = torch.tensor([[0.0, 0.0, 0.0], [-1e4, 5.0, -1e4], [3.0, 3.0, -2.0]])
    assert policy.actor_sample_ref(l, torch.tensor([0.0, 0.0, 0.0])).tolist() == [0, 1, 0]
    # u*s rounding up to s picks the last action; here u = 1 stands for it
    assert policy.actor_sample_ref(l, torch.tensor([1.0, 1.0, 1.0])).tolist() == [2, 2, 2]
    assert policy.actor_sample_ref(l, torch.tensor([0.4, 0.5, 0.6])).tolist() == [1, 1, 1]


def test_counters_are_distinct():
    B, N, seed = 16, 6, 7
    base = oracle_u(B, N, seed)
    assert len(np.unique(base)) == B * N                      # across agents and envs
    for other in (oracle_u(B, N, seed, draw=1), oracle_u(B, N, seed + 1), oracle_u(B, N, seed + (1 << 32)),
                  oracle_u(B, N, seed, env_base=B)):
        assert (other != base).mean() > 0.99
    # a shard is its slice of the full batch
    assert np.array_equal(oracle_u(B, N, seed, env_base=3)[:5], oracle_u(B, N, seed)[3:8])
    assert np.array_equal(policy.actor_uniform_ref(5, N, seed, 3).numpy(), base[3:8])


def test_dist_ref_matches_log_softmax():
    l = torch.randn(50, 3, 7, dtype=torch.float64) * 4
    logp, ent = policy.actor_dist_ref(l)
    ref = torch.log_softmax(l, -1)
    assert (logp - ref).abs().max() <= 1e-12
    assert (ent + (ref.exp() * ref).sum(-1)).abs().max() <= 1e-12


@pytest.mark.parametrize("hidden", [0, 32])
@pytest.mark.parametrize("with_ent", [False, True])
def test_eval_bwd_ref_against_autograd_fp64(hidden, with_ent):
    R, F, A = 37, 12, 5
    g = torch.Generator().manual_seed(hidden + with_ent)
    rnd = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)
    x = rnd(R, F).requires_grad_()
    w1 = (rnd(hidden, F) * 0.4).requires_grad_() if hidden else None
    b1 = (rnd(hidden) * 0.4).requires_grad_() if hidden else None
    w2 = (rnd(A, hidden or F) * 0.4).requires_grad_()
    b2 = (rnd(A) * 0.4).requires_grad_()
    actions = torch.randint(0, A, (R,), generator=g)
    g_logp, g_ent = rnd(R), (rnd(R) if with_ent else None)
    logp_all, ent = policy.actor_dist_ref(policy.actor_logits_ref(x, w1, b1, w2, b2))
    loss = (logp_all.gather(-1, actions[:, None])[:, 0] * g_logp).sum()
    if with_ent:
        loss = loss + (ent * g_ent).sum()
    params = [t for t in (w1, b1, w2, b2, x) if t is not None]
    want = dict(zip([n for n, t in zip(("dw1", "db1", "dw2", "db2", "dx"), (w1, b1, w2, b2, x)) if t is not None],
                    torch.autograd.grad(loss, params)))
    with torch.no_grad():
        got = dict(zip(("dw1", "db1", "dw2", "db2", "dx"),
                       policy.actor_eval_bwd_ref(g_logp, g_ent, x, w1, b1, w2, b2, actions)))
    for name, w in want.items():
        assert (got[name] - w).abs().max() <= 1e-10, name
    if not hidden:
        assert got["dw1"] is None and got["db1"] is None


@pytest.fixture(scope="module")
def lib():
    if not _lib.LIB_PATH.exists():
        import __graft_entry__ as g
        g.build()
    return _lib.load()


BAD_SHAPES = [dict(F=6), dict(F=132), dict(F=0), dict(hidden=8), dict(A=1), dict(A=9), dict(stride=44),
              dict(stride=50)]


@pytest.mark.parametrize("bad", BAD_SHAPES, ids=lambda d: "-".join(f"{k}{v}" for k, v in d.items()))
def test_entry_points_reject_bad_shapes_on_the_host(lib, bad):
    """GSM_EINVAL before a pointer is looked at or anything is launched."""
    s = dict(F=48, hidden=64, A=5, stride=None)
    s.update(bad)
    F, hidden, A = s["F"], s["hidden"], s["A"]
    stride = s["stride"] if s["stride"] is not None else F
    p = C.c_void_p(4096)
    rc = lib.gsm_actor_sample(p, stride, p, p, p, p, 4, 3, F, hidden, A, 1, 0, 0, None, 0, p, p, None, None, None, None)
    assert rc == _lib.GSM_EINVAL and _lib.last_error(lib)
    rc = lib.gsm_actor_eval(p, stride, p, p, p, p, 4, 3, F, hidden, A, p, p, None, None, None)
    assert rc == _lib.GSM_EINVAL
    rc = lib.gsm_actor_eval_bwd(p, None, p, stride, p, p, p, p, 4, 3, F, hidden, A, p, p, p, p, p, p, None, None, None)
    assert rc == _lib.GSM_EINVAL
    if "stride" not in bad:
        assert lib.gsm_actor_backward_work_floats(F, hidden, A, C.byref(C.c_int64())) == _lib.GSM_EINVAL


def test_entry_points_reject_bad_arguments_on_the_host(lib):
    p = C.c_void_p(4096)
    ok = (p, 48, p, p, p, p)
    assert lib.gsm_actor_sample(*ok, 4, 3, 48, 64, 5, 1, 0, 0, None, 2, p, p, None, None, None, None) == _lib.GSM_EINVAL
    assert "flags" in _lib.last_error(lib)
    assert lib.gsm_actor_sample(*ok, 1 << 30, 3, 48, 64, 5, 1, 0, 0, None, 0, p, p, None, None, None,
                                None) == _lib.GSM_EINVAL                       # R >= 2^31
    assert lib.gsm_actor_sample(None, 48, p, p, p, p, 4, 3, 48, 64, 5, 1, 0, 0, None, 0, p, p, None, None, None,
                                None) == _lib.GSM_EINVAL                       # x NULL
    assert lib.gsm_actor_sample(C.c_void_p(4100), 48, p, p, p, p, 4, 3, 48, 64, 5, 1, 0, 0, None, 0, p, p, None,
                                None, None, None) == _lib.GSM_EINVAL           # x not 16-byte aligned
    assert lib.gsm_actor_eval(*ok, 4, 3, 48, 64, 5, None, p, None, None, None) == _lib.GSM_EINVAL   # actions NULL
    assert lib.gsm_actor_eval(p, 48, None, None, p, p, 4, 3, 48, 64, 5, p, p, None, None, None) == _lib.GSM_EINVAL
    assert lib.gsm_actor_eval_bwd(p, None, *ok, 4, 3, 48, 64, 5, p, p, None, p, p, p, None, None,
                                  None) == _lib.GSM_EINVAL                     # dw1 NULL with a hidden layer
    # nothing to do: no pointer is needed and nothing is launched
    assert lib.gsm_actor_sample(None, 48, None, None, None, None, 0, 3, 48, 64, 5, 1, 0, 0, None, 0, None, None, None,
                                None, None, None) == _lib.GSM_OK
    assert lib.gsm_actor_eval(None, 48, None, None, None, None, 0, 3, 48, 64, 5, None, None, None, None,
                              None) == _lib.GSM_OK


@pytest.mark.parametrize("F,hidden,A", [(48, 64, 5), (128, 64, 8), (4, 0, 2), (52, 32, 5)])
def test_backward_work_floats(lib, F, hidden, A):
    n = C.c_int64()
    assert lib.gsm_actor_backward_work_floats(F, hidden, A, C.byref(n)) == _lib.GSM_OK
    partial = hidden * F + hidden + A * (hidden or F) + A       # dw1, db1, dw2, db2 of one workgroup
    assert n.value > 0 and n.value % partial == 0
    assert n.value // partial <= 1024                           # a few workgroups per CU
    assert lib.gsm_actor_backward_work_floats(F, hidden, A, None) == _lib.GSM_EINVAL


def test_off_gpu_act_raises_and_evaluate_falls_back():
    head = ActorHead(12, hidden=16, n_actions=5)
    x = torch.randn(6, 3, 12)
    with pytest.raises(_lib.GsmError, match="GPU"):
        head.act(x, seed=1)
    actions = torch.randint(0, 5, (6, 3), dtype=torch.int32)
    logp, ent = head.evaluate(x, actions)
    ref = torch.log_softmax(head.lin2(torch.relu(head.lin1(x))), -1)
    assert torch.allclose(logp, ref.gather(-1, actions.long()[..., None])[..., 0], atol=1e-6)
    assert torch.allclose(ent, -(ref.exp() * ref).sum(-1), atol=1e-6)
    (logp.sum() + ent.sum()).backward()
    assert all(p.grad is not None and p.grad.abs().sum() > 0 for p in head.parameters())
    # the linear head, in fp64
    lin = ActorHead(12, hidden=0, n_actions=3).double()
    assert lin.lin1 is None
    logp, _ = lin.evaluate(x.double(), actions % 3)
    assert logp.dtype == torch.float64 and logp.shape == (6, 3)
