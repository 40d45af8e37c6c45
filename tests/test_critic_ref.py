"""The critic head without a GPU: the torch restatements of gsmarl_amd.policy
(critic_values_ref, critic_bwd_ref) against an independent fp64 composition
and fp64 autograd, the host-side argument checks of the library's entry
points, the workspace size, PopArt's output-preserving update and the module's
fallback off the GPU."""
import ctypes as C

import pytest
import torch

from gsmarl_amd import CriticHead, PopArt, _lib, policy


def make(B, N, F, H, O, seed=0, dtype=torch.float64):
    g = torch.Generator().manual_seed(seed)
    rnd = lambda *s: torch.randn(*s, generator=g, dtype=dtype)
    return rnd(B, N, F), rnd(H, 2 * F) * 0.4, rnd(H) * 0.4, rnd(O, H) * 0.4, rnd(O) * 0.4


def composed(x, w1, b1, w2, b2, n_valid=None, denorm=None):
    """mean, cat, F.linear: an env at a time so that padding needs no masking."""
    B, N, F = x.shape
    out = torch.zeros(w2.shape[0], B, N, dtype=x.dtype)
    for b in range(B):
        n = N if n_valid is None else int(n_valid[b])
        if n == 0:
            continue
        xb = x[b, :n]
        pool = xb.mean(0, keepdim=True).expand(n, F)
        h = torch.relu(torch.nn.functional.linear(torch.cat([pool, xb], 1), w1, b1))
        v = torch.nn.functional.linear(h, w2, b2)
        if denorm is not None:
            v = v * denorm[:, 1] + denorm[:, 0]
        out[:, b, :n] = v.t()
    return out


N_VALID = torch.tensor([3, 0, 5, 1, 2, 5, 4])


@pytest.mark.parametrize("ragged", [False, True])
@pytest.mark.parametrize("with_denorm", [False, True])
def test_values_ref_against_composition_fp64(ragged, with_denorm):
    B, N, F, H, O = 7, 5, 12, 16, 2
    x, w1, b1, w2, b2 = make(B, N, F, H, O)
    n_valid = N_VALID if ragged else None
    denorm = torch.tensor([[0.7, 2.5], [-3.0, 0.25]], dtype=torch.float64) if with_denorm else None
    xin = x.clone()
    if ragged:                                   # padded rows are not read
        for b in range(B):
            xin[b, int(n_valid[b]):] = float("nan")
    got = policy.critic_values_ref(xin, w1, b1, w2, b2, n_valid, denorm)
    want = composed(x, w1, b1, w2, b2, n_valid, denorm)
    assert got.shape == (O, B, N) and got.is_contiguous()
    e = float((got - want).abs().max())
    print(f"values worst abs err = {e:.3e}")
    assert e <= 1e-12
    if ragged:
        for b in range(B):
            assert (got[:, b, int(n_valid[b]):] == 0).all()


@pytest.mark.parametrize("ragged", [False, True])
@pytest.mark.parametrize("O", [1, 2])
def test_bwd_ref_against_autograd_fp64(ragged, O):
    B, N, F, H = 7, 5, 12, 32
    x, w1, b1, w2, b2 = make(B, N, F, H, O, seed=1 + O)
    n_valid = N_VALID if ragged else None        # holds an env of 0 and an env of 1 valid agents
    g = torch.randn(O, B, N, generator=torch.Generator().manual_seed(9), dtype=torch.float64)
    leaves = [t.clone().requires_grad_() for t in (w1, b1, w2, b2, x)]
    v = policy.critic_values_ref(leaves[4], *leaves[:4], n_valid)
    want = torch.autograd.grad((v * g).sum(), leaves)
    with torch.no_grad():
        got = policy.critic_bwd_ref(g, x, w1, b1, w2, b2, n_valid)
    for name, a, b in zip(("dw1", "db1", "dw2", "db2", "dx"), got, want):
        e = float((a - b).abs().max())
        print(f"{name}: worst abs err = {e:.3e}")
        assert a.shape == b.shape and e <= 1e-10, name
    if ragged:
        for b in range(B):
            assert (got[4][b, int(n_valid[b]):] == 0).all()
    # denormalisation is not part of it: the gradient is with respect to the raw v
    assert float(got[0][:, :F].abs().sum()) > 0   # the pool path carries gradient


@pytest.fixture(scope="module")
def lib():
    if not _lib.LIB_PATH.exists():
        import __graft_entry__ as g
        g.build()
    return _lib.load()


BAD_SHAPES = [dict(F=0), dict(F=2), dict(F=68), dict(hidden=0), dict(hidden=8), dict(hidden=128), dict(O=0),
              dict(O=3), dict(N=0), dict(N=129), dict(stride=50), dict(stride=44)]


@pytest.mark.parametrize("bad", BAD_SHAPES, ids=lambda d: "-".join(f"{k}{v}" for k, v in d.items()))
def test_entry_points_reject_bad_shapes_on_the_host(lib, bad):
    """GSM_EINVAL before a pointer is looked at or anything is launched."""
    s = dict(F=48, hidden=64, O=2, N=3, stride=None)
    s.update(bad)
    F, hidden, O, N = s["F"], s["hidden"], s["O"], s["N"]
    stride = s["stride"] if s["stride"] is not None else F
    p = C.c_void_p(4096)
    rc = lib.gsm_critic_eval(p, stride, None, p, p, p, p, None, 4, N, F, hidden, O, p, None, None)
    assert rc == _lib.GSM_EINVAL and _lib.last_error(lib)
    rc = lib.gsm_critic_eval_bwd(p, p, stride, None, p, p, p, p, 4, N, F, hidden, O, p, p, p, p, p, None, None, None)
    assert rc == _lib.GSM_EINVAL
    if "stride" not in bad and "N" not in bad:
        assert lib.gsm_critic_backward_work_floats(F, hidden, O, C.byref(C.c_int64())) == _lib.GSM_EINVAL


def test_entry_points_reject_bad_arguments_on_the_host(lib):
    p = C.c_void_p(4096)
    shape = (4, 3, 48, 64, 2)
    ev = lambda x, w1, values, n_envs=4: lib.gsm_critic_eval(x, 48, None, w1, p, p, p, None, n_envs, *shape[1:],
                                                              values, None, None)
    assert ev(None, p, p) == _lib.GSM_EINVAL                        # x NULL
    assert ev(C.c_void_p(4100), p, p) == _lib.GSM_EINVAL            # x not 16-byte aligned
    assert ev(p, None, p) == _lib.GSM_EINVAL                        # w1 NULL
    assert ev(p, p, None) == _lib.GSM_EINVAL                        # values NULL
    assert ev(p, p, p, n_envs=1 << 30) == _lib.GSM_EINVAL           # R >= 2^31
    bw = lambda g, work, dw1, dx: lib.gsm_critic_eval_bwd(g, p, 48, None, p, p, p, p, *shape, work, dw1, p, p, p, dx,
                                                          None, None)
    assert bw(p, p, None, None) == _lib.GSM_EINVAL                  # dw1 NULL
    assert bw(None, p, p, None) == _lib.GSM_EINVAL                  # g NULL
    assert bw(p, None, p, None) == _lib.GSM_EINVAL                  # work NULL
    assert bw(p, p, p, C.c_void_p(4100)) == _lib.GSM_EINVAL         # dx not 16-byte aligned
    assert lib.gsm_critic_backward_work_floats(48, 64, 2, None) == _lib.GSM_EINVAL
    # nothing to do: no pointer is needed and nothing is launched
    assert lib.gsm_critic_eval(None, 48, None, None, None, None, None, None, 0, 3, 48, 64, 2, None, None,
                               None) == _lib.GSM_OK


@pytest.mark.parametrize("F,hidden,O", [(48, 64, 2), (64, 64, 2), (4, 16, 1), (52, 32, 2)])
def test_backward_work_floats(lib, F, hidden, O):
    n = C.c_int64()
    assert lib.gsm_critic_backward_work_floats(F, hidden, O, C.byref(n)) == _lib.GSM_OK
    partial = hidden * 2 * F + hidden + O * hidden + O            # dw1, db1, dw2, db2 of one workgroup
    assert n.value > 0 and n.value % partial == 0
    assert n.value // partial <= 1024                             # a few workgroups per CU
    assert policy.critic_work_floats(F, hidden, O) == n.value     # what the module's backward allocates


def test_popart_update_preserves_the_denormalised_values():
    torch.manual_seed(0)
    B, N, F = 9, 4, 8
    head = CriticHead(F, hidden=16, n_out=2)
    pop = PopArt(2, beta=0.9)
    x = torch.randn(B, N, F)
    returns = torch.stack([torch.randn(B, N) * 3.0 + 5.0, torch.rand(B, N) * 0.5])
    for step in range(3):
        with torch.no_grad():
            before = policy.critic_values_ref(x, *head._weights(), denorm=pop.stats())
        old = pop.stats().clone()
        pop.update(returns * (1.0 + step), head)
        assert not torch.equal(old, pop.stats())
        with torch.no_grad():
            after = policy.critic_values_ref(x, *head._weights(), denorm=pop.stats())
        e = float(((after - before).abs() / before.abs().clamp(min=1.0)).max())
        print(f"update {step}: worst relative change of the denormalised values = {e:.3e}")
        assert e <= 1e-5
    # without a head only the statistics move
    w = head.lin2.weight.clone()
    pop.update(returns)
    assert torch.equal(w, head.lin2.weight)


def test_popart_normalize_has_the_reported_moments():
    pop = PopArt(2)
    g = torch.Generator().manual_seed(3)
    returns = torch.stack([torch.randn(64, 6, generator=g) * 2.0 + 1.0, torch.randn(64, 6, generator=g) * 0.5 - 2.0])
    assert torch.equal(pop.stats(), torch.tensor([[0.0, 0.1], [0.0, 0.1]]))      # nothing seen: variance floor
    pop.update(returns)
    st = pop.stats()
    assert st.shape == (2, 2) and st.dtype == torch.float32
    flat = returns.reshape(2, -1)
    assert torch.allclose(st[:, 0], flat.mean(1), rtol=1e-4, atol=1e-5)          # debiased: the data's own moments
    assert torch.allclose(st[:, 1], flat.std(1, unbiased=False), rtol=1e-3)
    z = pop.normalize(returns).reshape(2, -1)
    assert float(z.mean(1).abs().max()) <= 1e-4
    assert float((z.std(1, unbiased=False) - 1).abs().max()) <= 1e-3
    # a constant head hits the variance floor of 1e-2
    flatpop = PopArt(1)
    flatpop.update(torch.full((1, 10), 4.0))
    assert torch.allclose(flatpop.stats(), torch.tensor([[4.0, 0.1]]), rtol=1e-4)


def test_off_gpu_forward_falls_back_to_the_restatement():
    torch.manual_seed(1)
    head = CriticHead(12, hidden=16, n_out=2, kernel_backward=True)
    x = torch.randn(6, 3, 12)
    n_valid = torch.tensor([3, 1, 0, 2, 3, 3])
    denorm = torch.tensor([[1.0, 2.0], [0.5, 0.1]])
    v = head(x, n_valid, denorm)
    assert v.shape == (2, 6, 3) and v.grad_fn is not None and head.status is None
    want = composed(x.double(), *(t.detach().double() for t in head._weights()), n_valid, denorm.double())
    assert float((v.detach().double() - want).abs().max()) <= 1e-5
    v.sum().backward()
    assert all(p.grad is not None and p.grad.abs().sum() > 0 for p in head.parameters())
    with pytest.raises(ValueError):
        head(torch.randn(6, 3, 8))
    with pytest.raises(ValueError):
        head(x, denorm=torch.zeros(3, 2))
    one = CriticHead(12, hidden=16, n_out=1).double()
    assert one(x.double()).shape == (1, 6, 3) and one(x.double()).dtype == torch.float64
