"""The critic head on the GPU (gsm_critic_eval / gsm_critic_eval_bwd behind
gsmarl_amd.policy.CriticHead) against the fp64 torch restatements.

Bounds (those of test_gpu_actor.py): values within 2e-5 * (1 + |ref|) of the
fp64 restatement; weight gradients and dx within 2e-5 * (1 + sum |terms|) of
fp64 autograd, sum |terms| being the same sums formed from the absolute values
of their factors. Everything the contract calls bit for bit is compared as
int32 words."""
import ctypes as C

import pytest
import torch

from gsmarl_amd import CriticHead, EnvConfig, GpuBatchEnv, GraphRolloutBuffer, PopArt, _lib, policy
from gsmarl_amd.gnn import TransformerConv

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BOUND = 2e-5
FWD_GRID, BWD_GRID = 2048, 512           # the kernels' grid caps, in tiles

# (B, N): 42 envs a tile; 5 envs a tile, 120 of 128 rows; many tiles; one env a tile (96 and 128
# rows); N = 1: pool = x and the cap of 64 envs a tile; a last partial tile
SHAPES = [(7, 3), (171, 24), (1366, 3), (5, 96), (3, 128), (300, 1), (40, 5)]
HEADS = [(4, 16, 1), (48, 64, 2), (64, 64, 2), (52, 32, 2)]
ids_s = [f"B{b}-N{n}" for b, n in SHAPES]
ids_h = [f"in{f}-h{h}-o{o}" for f, h, o in HEADS]


def make_head(F, hidden, O, seed=0, **kw):
    torch.manual_seed(seed)
    head = CriticHead(F, hidden, O, **kw).to(DEV)
    with torch.no_grad():
        head.lin1.weight.mul_(2.0)          # pool and x halves both matter, relu cuts about half
        head.lin2.bias.uniform_(-1.0, 1.0)
    return head


def make_x(B, N, F, seed=1):
    g = torch.Generator(device=DEV).manual_seed(seed)
    if F == 52:                              # a view of wider rows: row stride 64
        return torch.randn(B, N, 64, device=DEV, generator=g)[:, :, :F]
    return torch.randn(B, N, F, device=DEV, generator=g)


def make_counts(B, N, seed=2):
    g = torch.Generator(device=DEV).manual_seed(seed)
    n = torch.randint(0, N + 1, (B,), device=DEV, generator=g, dtype=torch.int32)
    n[0], n[B - 1] = N, 0                    # both ends are there whatever the draw
    if B > 2:
        n[1] = 1
    return n


def w64(head):
    return [t.detach().double() for t in head._weights()]


def bits(t):
    return t.contiguous().view(torch.int32)


def fwd(head, x, n_valid=None, denorm=None):
    """forward with no gradient wanted: the gsm_critic_eval launch."""
    with torch.no_grad():
        return head(x, n_valid, denorm)


def check_values(got, head, x, n_valid=None, denorm=None, what="values"):
    ref = policy.critic_values_ref(x.double(), *w64(head), n_valid, denorm.double() if denorm is not None else None)
    e = float(((got.double() - ref).abs() / (1 + ref.abs())).max())
    print(f"{what}: worst err / (1 + |ref|) = {e:.3e}")
    assert got.shape == ref.shape and e <= BOUND


@pytest.mark.parametrize("B,N", SHAPES, ids=ids_s)
@pytest.mark.parametrize("F,hidden,O", HEADS, ids=ids_h)
def test_forward_against_fp64(F, hidden, O, B, N):
    head, x = make_head(F, hidden, O), make_x(B, N, F)
    v = fwd(head, x)
    assert int(head.status.item()) == 0
    assert v.shape == (O, B, N) and v.is_contiguous() and v.dtype == torch.float32
    check_values(v, head, x)
    # ragged, with NaN in the padded rows, and denormalised
    n_valid = make_counts(B, N)
    st = torch.tensor([[0.5, 3.0], [-2.0, 0.25]], device=DEV)[:O].contiguous()
    xr = x.clone()
    xr[torch.arange(N, device=DEV)[None, :] >= n_valid[:, None]] = float("nan")
    vr = fwd(head, xr, n_valid, st)
    assert int(head.status.item()) == 0
    check_values(vr, head, xr, n_valid, st, "ragged, denormalised")


def test_forward_past_one_grid_of_tiles():
    """More tiles than the forward's grid has workgroups (2048 tiles of 42
    envs at 3 agents): a workgroup loops over tiles."""
    B, N, F = FWD_GRID * 42 + 300, 3, 4
    head, x = make_head(F, 16, 1), make_x(B, N, F)
    check_values(fwd(head, x), head, x)


def test_n_valid_padding_and_dense_batches_of_equal_count():
    B, N, F, hidden, O = 97, 6, 48, 64, 2
    head, x = make_head(F, hidden, O), make_x(B, N, F)
    n_valid = make_counts(B, N)
    pad = torch.arange(N, device=DEV)[None, :] >= n_valid[:, None]
    xr = x.clone()
    xr[pad] = float("nan")                   # padded rows are not read
    v = fwd(head, xr, n_valid)
    assert int(head.status.item()) == 0
    assert (bits(v)[:, pad] == 0).all()      # exactly +0.0
    g = torch.randn(O, B, N, device=DEV, generator=torch.Generator(device=DEV).manual_seed(7))
    got = _bwd(head, xr, g, n_valid)
    assert (bits(got["dx"])[pad] == 0).all() and torch.isfinite(got["dx"]).all()
    for name in ("dw1", "db1", "dw2", "db2"):
        assert torch.isfinite(got[name]).all(), name
    for n in range(1, N + 1):
        idx = (n_valid == n).nonzero()[:, 0]
        if idx.numel() == 0:
            continue
        xd = x[idx, :n].contiguous()
        vd = fwd(head, xd)
        assert torch.equal(bits(vd), bits(v[:, idx, :n])), n
        dd = _bwd(head, xd, g[:, idx, :n].contiguous())
        assert torch.equal(bits(dd["dx"]), bits(got["dx"][idx, :n])), n


def test_locality_one_env_changes_only_itself():
    B, N = 171, 24                           # 5 envs a tile
    head, x = make_head(48, 64, 2), make_x(B, N, 48)
    v = fwd(head, x)
    x2 = x.clone()
    x2[7, 3:9] += 1.0                        # env 7: the third env of the second tile
    v2 = fwd(head, x2)
    keep = torch.ones(B, dtype=torch.bool, device=DEV)
    keep[7] = False
    assert torch.equal(bits(v)[:, keep], bits(v2)[:, keep])
    assert (bits(v)[:, 7] != bits(v2)[:, 7]).any(1).all()   # env 7 itself moves, in both heads


@pytest.mark.parametrize("B,N", [(171, 24), (300, 3), (200, 1)], ids=["N24", "N3", "N1"])
def test_a_slice_of_the_batch_is_its_rows_of_the_full_batch(B, N):
    head, x = make_head(48, 64, 2), make_x(B, N, 48)
    n_valid = make_counts(B, N)
    full, full_r = fwd(head, x), fwd(head, x, n_valid)
    for b0, b1 in ((0, 100), (100, 101), (3, B), (7, 12), (43, 170)):
        assert torch.equal(bits(fwd(head, x[b0:b1])), bits(full[:, b0:b1])), (b0, b1)
        assert torch.equal(bits(fwd(head, x[b0:b1], n_valid[b0:b1])), bits(full_r[:, b0:b1])), (b0, b1)


def test_denorm_is_a_multiply_then_an_add_read_at_run_time():
    B, N = 171, 24
    head, x = make_head(48, 64, 2), make_x(B, N, 48)
    raw = fwd(head, x)
    pop = PopArt(2).to(DEV)
    pop.update(torch.stack([torch.randn(B, N, device=DEV) * 3 + 5, torch.rand(B, N, device=DEV)]))
    st = pop.stats()
    want = raw * st[:, 1, None, None]
    want = want + st[:, 0, None, None]
    assert torch.equal(bits(fwd(head, x, denorm=st)), bits(want))
    st.copy_(torch.tensor([[1.5, 0.75], [-4.0, 2.0]], device=DEV))   # in place: the same tensor, new statistics
    want2 = raw * st[:, 1, None, None]
    want2 = want2 + st[:, 0, None, None]
    got2 = fwd(head, x, denorm=st)
    assert torch.equal(bits(got2), bits(want2)) and not torch.equal(bits(got2), bits(want))


def _bwd(head, x, g, n_valid=None, want_dx=True, fill=float("nan")):
    """gsm_critic_eval_bwd called directly; a dict of dw1, db1, dw2, db2, dx, status."""
    lib = _lib.load()
    B, N, F = x.shape
    xk, stride = policy._rows(x)
    ws = head._weights()
    n = C.c_int64()
    assert lib.gsm_critic_backward_work_floats(F, head.hidden, head.n_out, C.byref(n)) == 0
    work = torch.full((n.value,), fill, dtype=torch.float32, device=DEV)
    dw1, db1, dw2, db2 = (torch.full_like(t, fill) for t in ws)
    dx = torch.full((B, N, F), fill, dtype=torch.float32, device=DEV) if want_dx else None
    status = torch.zeros(1, dtype=torch.int32, device=DEV)
    P = policy._ptr
    rc = lib.gsm_critic_eval_bwd(P(g), P(xk) if B else None, stride, P(n_valid), *(P(t) for t in ws), B, N, F,
                                 head.hidden, head.n_out, P(work), P(dw1), P(db1), P(dw2), P(db2),
                                 P(dx) if B else None, P(status), policy._stream(torch.device(DEV)))
    assert rc == 0, _lib.last_error(lib)
    return dict(dw1=dw1, db1=db1, dw2=dw2, db2=db2, dx=dx, status=status)


def _ref_bwd(head, x, g, n_valid=None):
    """fp64 autograd of the restatement, and 1 + sum |terms| of every gradient entry."""
    B, N, F = x.shape
    xd = x.double().clone().requires_grad_()
    ws = [t.clone().requires_grad_() for t in w64(head)]
    v = policy.critic_values_ref(xd, *ws, n_valid)
    grads = dict(zip(("dw1", "db1", "dw2", "db2", "dx"), torch.autograd.grad((v * g.double()).sum(), ws + [xd])))
    with torch.no_grad():
        w1, b1, w2, b2 = w64(head)
        mask = policy._critic_mask(x, n_valid)
        m = mask[..., None].double() if mask is not None else torch.ones(B, N, 1, dtype=torch.float64, device=DEV)
        x0 = torch.where(m > 0, x.double(), torch.zeros((), dtype=torch.float64, device=DEV))
        n = m.sum(1).clamp(min=1)                                 # [B, 1]
        pool = x0.sum(1) / n
        h = torch.relu((pool @ w1[:, :F].t() + b1)[:, None, :] + x0 @ w1[:, F:].t()) * m
        dv = g.double().permute(1, 2, 0).abs() * m
        dh = (dv @ w2.abs()) * (h > 0)
        s, apool = dh.sum(1), x0.abs().sum(1) / n
        scale = {"db2": 1 + dv.sum((0, 1)), "dw2": 1 + torch.einsum("bno,bnh->oh", dv, h),
                 "db1": 1 + dh.sum((0, 1)),
                 "dw1": 1 + torch.cat([s.t() @ apool, torch.einsum("bnh,bnf->hf", dh, x0.abs())], 1),
                 "dx": 1 + dh @ w1[:, F:].abs() + ((s @ w1[:, :F].abs()) / n)[:, None, :]}
    return grads, scale


def check_grads(got, head, x, g, n_valid=None, names=("dw1", "db1", "dw2", "db2", "dx")):
    ref, scale = _ref_bwd(head, x, g, n_valid)
    for name in names:
        e = float(((got[name].double().reshape(ref[name].shape) - ref[name]).abs() / scale[name]).max())
        print(f"{name}: worst err / (1 + sum|terms|) = {e:.3e}")
        assert e <= BOUND, name


BWD_SHAPES = [(7, 3), (171, 24), (5, 96), (300, 1)]


@pytest.mark.parametrize("B,N", BWD_SHAPES, ids=[f"B{b}-N{n}" for b, n in BWD_SHAPES])
@pytest.mark.parametrize("F,hidden,O", HEADS, ids=ids_h)
def test_backward_against_fp64_autograd(F, hidden, O, B, N):
    head, x = make_head(F, hidden, O), make_x(B, N, F)
    g = torch.randn(O, B, N, device=DEV, generator=torch.Generator(device=DEV).manual_seed(3))
    got = _bwd(head, x, g)
    assert int(got["status"].item()) == 0
    check_grads(got, head, x, g)
    again = _bwd(head, x, g)                 # bitwise reproducible
    for k in ("dw1", "db1", "dw2", "db2", "dx"):
        assert torch.equal(bits(again[k]), bits(got[k])), k
    no = _bwd(head, x, g, want_dx=False)     # dx = NULL: not wanted
    assert no["dx"] is None
    for k in ("dw1", "db1", "dw2", "db2"):
        assert torch.equal(bits(no[k]), bits(got[k])), k
    n_valid = make_counts(B, N)
    xr = x.clone()
    xr[torch.arange(N, device=DEV)[None, :] >= n_valid[:, None]] = float("nan")
    rag = _bwd(head, xr, g, n_valid)
    assert int(rag["status"].item()) == 0
    check_grads(rag, head, xr, g, n_valid)


@pytest.mark.parametrize("ragged", [False, True])
def test_backward_past_one_grid_of_tiles(ragged):
    """More tiles than the backward's capped grid (512 tiles of 64 envs at one
    agent): the workgroups add several tiles to their partial."""
    B, N, F, hidden, O = BWD_GRID * 64 + 1000, 1, 8, 16, 2
    head, x = make_head(F, hidden, O), make_x(B, N, F)
    g = torch.randn(O, B, N, device=DEV, generator=torch.Generator(device=DEV).manual_seed(4))
    n_valid = make_counts(B, N) if ragged else None
    check_grads(_bwd(head, x, g, n_valid), head, x, g, n_valid)


def test_backward_of_no_envs_is_zeros():
    head = make_head(48, 64, 2)
    got = _bwd(head, torch.zeros(0, 3, 48, device=DEV), torch.zeros(2, 0, 3, device=DEV))
    for k in ("dw1", "db1", "dw2", "db2"):
        assert (got[k] == 0).all(), k
    assert fwd(head, torch.zeros(0, 3, 48, device=DEV)).shape == (2, 0, 3)


def test_backward_pool_path_alone():
    """With the x half of W1 zero a row's value depends on its env's pool
    alone, so dx is the same for every valid row of an env."""
    B, N, F = 40, 5, 48
    head, x = make_head(F, 64, 2), make_x(B, N, F)
    with torch.no_grad():
        head.lin1.weight[:, F:] = 0
    n_valid = make_counts(B, N)
    g = torch.randn(2, B, N, device=DEV, generator=torch.Generator(device=DEV).manual_seed(5))
    got = _bwd(head, x, g, n_valid)
    check_grads(got, head, x, g, n_valid)
    dx = got["dx"]
    assert float(dx.abs().sum()) > 0
    for b in range(B):
        n = int(n_valid[b])
        assert torch.equal(bits(dx[b, :n]), bits(dx[b, :1].expand(n, F))), b
        assert (dx[b, n:] == 0).all()


@pytest.mark.parametrize("F,hidden,O", [(48, 64, 2), (52, 32, 2), (4, 16, 1)])
def test_module_backward_puts_the_kernel_gradients_on_the_parameters(F, hidden, O):
    B, N = 171, 6
    head, x = make_head(F, hidden, O, kernel_backward=True), make_x(B, N, F)
    x = x.requires_grad_()
    n_valid = make_counts(B, N)
    g = torch.randn(O, B, N, device=DEV, generator=torch.Generator(device=DEV).manual_seed(6))
    v = head(x, n_valid)
    assert v.grad_fn is not None and "CriticEval" in type(v.grad_fn).__name__
    assert torch.equal(bits(v.detach()), bits(fwd(head, x.detach(), n_valid)))
    (v * g).sum().backward()
    want = _bwd(head, x.detach(), g, n_valid)
    assert torch.equal(bits(head.lin1.weight.grad), bits(want["dw1"]))
    assert torch.equal(bits(head.lin1.bias.grad), bits(want["db1"]))
    assert torch.equal(bits(head.lin2.weight.grad), bits(want["dw2"]))
    assert torch.equal(bits(head.lin2.bias.grad), bits(want["db2"]))
    assert torch.equal(bits(x.grad), bits(want["dx"]))
    # with denorm the training path returns the kernel's denormalised bits (applied in torch)
    st = torch.tensor([[0.5, 3.0], [-2.0, 0.25]], device=DEV)[:O].contiguous()
    assert torch.equal(bits(head(x, n_valid, st).detach()), bits(fwd(head, x.detach(), n_valid, st)))
    # without kernel_backward the torch formulation trains, to the same gradients within the bound
    slow = make_head(F, hidden, O)
    slow.load_state_dict(head.state_dict())
    vs = slow(x.detach(), n_valid)
    assert "CriticEval" not in type(vs.grad_fn).__name__
    (vs * g).sum().backward()
    assert torch.allclose(slow.lin1.weight.grad, want["dw1"], rtol=1e-3, atol=1e-3)


def test_gradient_reaches_the_conv_through_forward_env():
    B, N = 64, 3
    env = GpuBatchEnv(EnvConfig(n_envs=B, n_agents=N, seed=3), DEV)
    out = env.reset(seed=3)
    torch.manual_seed(0)
    conv = TransformerConv(7, 16, heads=2, kernel_backward=True).to(DEV)
    head = make_head(32, 16, 2, kernel_backward=True)
    feats = conv.forward_env(out, rows="agents", n_agents=N)
    assert feats.shape == (B, N, 32) and feats.requires_grad
    v = head(feats)
    assert "CriticEval" in type(v.grad_fn).__name__
    (v[0].sum() + 0.5 * v[1].sum()).backward()
    for lin in (conv.lin_query, conv.lin_key, conv.lin_value, conv.lin_skip):
        assert lin.weight.grad is not None and torch.isfinite(lin.weight.grad).all()
        assert float(lin.weight.grad.abs().sum()) > 0
    assert float(head.lin1.weight.grad[:, :32].abs().sum()) > 0
    env.close()


def test_status_nonfinite_row_and_bad_count():
    B, N = 171, 6
    head, x = make_head(48, 64, 2), make_x(B, N, 48)
    clean = fwd(head, x)
    assert int(head.status.item()) == 0
    bad = x.clone()
    bad[100, 2, 7] = float("nan")
    got = fwd(head, bad)
    assert int(head.status.item()) == _lib.CRITIC_NONFINITE
    assert torch.isnan(got[:, 100]).all()            # written; through the pool the whole env
    keep = torch.ones(B, dtype=torch.bool, device=DEV)
    keep[100] = False
    assert torch.equal(bits(got)[:, keep], bits(clean)[:, keep])
    # a NaN in a padded row is no finding
    n_valid = torch.full((B,), N, dtype=torch.int32, device=DEV)
    n_valid[100] = 2
    fwd(head, bad, n_valid)
    assert int(head.status.item()) == 0
    # counts out of range are clamped to [0, N]
    n_bad = n_valid.clone()
    n_bad[5], n_bad[6] = N + 3, -1
    n_clamped = n_valid.clone()
    n_clamped[5], n_clamped[6] = N, 0
    got = fwd(head, bad, n_bad)
    assert int(head.status.item()) == _lib.CRITIC_BAD_COUNT
    assert torch.equal(bits(got), bits(fwd(head, bad, n_clamped)))
    assert (got[:, 6] == 0).all()
    g = torch.randn(2, B, N, device=DEV)
    assert int(_bwd(head, bad, g, n_bad)["status"].item()) == _lib.CRITIC_BAD_COUNT


def test_captured_forward_replays_with_updated_inputs_and_statistics():
    B, N = 171, 6
    head = make_head(48, 64, 2)
    x, st = make_x(B, N, 48), torch.tensor([[0.5, 3.0], [-2.0, 0.25]], device=DEV)
    side = torch.cuda.Stream(device=DEV)
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        fwd(head, x, denorm=st)                       # warm the kernel
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = fwd(head, x, denorm=st)
    x.copy_(make_x(B, N, 48, seed=11))
    graph.replay()
    first = out.clone()
    st.copy_(torch.tensor([[1.5, 0.75], [-4.0, 2.0]], device=DEV))
    graph.replay()
    second = out.clone()
    torch.cuda.synchronize()
    del graph
    st_old = torch.tensor([[0.5, 3.0], [-2.0, 0.25]], device=DEV)
    assert torch.equal(bits(first), bits(fwd(head, x, denorm=st_old)))
    assert torch.equal(bits(second), bits(fwd(head, x, denorm=st)))
    assert not torch.equal(bits(first), bits(second))


def test_end_to_end_buffer_conv_critic_returns():
    """Slots of a rollout buffer -> forward_env -> one CriticHead call over
    all (T+1) * B stored envs -> GAE for both critics."""
    B, N, T = 8, 6, 4
    env = GpuBatchEnv(EnvConfig(n_envs=B, n_agents=N, seed=5, episode_length=T), DEV)
    buf = GraphRolloutBuffer(env)
    buf.reset(seed=5)
    g = torch.Generator(device=DEV).manual_seed(8)
    for _ in range(T):
        buf.insert(torch.randint(0, 5, (B, N), device=DEV, generator=g, dtype=torch.int32))
    torch.manual_seed(0)
    conv = TransformerConv(7, 16, heads=3).to(DEV)
    head = make_head(48, 64, 2)
    with torch.no_grad():
        feats = torch.cat([conv.forward_env(buf.slot(t), rows="agents", n_agents=N) for t in range(T + 1)])
        assert feats.shape == ((T + 1) * B, N, 48)
        values = head(feats).view(2, T + 1, B, N)
    assert int(head.status.item()) == 0
    check_values(values.view(2, -1, N), head, feats)
    for which, v in (("reward", values[0]), ("cost", values[1])):
        assert v.is_contiguous()
        ret = buf.compute_returns(v, which=which, kernel=True)
        assert ret.shape == (T, B, N) and torch.isfinite(ret).all()
        assert torch.equal(bits(ret), bits(buf.compute_returns(v, which=which)))
    env.close()
