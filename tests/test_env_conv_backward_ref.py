"""CPU checks of the fused first layer's backward, torch side and host side:
gnn.env_conv_bwd_ref (the written-out weight gradients the HIP backward is
written against) against autograd of gnn.env_conv_ref in fp64, the host-only
argument checks of gsm_env_conv_fwd / gsm_env_conv_bwd /
gsm_env_conv_backward_work_floats, and forward_env(kernel_backward=True)
keeping the torch fallback off the GPU."""
import ctypes as C

import numpy as np
import pytest
import torch

from gsmarl_amd import _lib, gnn
from test_env_conv_ref import B, E, N, _graph

OPTS = [(True, True), (False, False), (True, False), (False, True)]


def _oracle_graph():
    """One env graph of the CPU oracle at 6 agents: E = 18 entities."""
    from oracle import batch_ref as br
    cfg = br.make_cfg(n_envs=1, n_agents=6, seed=2)
    st = br.new_state(cfg, seed=2, dtype=np.float64)
    ptr, ei, attr = br.edges(cfg, st["pos"], np.float64)
    n_ent = st["pos"].shape[1]
    gen = torch.Generator().manual_seed(9)
    nf = torch.randn(1, n_ent, 7, generator=gen, dtype=torch.float64)
    return dict(node_feat=nf, edge_ptr=torch.from_numpy(np.asarray(ptr, np.int64)),
                edge_index=torch.from_numpy(np.asarray(ei, np.int32)),
                edge_attr=torch.from_numpy(np.asarray(attr, np.float64)).reshape(-1)), 6


def _check(gr, rows_out, skip, edge, heads=3, Cc=4):
    nf = gr["node_feat"]
    HC = heads * Cc
    gen = torch.Generator().manual_seed(3)
    w = torch.randn(4 if skip else 3, HC, 8, generator=gen, dtype=torch.float64).requires_grad_(True)
    w_e = torch.randn(HC, generator=gen, dtype=torch.float64).requires_grad_(True) if edge else None
    g = torch.randn(nf.shape[0], rows_out, HC, generator=gen, dtype=torch.float64)
    args = (nf, gr["edge_ptr"], gr["edge_index"], gr["edge_attr"])
    out = gnn.env_conv_ref(*args, w, w_e, heads, rows_out, skip)
    want = torch.autograd.grad(out, [w] + ([w_e] if edge else []), g)
    with torch.no_grad():
        dw, dw_e = gnn.env_conv_bwd_ref(g, *args, w, w_e, heads, rows_out, skip)
        _, _, nodes = gnn.env_conv_bwd_ref(g, *args, w, w_e, heads, rows_out, skip, node_grads=True)
    assert dw.shape == w.shape and dw.dtype == torch.float64
    assert float((dw - want[0]).abs().max()) <= 1e-10
    if edge:
        assert dw_e.shape == (HC,) and float((dw_e - want[1]).abs().max()) <= 1e-10
    else:
        assert dw_e is None
    n = nf.shape[0] * nf.shape[1]
    assert len(nodes) == 4 and all(d.shape == (n, HC) for d in nodes)
    return dw, nodes


@pytest.mark.parametrize("skip,edge", OPTS)
@pytest.mark.parametrize("rows_out", [E, N])
def test_bwd_ref_matches_autograd_two_env_graph(rows_out, skip, edge):
    gr = _graph()
    dw, (dq, dk, dv, g) = _check(gr, rows_out, skip, edge)
    # the padding row (zero features, no edges) reaches the bias column of W_skip only
    pad = 0 * E + 4
    assert torch.count_nonzero(dq[pad]) == 0 and torch.count_nonzero(dk[pad]) == 0
    assert torch.count_nonzero(dq[2]) == 0                    # the empty row
    if rows_out == N:
        assert torch.count_nonzero(g.view(B, E, -1)[:, N:]) == 0


@pytest.mark.parametrize("skip,edge", OPTS)
@pytest.mark.parametrize("agents_only", [False, True])
def test_bwd_ref_matches_autograd_oracle_graph(agents_only, skip, edge):
    gr, n_agents = _oracle_graph()
    n_ent = gr["node_feat"].shape[1]
    assert n_ent == 18 and int(gr["edge_ptr"][-1]) > 0
    _check(gr, n_agents if agents_only else n_ent, skip, edge)


def test_bwd_ref_fp32_and_rejects_bad_w():
    gr = _graph(torch.float32)
    w, w_e, g = torch.randn(4, 12, 8), torch.randn(12), torch.randn(B, E, 12)
    args = (gr["node_feat"], gr["edge_ptr"], gr["edge_index"], gr["edge_attr"])
    dw, dw_e = gnn.env_conv_bwd_ref(g, *args, w, w_e, 3, E, True)
    assert dw.dtype == torch.float32 and dw_e.dtype == torch.float32
    with pytest.raises(ValueError):
        gnn.env_conv_bwd_ref(g, *args, w[:3], w_e, 3, E, True)


def test_abi_argument_checks_host_only():
    """The workspace size and the shape and pointer checks touch no GPU."""
    lib = _lib.load()
    nf = C.c_int64()
    ok = (8192, 72, 1 << 20, 3, 16, _lib.CONV_SKIP)
    assert lib.gsm_env_conv_backward_work_floats(*ok, C.byref(nf)) == _lib.GSM_OK
    assert nf.value >= 2 * (1 << 20) * 3 + 4 * 48 * 8 + 48    # a_ij, ds_ij per (entry, head) + one partial
    a = C.c_void_p(4096)                                     # never dereferenced: the checks fail first
    bads = ((8192, 72, 1 << 20, 1, 48, 0), (8192, 72, 1 << 20, 2, 64, 0), (8192, 289, 1 << 20, 3, 16, 0),
            (8192, 0, 1 << 20, 3, 16, 0), (-1, 72, 0, 3, 16, 0), (1 << 26, 72, 0, 3, 16, 0),
            (8192, 72, 1 << 31, 3, 16, 0), (8192, 72, -1, 3, 16, 0), (8192, 72, 1 << 20, 3, 16, 2))
    for n_envs, n_ent, limit, heads, ch, flags in bads:
        bad = (n_envs, n_ent, limit, heads, ch, flags)
        assert lib.gsm_env_conv_backward_work_floats(*bad, C.byref(nf)) == _lib.GSM_EINVAL, bad
        assert lib.gsm_env_conv_bwd(a, a, a, a, limit, a, limit, a, a, a, a, n_envs, n_ent, heads, ch, 1.0, flags, 1,
                                    a, a, a, a, None) == _lib.GSM_EINVAL, bad
        assert lib.gsm_env_conv_fwd(a, a, a, limit, a, limit, a, a, n_envs, n_ent, heads, ch, 1.0, flags, 1, a, a,
                                    None, a, None) == _lib.GSM_EINVAL, bad
    assert lib.gsm_env_conv_backward_work_floats(*ok, None) == _lib.GSM_EINVAL
    shape = (4, 9, 3, 16, 1.0, _lib.CONV_SKIP)
    # n_rows_out outside [1, E]; a row stride below the entry bound
    assert lib.gsm_env_conv_bwd(a, a, a, a, 16, a, 16, a, a, a, a, *shape, 10, a, a, a, a, None) == _lib.GSM_EINVAL
    assert lib.gsm_env_conv_bwd(a, a, a, a, 8, a, 16, a, a, a, a, *shape, 9, a, a, a, a, None) == _lib.GSM_EINVAL
    # required pointers, each NULL in turn, are checked before any launch
    names = ["grad_out", "node_feat", "edge_ptr", "edge_index", "edge_attr", "w", "out", "lse", "work", "dw",
             "status"]
    for miss in names:
        v = {k: (None if k == miss else a) for k in names}
        rc = lib.gsm_env_conv_bwd(v["grad_out"], v["node_feat"], v["edge_ptr"], v["edge_index"], 16, v["edge_attr"],
                                  16, v["w"], a, v["out"], v["lse"], *shape, 9, v["work"], v["dw"], a, v["status"],
                                  None)
        assert rc == _lib.GSM_EINVAL, miss
        assert "NULL" in _lib.last_error(lib), miss
    # dw_e without w_e
    assert lib.gsm_env_conv_bwd(a, a, a, a, 16, a, 16, a, None, a, a, *shape, 9, a, a, a, a, None) == _lib.GSM_EINVAL
    # the forward with statistics needs lse, out and status
    for miss in ("out", "lse", "status"):
        v = {k: (None if k == miss else a) for k in ("out", "lse", "status")}
        assert lib.gsm_env_conv_fwd(a, a, a, 16, a, 16, a, a, *shape, 9, v["out"], v["lse"], None, v["status"],
                                    None) == _lib.GSM_EINVAL, miss


@pytest.mark.parametrize("root_weight,edge_dim", [(True, 1), (False, None)])
def test_forward_env_kernel_backward_falls_back_on_cpu(root_weight, edge_dim):
    """Off the GPU the flag changes nothing: the same torch path, the same
    gradients bit for bit."""
    gr = _graph(torch.float32)
    torch.manual_seed(1)
    conv_k = gnn.TransformerConv(7, 4, heads=3, edge_dim=edge_dim, root_weight=root_weight, kernel_backward=True)
    conv_t = gnn.TransformerConv(7, 4, heads=3, edge_dim=edge_dim, root_weight=root_weight)
    conv_t.load_state_dict(conv_k.state_dict())
    outs = []
    for conv in (conv_k, conv_t):
        out = conv.forward_env(gr, rows="agents", n_agents=N)
        assert "EnvConv" not in type(out.grad_fn).__name__
        out.square().sum().backward()
        outs.append(out.detach())
    assert torch.equal(outs[0], outs[1])
    for (name, a), (_, b) in zip(conv_k.named_parameters(), conv_t.named_parameters()):
        assert a.grad is not None and torch.equal(a.grad, b.grad), name


def test_autograd_entry_needs_a_gpu_and_no_env_gradients():
    gr = _graph(torch.float32)
    w, w_e = torch.randn(4, 12, 8, requires_grad=True), torch.randn(12)
    args = (gr["node_feat"], gr["edge_ptr"], gr["edge_index"], gr["edge_attr"])
    with pytest.raises(_lib.GsmError):
        gnn.env_conv_autograd(*args, w, w_e, 3, E, True)
    with pytest.raises(ValueError):
        gnn.env_conv_autograd(gr["node_feat"].clone().requires_grad_(True), *args[1:], w, w_e, 3, E, True)
