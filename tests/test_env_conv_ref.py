"""CPU checks of the fused first layer's torch side (gsmarl_amd.gnn):
pack_conv_params' layout, env_conv_ref against TransformerConv.forward on
env_csr of the same graph, the agent-row slice, the row offsets, and
forward_env's differentiable fallback."""
import pytest
import torch

from gsmarl_amd import gnn

B, E, N = 2, 5, 2


def _graph(dtype=torch.float64, feats=7):
    """Two envs of five nodes. Env 0: rows 0, 1, 3 have entries, row 2 is
    empty and row 4 is a padding row (type -1, zero features, no edges).
    Env 1: a triangle on nodes 0-2 and the pair 3-4. Global ids b*E + e,
    entries sorted by (row, col), every edge both ways."""
    g = torch.Generator().manual_seed(5)
    nf = torch.randn(B, E, feats, generator=g, dtype=dtype)
    nf[0, 4] = 0.0
    if feats == 7:
        nf[0, 4, 6] = -1.0
        nf[0, 4, :6] = 0.0
    e0 = [(0, 1), (0, 3), (1, 0), (1, 3), (3, 0), (3, 1)]
    e1 = [(0, 1), (0, 2), (1, 0), (1, 2), (2, 0), (2, 1), (3, 4), (4, 3)]
    rows = [r for r, _ in e0] + [E + r for r, _ in e1]
    cols = [c for _, c in e0] + [E + c for _, c in e1]
    ei = torch.tensor([rows, cols], dtype=torch.int32)
    ea = torch.rand(ei.shape[1], generator=g, dtype=dtype) + 0.1
    ptr = torch.tensor([0, len(e0), len(e0) + len(e1)], dtype=torch.int64)
    return dict(node_feat=nf, edge_ptr=ptr, edge_index=ei, edge_attr=ea)


@pytest.mark.parametrize("root_weight,edge_dim", [(True, 1), (False, 1), (True, None), (False, None)])
def test_pack_conv_params_round_trip(root_weight, edge_dim):
    conv = gnn.TransformerConv(7, 4, heads=3, edge_dim=edge_dim, root_weight=root_weight)
    w, w_e = gnn.pack_conv_params(conv)
    lins = [conv.lin_query, conv.lin_key, conv.lin_value] + ([conv.lin_skip] if root_weight else [])
    assert w.shape == (len(lins), 12, 8) and w.is_contiguous()
    for blk, lin in enumerate(lins):
        assert torch.equal(w[blk, :, :7], lin.weight)        # columns 0-6: the 7 features
        assert torch.equal(w[blk, :, 7], lin.bias)           # column 7: the bias
    if edge_dim is None:
        assert w_e is None
    else:
        assert w_e.shape == (12,) and torch.equal(w_e, conv.lin_edge.weight[:, 0])
    with pytest.raises(ValueError):
        gnn.pack_conv_params(gnn.TransformerConv(7, 4, heads=3, concat=False))


@pytest.mark.parametrize("root_weight,edge_dim", [(True, 1), (False, None)])
def test_ref_equals_forward_on_env_csr(root_weight, edge_dim):
    gr = _graph()
    conv = gnn.TransformerConv(7, 4, heads=3, edge_dim=edge_dim, root_weight=root_weight).double()
    w, w_e = gnn.pack_conv_params(conv)
    with torch.no_grad():
        out, ptr = gnn.env_conv_ref(gr["node_feat"], gr["edge_ptr"], gr["edge_index"], gr["edge_attr"], w, w_e, 3, E,
                                    root_weight, row_ptr=True)
        csr = gnn.env_csr(gr["edge_index"], B * E)
        ref = conv(gr["node_feat"].reshape(B * E, 7), csr, gr["edge_index"][1], gr["edge_attr"].reshape(-1, 1))
    assert out.shape == (B, E, 12)
    assert float((out.reshape(B * E, 12) - ref).abs().max()) <= 1e-12
    assert torch.equal(ptr, csr)                              # the fallback's row_ptr
    assert ptr.tolist() == [0, 2, 4, 4, 6, 6, 8, 10, 12, 13, 14]
    # the empty row and the padding row: skip alone, or exactly 0 without it
    with torch.no_grad():
        sk = conv.lin_skip(gr["node_feat"][0, [2, 4]]) if root_weight else torch.zeros(2, 12, dtype=torch.float64)
    assert float((out[0, [2, 4]] - sk).abs().max()) <= 1e-12
    if not root_weight:
        assert torch.all(out[0, [2, 4]] == 0)


def test_agent_rows_are_the_slice():
    gr = _graph()
    conv = gnn.TransformerConv(7, 4, heads=3).double()
    with torch.no_grad():
        full = conv.forward_env(gr)
        agents = conv.forward_env(gr, rows="agents", n_agents=N)
    assert full.shape == (B, E, 12) and agents.shape == (B, N, 12)
    assert torch.equal(agents, full[:, :N])
    with pytest.raises(ValueError):
        conv.forward_env(gr, rows="agents")


def test_forward_env_fallback_gradients():
    gr = _graph(torch.float32)
    conv = gnn.TransformerConv(7, 4, heads=3)
    out, ptr = conv.forward_env(gr, row_ptr=True)
    assert out.shape == (B, E, 12) and out.requires_grad
    assert torch.equal(ptr, gnn.env_csr(gr["edge_index"], B * E))
    out.square().sum().backward()
    for name, p in conv.named_parameters():
        assert p.grad is not None and torch.isfinite(p.grad).all() and p.grad.abs().sum() > 0, name


@pytest.mark.parametrize("kw,feats", [(dict(concat=False), 7), (dict(), 5), (dict(concat=False, root_weight=False), 7)])
def test_forward_env_other_layers_match_forward(kw, feats):
    gr = _graph(feats=feats)
    conv = gnn.TransformerConv(feats, 4, heads=3, **kw).double()
    with torch.no_grad():
        out = conv.forward_env(gr, rows="agents", n_agents=N)
        ref = conv(gr["node_feat"].reshape(B * E, feats), gnn.env_csr(gr["edge_index"], B * E), gr["edge_index"][1],
                   gr["edge_attr"].reshape(-1, 1))
    assert float((out - ref.view(B, E, -1)[:, :N]).abs().max()) <= 1e-12


def test_unsliced_edge_arrays_and_truncation():
    gr = _graph()
    conv = gnn.TransformerConv(7, 4, heads=3).double()
    big = dict(gr)
    big["edge_index"] = torch.cat([gr["edge_index"], torch.zeros(2, 6, dtype=torch.int32)], 1)
    big["edge_attr"] = torch.cat([gr["edge_attr"], torch.zeros(6, dtype=torch.float64)])
    with torch.no_grad():
        assert torch.equal(conv.forward_env(big), conv.forward_env(gr))
        cut = dict(gr)
        cut["edge_index"] = gr["edge_index"][:, :10]
        with pytest.raises(ValueError):
            conv.forward_env(cut)
