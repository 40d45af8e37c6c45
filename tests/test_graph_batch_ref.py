"""Minibatch assembly, the parts that need no GPU: on the oracle's env graphs
the sort-free transposed CSR (gnn.csr_transpose_symmetric: t_ptr = row_ptr,
t_tgt = col, t_edge by one search in the sorted rows) equals gnn.csr_transpose
element for element, a missing reverse entry is reported with every index in
range, and the new C entry points reject bad arguments on the host."""
import ctypes as C

import numpy as np
import pytest
import torch


def _nav_graph(n_agents, n_envs, seed=3):
    from oracle import batch_ref as br
    cfg = br.make_cfg(n_agents=n_agents, n_envs=n_envs, seed=seed)
    st = br.new_state(cfg, seed=seed, dtype=np.float32)
    _, ei, _ = br.edges(cfg, st["pos"], np.float32)
    return ei, n_envs * br.Spec(cfg, np.float32).E


def _ragged_graph(scenario, n_agents, n_envs, seed=4):
    from oracle import ragged_ref as rr
    cfg = rr.make_cfg(scenario=scenario, n_agents=n_agents, n_envs=n_envs, seed=seed)
    ob = rr.observe(cfg, rr.new_state(cfg))
    return ob["edge_index"], n_envs * rr.RSpec(cfg).Emax


GRAPHS = {
    "nav3x5": lambda: _nav_graph(3, 5), "nav6x7": lambda: _nav_graph(6, 7), "nav24x4": lambda: _nav_graph(24, 4),
    "mixed12x12": lambda: _ragged_graph("mixed", 12, 12), "polygon5x4": lambda: _ragged_graph("polygon", 5, 4),
    "line6x4": lambda: _ragged_graph("line", 6, 4),
}


def _csr(ei, n):
    from gsmarl_amd import gnn
    ei = torch.from_numpy(np.ascontiguousarray(ei))
    return gnn.env_csr(ei, n), ei[1].contiguous()


@pytest.mark.parametrize("name", sorted(GRAPHS))
def test_symmetric_transpose_equals_sorted_transpose(name):
    from gsmarl_amd import gnn
    ei, n = GRAPHS[name]()
    assert ei.shape[1] > 0
    row_ptr, col = _csr(ei, n)
    if name == "mixed12x12":      # padded nodes: rows without entries
        assert int((row_ptr[1:] == row_ptr[:-1]).sum()) > 0
    t_ptr, t_edge, t_tgt = gnn.csr_transpose(row_ptr, col)
    s_ptr, s_edge, s_tgt, ok = gnn.csr_transpose_symmetric(row_ptr, col)
    assert ok.dtype == torch.bool and bool(ok.all())
    assert s_ptr.dtype == t_ptr.dtype and torch.equal(s_ptr, t_ptr)
    assert s_edge.dtype == t_edge.dtype and torch.equal(s_edge, t_edge)
    assert s_tgt.dtype == t_tgt.dtype and torch.equal(s_tgt, t_tgt)


@pytest.mark.parametrize("name", ["nav3x5", "nav24x4", "mixed12x12"])
@pytest.mark.parametrize("where", ["first", "middle", "last"])
def test_dropped_entry_is_reported_and_indices_stay_in_range(name, where):
    from gsmarl_amd import gnn
    ei, n = GRAPHS[name]()
    nE = ei.shape[1]
    drop = {"first": 0, "middle": nE // 2, "last": nE - 1}[where]
    ei = np.delete(ei, drop, axis=1)
    row_ptr, col = _csr(ei, n)
    s_ptr, s_edge, s_tgt, ok = gnn.csr_transpose_symmetric(row_ptr, col)
    assert not bool(ok.all())
    assert int((~ok).sum()) == 1                       # the dropped entry's partner
    assert s_edge.numel() == nE - 1 and int(s_edge.min()) >= 0 and int(s_edge.max()) < nE - 1
    assert int(s_tgt.min()) >= 0 and int(s_tgt.max()) < n
    assert torch.equal(s_ptr, row_ptr)


@pytest.mark.parametrize("n", [0, 1, 9])
def test_no_edges(n):
    from gsmarl_amd import gnn
    row_ptr = torch.zeros(n + 1, dtype=torch.int64)
    col = torch.zeros(0, dtype=torch.int32)
    ref = gnn.csr_transpose(row_ptr, col)
    got = gnn.csr_transpose_symmetric(row_ptr, col)
    for r, g in zip(ref, got[:3]):
        assert g.shape == r.shape and g.dtype == r.dtype and torch.equal(g, r)
    assert got[3].dtype == torch.bool and got[3].numel() == 0 and bool(got[3].all())


@pytest.fixture(scope="module")
def lib():
    from gsmarl_amd import _lib
    if not _lib.LIB_PATH.exists():
        import __graft_entry__ as g
        g.build()
    return _lib.load()


def test_entry_points_reject_bad_arguments_on_the_host(lib):
    """Every call below fails its argument check before any HIP call (fake
    non-NULL pointers are never dereferenced on the host)."""
    from gsmarl_amd import _lib
    p = C.c_void_p(4096)
    E = _lib.GSM_EINVAL
    # gsm_graph_batch_ptr(edge_ptr, S, B, cap, t_idx, b_idx, K, sample_ptr, status, stream)
    assert lib.gsm_graph_batch_ptr(p, 4, 8, 64, p, p, -1, p, p, None) == E
    assert "n_samples" in _lib.last_error(lib)
    assert lib.gsm_graph_batch_ptr(p, 4, 8, 64, p, p, 5, None, p, None) == E
    assert lib.gsm_graph_batch_ptr(p, 4, 8, 64, p, p, 5, p, None, None) == E
    assert lib.gsm_graph_batch_ptr(None, 4, 8, 64, p, p, 5, p, p, None) == E
    assert lib.gsm_graph_batch_ptr(p, 4, 8, 64, None, p, 5, p, p, None) == E
    assert lib.gsm_graph_batch_ptr(p, 0, 8, 64, p, p, 5, p, p, None) == E
    assert lib.gsm_graph_batch_ptr(p, 4, 0, 64, p, p, 5, p, p, None) == E
    assert lib.gsm_graph_batch_ptr(p, 4, 8, -1, p, p, 5, p, p, None) == E

    def gather(K=5, nE=10, E_=9, nf=p, row=p, col=p, attr=p, status=p, node_in=p):
        return lib.gsm_graph_batch_gather(node_in, p, p, p, 4, 8, E_, 64, p, p, p, K, nE, nf, row, col, attr, p,
                                          status, None)
    assert gather(K=-1) == E
    assert gather(nE=-1) == E
    assert gather(nE=1 << 31) == E
    assert gather(E_=0) == E
    assert gather(K=1 << 30, E_=9) == E                 # K*E >= 2^31
    assert gather(nf=None) == E
    assert gather(row=None) == E
    assert gather(col=None) == E
    assert gather(attr=None) == E
    assert gather(status=None) == E
    assert gather(node_in=None) == E
    assert gather(K=0, nE=3) == E
    assert "edges without samples" in _lib.last_error(lib)
    # gsm_gae(reward, value, done, T, B, N, gamma, gamma_lambda, ret, stream)
    assert lib.gsm_gae(p, p, p, 0, 8, 3, 0.99, 0.94, p, None) == E
    assert "n_steps" in _lib.last_error(lib)
    assert lib.gsm_gae(p, p, p, -3, 8, 3, 0.99, 0.94, p, None) == E
    assert lib.gsm_gae(p, p, p, 5, 0, 3, 0.99, 0.94, p, None) == E
    assert lib.gsm_gae(p, p, p, 5, 8, 0, 0.99, 0.94, p, None) == E
    assert lib.gsm_gae(p, p, p, 5, 8, 3, 0.99, 0.94, None, None) == E
    assert lib.gsm_gae(None, p, p, 5, 8, 3, 0.99, 0.94, p, None) == E
