"""Guard bands around the fused first GNN layer (gsm_env_conv through
gnn.env_conv, gsm_env_conv_fwd and gsm_env_conv_bwd through
gnn.env_conv_autograd): the five assertions of tests/guard.py on the graphs of
test_gpu_env_conv.py and test_gpu_env_conv_backward.py.

Graphs: n3 (E = 9, seven envs a workgroup, a partial last group), n24, n96
(E = 288: the recompute form at 3 x 16), mixed (padded rows), capped (more env
groups than the backward's grid), each with that file's four (skip, edge,
rows) options, rows "all" also asking for row_ptr_out; 3 x 16 takes the float4
kernels and 1 x 1 the scalar ones. The edge arrays are the env's unsliced
ones, longer than the total. `slot` is a graph as a rollout-buffer slot view
gives it: edge_index [:, :total] of rows `cap` apart, so that what lies past
the total in either row is band.

Inputs under guard: node_feat, edge_attr, w, w_e, grad_out (floats), edge_ptr
(offsets), edge_index (node ids 0 / B*E-1). Outputs under guard through the
wrappers' own torch.empty: out, row_ptr_out, lse, dw, dw_e and the workspace.

Exceptions of (b): none for the outputs. include/gsm.h: "an empty row gives
skip_i, or exactly 0 without skip", "an empty row, or a row of an env treated
as edgeless, stores 0" (lse), row_ptr_out "[n_envs*n_entities+1]": every row,
padded ones included, is written. The workspace
(gsm_env_conv_backward_work_floats: "a_ij and ds_ij per entry position and
head, and one partial per workgroup") is sized by edge_limit and the grid cap;
it is exempt from (b) as a whole, wherever the unwritten elements lie (past the
graph's total inside each region, past the launch's workgroups). It has to be
allocated under guard, so (a) holds for it, and what it held before must not
reach an output (e)."""
import pytest
import torch

import guard as G
import test_gpu_env_conv_backward as bwd
from gsmarl_amd import _lib, gnn

pytestmark = pytest.mark.gpu
KINDS = ["n3", "n24", "n96", "mixed"]
HEADS = [(3, 16), (1, 1)]


def _inputs(g, w, w_e, go, slot=False):
    n, total = g["B"] * g["E"], g["total"]
    ei, ea = g["edge_index"], g["edge_attr"].reshape(-1)
    ids = lambda f: G.ids(f, n)
    if slot:
        edge_index = G.In(ei[:, :total], ids, base_shape=tuple(ei.shape), view=lambda t: t[:, :total])
        edge_attr = G.In(ea[:total].contiguous(), G.floats)
    else:
        edge_index, edge_attr = G.In(ei, ids), G.In(ea, G.floats)
    return dict(node_feat=G.In(g["node_feat"], G.floats),
                edge_ptr=G.In(g["edge_ptr"], lambda f: G.offsets(f, g["edge_ptr"])), edge_index=edge_index,
                edge_attr=edge_attr, w=G.In(w, G.floats), w_e=G.In(w_e, G.floats) if w_e is not None else None,
                go=G.In(go, G.floats) if go is not None else None)


def _call(heads, R, skip, want_ptr, want_dwe=True):
    def call(node_feat, edge_ptr, edge_index, edge_attr, w, w_e, go):
        if go is None:
            res = gnn.env_conv(node_feat, edge_ptr, edge_index, edge_attr, w, w_e, heads, R, skip, row_ptr=want_ptr)
            out, ptr = res if want_ptr else (res, None)
            return dict(out=out, row_ptr=ptr)
        wl = w.detach().requires_grad_(True)
        wel = w_e.detach().requires_grad_(want_dwe) if w_e is not None else None
        res = gnn.env_conv_autograd(node_feat, edge_ptr, edge_index, edge_attr, wl, wel, heads, R, skip,
                                    row_ptr=want_ptr)
        out, ptr = res if want_ptr else (res, None)
        grads = torch.autograd.grad(out, [wl] + ([wel] if wel is not None and want_dwe else []), go)
        return dict(out=out.detach(), row_ptr=ptr, dw=grads[0], dw_e=grads[1] if len(grads) > 1 else None)
    return call


def _run(kind, heads, C, backward, opts=bwd.OPTS, slot=False):
    g = bwd._get(kind)
    limit = g["total"] if slot else g["edge_index"].shape[1]
    for skip, edge, rows in opts:
        R = g["E"] if rows == "all" else g["N"]
        w, w_e = bwd._weights(heads, C, skip, edge, seed=heads * 100 + C)
        go = bwd._grad_out(g, R, heads * C) if backward else None
        work = (_lib.work_floats("gsm_env_conv_backward_work_floats", g["B"], g["E"], limit, heads, C,
                                 _lib.CONV_SKIP if skip else 0),)
        plain = G.run_case(_call(heads, R, skip, rows == "all"), _inputs(g, w, w_e, go, slot),
                           work=[work] if backward else [])
        assert plain["out"].shape == (g["B"], R, heads * C) and (plain["row_ptr"] is not None) == (rows == "all")


@pytest.mark.parametrize("heads,C", HEADS)
@pytest.mark.parametrize("kind", KINDS)
def test_env_conv_forward(kind, heads, C):
    """gsm_env_conv."""
    _run(kind, heads, C, backward=False)


@pytest.mark.parametrize("heads,C", HEADS)
@pytest.mark.parametrize("kind", KINDS)
def test_env_conv_forward_backward(kind, heads, C):
    """gsm_env_conv_fwd and gsm_env_conv_bwd."""
    _run(kind, heads, C, backward=True)


@pytest.mark.parametrize("backward", [False, True], ids=["forward", "backward"])
def test_env_conv_past_the_grid_cap(backward):
    _run("capped", 3, 16, backward, opts=bwd.OPTS[:2])


@pytest.mark.parametrize("backward", [False, True], ids=["forward", "backward"])
@pytest.mark.parametrize("kind", ["n3", "n24"])
def test_env_conv_on_a_slot_view(kind, backward):
    _run(kind, 3, 16, backward, opts=bwd.OPTS[:2], slot=True)


@pytest.mark.parametrize("kind", ["n3", "n96"])
def test_env_conv_backward_without_dw_e(kind):
    """dw_e "or NULL (not wanted; it needs w_e)": the edge term is used and its gradient is not written."""
    g = bwd._get(kind)
    heads, C, R = 3, 16, g["E"]
    w, w_e = bwd._weights(heads, C, True, True, seed=316)
    go = bwd._grad_out(g, R, heads * C)
    work = (_lib.work_floats("gsm_env_conv_backward_work_floats", g["B"], g["E"], g["edge_index"].shape[1], heads, C,
                             _lib.CONV_SKIP),)
    ins = _inputs(g, w, w_e, go)
    full = G.run_case(_call(heads, R, True, False), ins, work=[work])
    plain = G.run_case(_call(heads, R, True, False, want_dwe=False), ins, work=[work])
    assert plain["dw_e"] is None and full["dw_e"] is not None and G.same_bits(plain["dw"], full["dw"])
