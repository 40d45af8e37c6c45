"""Guard bands around the attention launches (gsm_attn_aggregate,
gsm_attn_aggregate_fwd, gsm_attn_aggregate_bwd) through gnn.attn_aggregate and
gnn.attn_aggregate_autograd: the five assertions of tests/guard.py on
test_gpu_gnn_backward's planted graph (n = 1003) for every dispatched
instantiation, misaligned bases, a shape past the grid cap, and the no-edge
and one-node graphs. The values are that file's (held to fp64 there); here
only where the kernels read and write is checked, bit for bit.

Inputs under guard: q, k, v, skip, grad_out, edge_w, w_e (floats), row_ptr and
t_ptr (offsets), col and t_tgt (node ids), t_edge (entry ids). Outputs under
guard through the wrapper's own torch.empty: out, lse, dq, dk, dv, dedge_w,
dw_e and the workspace.

Exceptions of (b): none for the outputs. include/gsm.h: "dq, dk, dv: f32
[n_nodes][heads*channels], every row written", "an empty row stores 0" (lse).
The workspace (gsm_attn_backward_work_floats) is exempt from (b) as a whole,
wherever the unwritten elements lie: "a_ij and ds_ij per entry and head, and
the dw_e block partials" are written only for the entries and workgroups of
the launch (past the grid cap every partial is). It has to be allocated under
guard, so (a) holds for it, and what it held before must not reach an output
(e)."""
import pytest
import torch

import guard as G
from gsmarl_amd import _lib, gnn
from test_gnn_dispatch_ref import DISPATCH, select
from test_gpu_gnn_backward import BWD_MAX_BLOCKS, CAPPED, OPTS, _case, _groups
from test_gpu_gnn_dispatch import _run_misaligned

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FLOATS = ("q", "k", "v", "ew", "we", "sk")
GRADS = ("dq", "dk", "dv", "dedge_w", "dw_e")


def _inputs(c, transpose, misalign=()):
    n, nE = c["q"].shape[0], c["col"].numel()
    ins = {}
    for name in FLOATS + ("g",):
        if c[name] is not None and c[name].numel():
            ins[name] = G.In(c[name], G.floats, misalign=4 if name in misalign else 0)
        else:
            ins[name] = c[name]
    ins["ptr"] = G.In(c["ptr"], lambda f: G.offsets(f, c["ptr"]))
    ins["col"] = G.In(c["col"], lambda f: G.ids(f, n)) if nE else c["col"]
    if transpose is not None:
        t_ptr, t_edge, t_tgt = transpose
        ins["t_ptr"] = G.In(t_ptr, lambda f: G.offsets(f, t_ptr))
        ins["t_edge"] = G.In(t_edge, lambda f: G.ids(f, nE)) if nE else t_edge
        ins["t_tgt"] = G.In(t_tgt, lambda f: G.ids(f, n)) if nE else t_tgt
    else:
        ins["t_ptr"] = ins["t_edge"] = ins["t_tgt"] = None
    return ins


def _fwd_bwd(heads, frozen=()):
    def call(q, k, v, ew, we, sk, g, ptr, col, t_ptr, t_edge, t_tgt):
        leaves = [t.detach().requires_grad_(name not in frozen) if t is not None else None
                  for name, t in zip(FLOATS, (q, k, v, ew, we, sk))]
        transpose = (t_ptr, t_edge, t_tgt) if t_ptr is not None else None
        out = gnn.attn_aggregate_autograd(*leaves[:3], ptr, col, *leaves[3:], heads, transpose=transpose)
        want = [t for t in leaves[:5] if t is not None and t.requires_grad]
        got = iter(torch.autograd.grad(out, want, g))
        grads = [next(got) if t is not None and t.requires_grad else None for t in leaves[:5]]
        return dict(out=out.detach(), **dict(zip(GRADS, grads)))
    return call


def _work(c):
    n, nE, heads = c["q"].shape[0], c["col"].numel(), c["heads"]
    return [(_lib.work_floats("gsm_attn_backward_work_floats", n, nE, heads, c["q"].shape[1] // heads),)]


def _plain(c, out=None, grads=None):
    out, grads = (c["out"], c["grads"]) if out is None else (out, grads)
    return dict(out=out, **dict(zip(GRADS, grads[:5])))


@pytest.mark.parametrize("heads,C", DISPATCH)
@pytest.mark.parametrize("edge,skip", OPTS)
def test_attention_forward_backward(heads, C, edge, skip):
    """gsm_attn_aggregate_fwd and gsm_attn_aggregate_bwd, `transpose` passed in."""
    c = _case(heads, C, edge, skip)
    G.run_case(_fwd_bwd(heads), _inputs(c, c["transpose"]), plain=_plain(c), work=_work(c))


@pytest.mark.parametrize("heads,C", [(3, 16), (1, 1)])
def test_attention_transpose_built_inside(heads, C):
    c = _case(heads, C, True, True)
    G.run_case(_fwd_bwd(heads), _inputs(c, None), plain=_plain(c), work=_work(c))


@pytest.mark.parametrize("frozen", [("ew",), ("we",), ("ew", "we")], ids=["edge_w", "w_e", "both"])
@pytest.mark.parametrize("heads,C", [(3, 16), (3, 2)])
def test_attention_gradients_not_wanted(heads, C, frozen):
    """dedge_w and dw_e "may be NULL (not wanted)": the launches with one or both left out write the
    others as before and nothing else."""
    c = _case(heads, C, True, True)
    plain = _plain(c)
    for name, out in (("ew", "dedge_w"), ("we", "dw_e")):
        if name in frozen:
            plain[out] = None
    G.run_case(_fwd_bwd(heads, frozen), _inputs(c, c["transpose"]), plain=plain, work=_work(c))


@pytest.mark.parametrize("which", [("q", "k", "v", "sk"), ("g",)])
def test_attention_misaligned(which):
    """(3, 16) with bases 4 bytes past a 256-byte boundary: the scalar kernels; with grad_out alone
    misaligned a float4 forward and a scalar backward."""
    assert select(3, 16)[1] == 4 and select(3, 16, aligned=False)[1] == 1
    c = _case(3, 16, True, True)
    out, grads = _run_misaligned(c, which)
    ins = _inputs(c, c["transpose"], misalign=which)
    G.run_case(_fwd_bwd(3), ins, plain=_plain(c, out, grads), work=_work(c))


@pytest.mark.parametrize("heads,C,n", CAPPED[1:3], ids=["4x16-unequal-walks", "3x2-dead-lanes"])
def test_attention_past_the_grid_cap(heads, C, n):
    """More node groups than the target kernel's grid has workgroups: the stride loop takes further trips,
    the workgroups walk unequal numbers of groups, and all kBwdMaxBlocks partials of `work` are in use."""
    groups, per_group = _groups(heads, C, n)
    assert groups > BWD_MAX_BLOCKS and groups % BWD_MAX_BLOCKS and n % per_group
    c = _case(heads, C, True, True, n)
    G.run_case(_fwd_bwd(heads), _inputs(c, c["transpose"]), plain=_plain(c), work=_work(c))


@pytest.mark.parametrize("n", [5, 1])
def test_attention_without_edges(n):
    """The no-edge graph and the one-node graph: out = skip, the gradients zeros, all of them written."""
    gen = torch.Generator(device=DEV).manual_seed(0)
    q, k, v, sk, g = (torch.randn(n, 8, device=DEV, generator=gen) for _ in range(5))
    c = dict(heads=2, q=q, k=k, v=v, sk=sk, g=g, ew=torch.zeros(0, device=DEV),
             we=torch.randn(8, device=DEV, generator=gen), ptr=torch.zeros(n + 1, dtype=torch.int64, device=DEV),
             col=torch.zeros(0, dtype=torch.int32, device=DEV))
    call = _fwd_bwd(2)
    ins = _inputs(c, None)
    plain = G.run_case(call, ins, work=_work(c))
    assert torch.equal(plain["out"], sk) and all(int(torch.count_nonzero(plain[k_])) == 0 for k_ in GRADS)


def test_attention_one_node_with_a_self_loop():
    gen = torch.Generator(device=DEV).manual_seed(1)
    q, k, v, sk, g = (torch.randn(1, 8, device=DEV, generator=gen) for _ in range(5))
    c = dict(heads=2, q=q, k=k, v=v, sk=sk, g=g, ew=torch.rand(1, device=DEV, generator=gen),
             we=torch.randn(8, device=DEV, generator=gen), ptr=torch.tensor([0, 1], device=DEV),
             col=torch.zeros(1, dtype=torch.int32, device=DEV))
    plain = G.run_case(_fwd_bwd(2), _inputs(c, None), work=_work(c))
    e = c["ew"] * c["we"]
    assert torch.allclose(plain["out"], v + e + sk, atol=1e-6)       # one entry: its softmax weight is 1
    assert torch.allclose(plain["dv"], g, atol=1e-6)


@pytest.mark.parametrize("heads,C,edge,skip", [(3, 16, True, True), (1, 1, False, False), (5, 2, True, True),
                                               (64, 1, False, False)])
def test_attention_forward(heads, C, edge, skip):
    """gsm_attn_aggregate (no statistics), its float4 and scalar forms."""
    c = _case(heads, C, edge, skip)

    def call(q, k, v, ew, we, sk, ptr, col):
        return dict(out=gnn.attn_aggregate(q, k, v, ptr, col, ew, we, sk, heads))

    ins = {k_: v_ for k_, v_ in _inputs(c, None).items() if k_ in FLOATS + ("ptr", "col")}
    G.run_case(call, ins, plain=dict(out=c["out"]))
