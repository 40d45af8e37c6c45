"""Every instantiation the four launchers of gsm_gnn.hip can select
(gsm_attn_aggregate_fwd / _bwd, gsm_env_conv / _fwd / _bwd), run and compared
with the fp64 references. test_gnn_dispatch_ref.py restates the launchers' rule
on the CPU and shows that DISPATCH maps onto all twelve (lanes per node,
channels per lane) cases; this file walks the list.

Attention: forward and backward through gnn.attn_aggregate_autograd on
test_gpu_gnn_backward's planted graph (hub, a row of 40, self loop, duplicate,
never-a-source, empty rows, n = 1003) with that file's criteria unchanged, and
`out` held to 2e-5 * (1 + |ref|) against fp64 as well. Then the other route to
one channel per lane: contiguous tensors whose base is 4 bytes past a 16-byte
boundary, one input at a time (a single misaligned pointer has to flip the
whole launch), the last of them the upstream gradient alone, which gives a
float4 forward followed by a scalar backward over the same saved statistics.

env_conv: forward through TransformerConv.forward_env, gradients through
gnn.env_conv_autograd, with test_gpu_env_conv*.py's helpers and bounds. Table
form: every DISPATCH entry on "n3" (E = 9: seven envs a workgroup, a partial
last group) and "n24" (E = 72). Recompute form: RECOMPUTE on "n96" (E = 288),
which selects (8,4), (16,4), (32,1) and (64,1). The table form needs 10400 +
2304 * HC bytes of LDS at E = 288 and never exceeds 64 KiB at E = 9, 18, 72, so
the recompute form starts at HC = 24 (HC = 20 in the backward, whose stage
comes on top), where LP * VEC >= 24: those four are the only recompute
instantiations a legal shape can reach (test_gnn_dispatch_ref.py checks the
arithmetic); the other eight are compiled and never launched."""
import pytest
import torch

import test_gpu_env_conv as fwd
import test_gpu_env_conv_backward as bwd
from gsmarl_amd import gnn
from test_gnn_dispatch_ref import DISPATCH, RECOMPUTE, select
from test_gpu_gnn_backward import (BOUND, HUB, LONG, N, NEVER, OPTS, _case, _exact_rows_and_forward, _is_reproducible,
                                   _matches_reference, _norm_err)

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
# one shape per instantiation: these run all four (skip, edge) combinations of env_conv
ALL_OPTS = [(1, 4), (2, 4), (2, 8), (3, 8), (3, 16), (1, 1), (1, 2), (3, 1), (3, 2), (5, 2), (12, 2), (20, 2)]
MISALIGNED = {"q k v skip": ("q", "k", "v", "sk"), "v": ("v",), "w_e": ("we",), "grad_out": ("g",)}
_OUT_REF = {}


def _out_ref(c, key):
    """fp64 forward of a test_gpu_gnn_backward case, computed once."""
    if key not in _OUT_REF:
        d = lambda t: t.double() if t is not None else None
        _OUT_REF[key] = gnn.attn_aggregate_ref(d(c["q"]), d(c["k"]), d(c["v"]), c["ptr"], c["col"], d(c["ew"]),
                                               d(c["we"]), d(c["sk"]), c["heads"])
    return _OUT_REF[key]


@pytest.mark.parametrize("heads,C", DISPATCH)
@pytest.mark.parametrize("edge,skip", OPTS)
def test_attention_every_instantiation(heads, C, edge, skip):
    c = _case(heads, C, edge, skip)
    ref = _out_ref(c, (heads, C, edge, skip))
    e_out = float(((c["out"].double() - ref).abs() / (1 + ref.abs())).max())
    print(f"H{heads} C{C} {select(heads, C)} edge={edge} skip={skip} out: worst normalised error {e_out:.3e}")
    assert e_out <= BOUND
    _matches_reference(c, heads, C, edge, skip)
    _exact_rows_and_forward(c, heads, skip)
    _is_reproducible(c)


def _misaligned(t):
    """A contiguous copy of t that starts 4 bytes past a 16-byte boundary."""
    m = torch.empty(t.numel() + 1, dtype=t.dtype, device=t.device)[1:].view(t.shape)
    m.copy_(t)
    assert m.is_contiguous() and m.data_ptr() % 16 == 4
    return m.detach()


def _run_misaligned(c, which):
    ins = {}
    for name in ("q", "k", "v", "ew", "we", "sk"):
        t = _misaligned(c[name]) if name in which else c[name].clone()
        assert (t.data_ptr() % 16 == 4) == (name in which)
        ins[name] = t.requires_grad_(True)
    g = _misaligned(c["g"]) if "g" in which else c["g"]
    out = gnn.attn_aggregate_autograd(ins["q"], ins["k"], ins["v"], c["ptr"], c["col"], ins["ew"], ins["we"], ins["sk"],
                                      c["heads"], transpose=c["transpose"])
    out.backward(g)
    return out.detach(), tuple(ins[name].grad for name in ("q", "k", "v", "ew", "we", "sk"))


@pytest.mark.parametrize("heads,C", [(3, 16), (2, 8), (1, 4)])
@pytest.mark.parametrize("what", list(MISALIGNED))
def test_attention_misaligned_inputs(heads, C, what):
    assert select(heads, C)[1] == 4 and select(heads, C, aligned=False)[1] == 1
    c = _case(heads, C, True, True)
    ref = _out_ref(c, (heads, C, True, True))
    out, grads = _run_misaligned(c, MISALIGNED[what])
    e_out = float(((out.double() - ref).abs() / (1 + ref.abs())).max())
    e_al = float(((out.double() - c["out"].double()).abs() / (1 + ref.abs())).max())
    kern, aligned = _norm_err(c, grads), _norm_err(c, c["grads"])
    print(f"H{heads} C{C} misaligned {what}: out vs fp64 {e_out:.3e} vs the aligned run {e_al:.3e} | "
          f"gradients {kern} | aligned {aligned}")
    assert e_out <= BOUND and e_al <= BOUND
    # one channel per lane sums a head's score over lanes, four per lane inside a lane first: the launch
    # that took the other kernels shows in the last bits of some element
    if what == "grad_out":
        assert torch.equal(out, c["out"])                    # the aligned (float4) forward, then a scalar backward
    else:
        assert not torch.equal(out, c["out"])
    assert not torch.equal(grads[0], c["grads"][0])
    for name, e in kern.items():
        assert e <= BOUND, (name, e)
    dq, dk, dv, _, _, dsk = grads
    assert torch.equal(dsk, c["g"])                          # dskip is grad_out, bitwise
    assert torch.count_nonzero(dk[NEVER]) == 0 and torch.count_nonzero(dv[NEVER]) == 0
    empty = c["ptr"][1:] == c["ptr"][:-1]
    assert int(empty.sum()) > 50 and torch.count_nonzero(dq[empty]) == 0
    assert torch.count_nonzero(dk[HUB]) > 0 and torch.count_nonzero(dq[LONG]) > 0
    out2, again = _run_misaligned(c, MISALIGNED[what])
    assert torch.equal(out2, out)
    for a, b in zip(again, grads):
        assert torch.equal(a, b)


def _conv_opts(heads, C):
    return bwd.OPTS if (heads, C) in ALL_OPTS else bwd.OPTS[:2]


def _conv_cases():
    table = [(kind, h, C) for kind in ("n3", "n24") for h, C in DISPATCH]
    return table + [("n96", h, C) for h, C in RECOMPUTE]


def test_conv_cases_cover_every_instantiation():
    assert {select(h, C) for h, C in ALL_OPTS} == {select(h, C) for h, C in DISPATCH} and len(ALL_OPTS) == 12
    assert {select(h, C) for h, C in RECOMPUTE} == {select(h, C) for h, C in RECOMPUTE if (h, C) in ALL_OPTS}
    assert {rows for _, _, rows in bwd.OPTS[:2]} == {"all", "agents"}
    assert fwd.SHAPES["n3"][0] * 3 == 9 and fwd.SHAPES["n24"][0] * 3 == 72 and fwd.SHAPES["n96"][0] * 3 == 288
    assert N == 1003


@pytest.mark.parametrize("kind,heads,C", _conv_cases())
def test_env_conv_forward(kind, heads, C):
    g = fwd._graph(kind)
    assert g["E"] == 3 * fwd.SHAPES[kind][0]
    for skip, edge, rows in _conv_opts(heads, C):
        R = g["E"] if rows == "all" else g["N"]
        conv = fwd._conv(heads, C, skip, edge, seed=heads * 100 + C)
        with torch.no_grad():
            out = conv.forward_env(g, rows=rows, n_agents=g["N"])
        assert out.shape == (g["B"], R, heads * C) and out.dtype == torch.float32
        e = fwd._nerr(out, fwd._ref64(g, conv, R))
        print(f"{kind} {heads}x{C} {select(heads, C)} skip={skip} edge={edge} rows={rows}: out worst normalised "
              f"error {e:.3e}")
        assert e <= 2e-5


@pytest.mark.parametrize("kind,heads,C", _conv_cases())
def test_env_conv_gradients(kind, heads, C):
    g = fwd._graph(kind)
    for skip, edge, rows in _conv_opts(heads, C):
        R = g["E"] if rows == "all" else g["N"]
        w, w_e = bwd._weights(heads, C, skip, edge, seed=heads * 100 + C)
        go = bwd._grad_out(g, R, heads * C)
        out, dw, dw_e, st = bwd._kernel_grads(g, w, w_e, heads, R, skip, go)
        assert st == 0
        fwd._same(out, gnn.env_conv(*bwd._args(g), w, w_e, heads, R, skip), "out of the forward with statistics")
        _, lse, _ = bwd._fwd_raw(g, w, w_e, heads, R, skip)
        ref, full = bwd._lse64(g, w, w_e, heads)
        ref, full = ref[:, :R], full[:, :R]
        assert bool(full.any()) and bool((lse[~full] == 0).all())
        e_l = float(((lse.double() - ref).abs() / (1 + ref.abs()))[full].max())
        rw, re, s_w, s_e = bwd._reference(g, w, w_e, heads, R, skip, go)
        tw, te = bwd._torch32(g, w, w_e, heads, R, skip, go)
        e_k, e_t = bwd._nerr(dw, rw, s_w), bwd._nerr(tw, rw, s_w)
        msg = (f"{kind} {heads}x{C} {select(heads, C)} skip={skip} edge={edge} rows={rows}: lse {e_l:.3e} | "
               f"dw kernel {e_k:.3e} torch fp32 {e_t:.3e}")
        if edge:
            f_k, f_t = bwd._nerr(dw_e, re, s_e), bwd._nerr(te, re, s_e)
            msg += f" | dw_e kernel {f_k:.3e} torch fp32 {f_t:.3e}"
        print(msg)
        assert e_l <= bwd.BOUND and e_k <= bwd.BOUND, msg
        if edge:
            assert f_k <= bwd.BOUND, msg
        else:
            assert dw_e is None
        _, dw2, dw_e2, _ = bwd._kernel_grads(g, w, w_e, heads, R, skip, go)
        fwd._same(dw, dw2, "dw of two calls")
        if edge:
            fwd._same(dw_e, dw_e2, "dw_e of two calls")
