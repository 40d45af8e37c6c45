"""CPU side of the GNN kernels' dispatch matrix (tests/test_gpu_gnn_dispatch.py
runs it on the GPU): the launchers' choice of instantiation and of env_conv's
table / recompute form restated in Python from their description (the source
is not parsed), so that the list of shapes the GPU file walks is shown to
reach every case of the switch and every reachable recompute instantiation;
and the two fp64 references checked against autograd at the new shapes before
they judge a kernel.

The rule (launch_attn_aggregate, launch_attn_backward, launch_env_conv,
launch_env_conv_backward): a lane takes VEC = 4 channels iff C % 4 == 0 and
H*C % 4 == 0 and every row pointer is 16-byte aligned, else VEC = 1; a node
takes LP lanes, the smallest power of two with LP * VEC >= H*C."""
import itertools

import numpy as np
import pytest

import test_env_conv_backward_ref as conv_ref
import test_gnn_backward_ref as attn_ref
from test_env_conv_ref import E as REF_E, N as REF_N, _graph as _two_env_graph

# (heads, C): every case of the 12-way switch; HC = 24 and HC = 3 leave dead lanes
DISPATCH = [(1, 4), (2, 4), (1, 8), (2, 8), (3, 8), (2, 16), (3, 16), (4, 16),
            (1, 1), (1, 2), (2, 1), (3, 1), (3, 2), (5, 2), (8, 2), (12, 2), (16, 2), (20, 2), (32, 2), (64, 1)]
CASES = [(1, 4), (2, 4), (4, 4), (8, 4), (16, 4), (1, 1), (2, 1), (4, 1), (8, 1), (16, 1), (32, 1), (64, 1)]
# the shapes test_gpu_gnn_dispatch runs on the 288-entity graph
RECOMPUTE = [(3, 8), (2, 16), (3, 16), (4, 16), (12, 2), (16, 2), (20, 2), (32, 2), (64, 1)]
RECOMPUTE_CASES = {(8, 4), (16, 4), (32, 1), (64, 1)}
LDS_MAX = 64 * 1024
CONV_THREADS = 256


def select(heads, C, aligned=True):
    """(LP, VEC) of a launch."""
    HC = heads * C
    vec = 4 if (C % 4 == 0 and HC % 4 == 0 and aligned) else 1
    lp = 1
    while lp * vec < HC:
        lp *= 2
    return lp, vec


def legal_shapes():
    """Every (heads, C) the ABI accepts: C a power of two, heads * C <= 64."""
    return [(h, C) for C in (1, 2, 4, 8, 16, 32, 64) for h in range(1, 64 // C + 1)]


def envs_per_block(E):
    return 1 if E >= 64 else 64 // E


def conv_lds(epb, E, HC, table):
    """Bytes of LDS of an env_conv workgroup: rows [n][8] f32, per env a checked
    start (int64), a count and a flag (int), row starts [E+1] int, rounded up to
    16; then, in the table form, k and v [2][n][HC] f32."""
    n = epb * E
    rs = n * 32 + epb * 8 + epb * 4 + epb * 4
    tab = (rs + epb * (E + 1) * 4 + 15) & ~15
    return tab + (2 * n * HC * 4 if table else 0)


def conv_bwd_stage(vec, HC):
    """The backward's pass stage [2][256 * VEC] and accumulators [16][2 * HC], f32."""
    return 2 * CONV_THREADS * vec * 4 + 16 * 2 * HC * 4


def conv_form(E, heads, C, aligned=True, backward=False):
    """'table' or 'recompute' for a legal launch (one of the two always fits)."""
    HC = heads * C
    _, vec = select(heads, C, aligned)
    extra = conv_bwd_stage(vec, HC) if backward else 0
    epb = envs_per_block(E)
    if conv_lds(epb, E, HC, True) + extra <= LDS_MAX:
        return "table"
    assert conv_lds(epb, E, HC, False) + extra <= LDS_MAX
    return "recompute"


def test_dispatch_list_reaches_every_case():
    assert all((h, C) in legal_shapes() for h, C in DISPATCH)
    reached = [select(h, C) for h, C in DISPATCH]
    assert set(reached) == set(CASES) and len(set(CASES)) == 12
    for case in CASES:                                       # the table of the issue, row by row
        assert case in reached
    want = {(1, 4): (1, 4), (2, 4): (2, 4), (1, 8): (2, 4), (2, 8): (4, 4), (3, 8): (8, 4), (2, 16): (8, 4),
            (3, 16): (16, 4), (4, 16): (16, 4), (1, 1): (1, 1), (1, 2): (2, 1), (2, 1): (2, 1), (3, 1): (4, 1),
            (3, 2): (8, 1), (5, 2): (16, 1), (8, 2): (16, 1), (12, 2): (32, 1), (16, 2): (32, 1), (20, 2): (64, 1),
            (32, 2): (64, 1), (64, 1): (64, 1)}
    assert {s: select(*s) for s in DISPATCH} == want
    # dead lanes: LP * VEC > HC
    assert select(3, 8) == (8, 4) and 8 * 4 > 24 and select(3, 1) == (4, 1) and 4 > 3
    # no legal shape reaches anything else, aligned or not
    for h, C in legal_shapes():
        assert select(h, C) in CASES and select(h, C, aligned=False) in CASES


def test_misaligned_base_takes_the_scalar_kernels():
    assert select(3, 16, aligned=False) == (64, 1)
    assert select(2, 8, aligned=False) == (16, 1)
    assert select(1, 4, aligned=False) == (4, 1)
    for h, C in DISPATCH:
        assert select(h, C, aligned=False)[1] == 1


def test_env_conv_recompute_reachability():
    """The table form needs 10400 + 2304 * HC <= 65536 bytes at E = 288 (one env
    a workgroup), so the forward's recompute form starts at HC = 24; the
    backward adds its stage (8192 + 128 * HC bytes at VEC = 4, 2048 + 128 * HC at
    VEC = 1), which moves its threshold to HC = 20 resp. 22 and adds no
    instantiation; E in {9, 18, 72} never recomputes. Hence the only recompute
    instantiations a legal shape reaches are (8,4), (16,4), (32,1), (64,1)."""
    assert envs_per_block(288) == 1 and conv_lds(1, 288, 0, False) == 10400
    for HC in range(1, 65):
        assert conv_lds(1, 288, HC, True) == 10400 + 2304 * HC
    assert 10400 + 2304 * 23 <= LDS_MAX < 10400 + 2304 * 24
    assert [envs_per_block(E) for E in (9, 18, 72)] == [7, 3, 1]
    fwd, bwd = set(), set()
    for (h, C), aligned in itertools.product(legal_shapes(), (True, False)):
        for E in (9, 18, 72):
            assert conv_form(E, h, C, aligned) == "table" and conv_form(E, h, C, aligned, backward=True) == "table"
        assert (conv_form(288, h, C, aligned) == "recompute") == (h * C >= 24)
        vec = select(h, C, aligned)[1]
        assert (conv_form(288, h, C, aligned, backward=True) == "recompute") == (h * C >= (20 if vec == 4 else 22))
        if conv_form(288, h, C, aligned) == "recompute":
            fwd.add(select(h, C, aligned))
        if conv_form(288, h, C, aligned, backward=True) == "recompute":
            bwd.add(select(h, C, aligned))
    assert fwd == RECOMPUTE_CASES and bwd == RECOMPUTE_CASES
    # the GPU file's list for the 288-entity graph: all of them recompute, in both directions, and reach all four
    assert all(s in DISPATCH for s in RECOMPUTE)
    assert all(conv_form(288, h, C) == conv_form(288, h, C, backward=True) == "recompute" for h, C in RECOMPUTE)
    assert {select(h, C) for h, C in RECOMPUTE} == RECOMPUTE_CASES
    # and every other DISPATCH entry takes the table form there
    assert all(conv_form(288, h, C, backward=True) == "table" for h, C in DISPATCH if (h, C) not in RECOMPUTE)


REF_SHAPES = [(3, 1), (20, 2), (32, 2), (64, 1), (2, 16)]


@pytest.mark.parametrize("heads,Cc", REF_SHAPES)
@pytest.mark.parametrize("edge,skip", [(True, True), (False, False)])
def test_attn_bwd_ref_matches_autograd(heads, Cc, edge, skip):
    ptr, col = attn_ref._graph(23, np.random.default_rng(heads * 10 + Cc))
    attn_ref._check(ptr, col, heads, Cc, edge, skip, seed=1)
    attn_ref._check(*attn_ref._adversarial(), heads, Cc, edge, skip, seed=2)


@pytest.mark.parametrize("heads,Cc", REF_SHAPES)
@pytest.mark.parametrize("skip,edge", [(True, True), (False, False)])
def test_env_conv_bwd_ref_matches_autograd(heads, Cc, skip, edge):
    conv_ref._check(_two_env_graph(), REF_E, skip, edge, heads=heads, Cc=Cc)
    conv_ref._check(_two_env_graph(), REF_N, skip, edge, heads=heads, Cc=Cc)
    gr, n_agents = conv_ref._oracle_graph()
    conv_ref._check(gr, n_agents, skip, edge, heads=heads, Cc=Cc)
