"""gsm_attn_aggregate (HIP, gsm_gnn.hip) vs the torch formulation
(gsmarl_amd.gnn.attn_aggregate_ref, fp32 and fp64) on random CSR graphs and on
the env's own graph at the headline size. Tolerance: 2e-5 absolute /
relative against fp64 (hardware exp in the online softmax)."""
import math

import numpy as np
import pytest
import torch

from gsmarl_amd import gnn

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _graph(n, rng, max_deg=6, empty=0.2):
    deg = rng.integers(0, max_deg + 1, size=n)
    deg[rng.random(n) < empty] = 0
    ptr = np.zeros(n + 1, np.int64)
    np.cumsum(deg, out=ptr[1:])
    col = rng.integers(0, n, size=int(ptr[-1])).astype(np.int32)
    return torch.from_numpy(ptr).to(DEV), torch.from_numpy(col).to(DEV)


@pytest.mark.parametrize("heads,C", [(1, 1), (1, 4), (2, 8), (3, 16), (4, 16), (2, 32), (1, 64)])
@pytest.mark.parametrize("edge,skip", [(True, True), (False, False)])
def test_kernel_matches_reference(heads, C, edge, skip):
    rng = np.random.default_rng(heads * 100 + C)
    n = 2000
    ptr, col = _graph(n, rng)
    HC = heads * C
    g = torch.Generator(device=DEV).manual_seed(3)
    q, k, v, sk = (torch.randn(n, HC, device=DEV, generator=g) for _ in range(4))
    ew = torch.rand(col.numel(), device=DEV, generator=g) if edge else None
    we = torch.randn(HC, device=DEV, generator=g) if edge else None
    s = sk if skip else None
    out = gnn.attn_aggregate(q, k, v, ptr, col, ew, we, s, heads)
    ref = gnn.attn_aggregate_ref(q.double(), k.double(), v.double(), ptr, col,
                                 ew.double() if edge else None, we.double() if edge else None,
                                 s.double() if skip else None, heads)
    err = (out.double() - ref).abs()
    assert torch.all(err <= 2e-5 * (1 + ref.abs())), float(err.max())
    empty = (ptr[1:] == ptr[:-1])
    base = s if skip else torch.zeros_like(q)
    assert torch.equal(out[empty], base[empty])          # no neighbours -> 0 (+ skip)


# Scores that are exact in fp32 and far apart, so that the online softmax's
# rescale from mx = -inf and across large jumps is what decides the result:
# scale = 1, no edge term, q_i[h] = (8, 0, ..), k_j[h][0] an integer in
# [-16, 16] (the head's other channels random: they meet q's zeros), so a score
# is 8 * k_j[h][0], an integer in [-128, 128]; v random. A row has its own
# sources, listed in the order of the pattern.
ORDERED_SHAPES = [(1, 1), (2, 4), (3, 16)]
PATTERNS = ("ascending", "descending", "middle", "equal", "tied")
ORDERED_DEGS = (33,) * 10 + (300,) * 5                     # row r, head h: PATTERNS[(r + h) % 5]
_ORDERED = {}


def _pattern(name, d):
    """k_j[h][0] along a row of d entries."""
    t = np.arange(d)
    if name == "ascending":                                 # every step raises the maximum (d = 33: by 8)
        return np.round(np.linspace(-16, 16, d))
    if name == "descending":
        return np.round(np.linspace(16, -16, d))
    if name == "middle":                                    # the maximum in the middle
        return np.round(16 - 32 * np.abs(t - d // 2) / (d // 2))
    if name == "equal":                                     # the output is the plain mean
        return np.full(d, 3.0)
    x = np.full(d, -4.0)                                    # two tied maxima 13 steps = 104 above the rest (the
    x[[d // 6, (2 * d) // 3]] = 9.0                         # multiple of 8 next to 100): the rest weigh exp(-104)
    return x


def ordered_case(heads, C):
    """The graph and inputs above; built once per shape and left unchanged."""
    if (heads, C) in _ORDERED:
        return _ORDERED[(heads, C)]
    R, HC = len(ORDERED_DEGS), heads * C
    n = R + sum(ORDERED_DEGS)
    deg = np.zeros(n, np.int64)
    deg[:R] = ORDERED_DEGS
    ptr = np.zeros(n + 1, np.int64)
    np.cumsum(deg, out=ptr[1:])
    col = np.arange(R, n, dtype=np.int32)                   # row r's sources: its own run of nodes
    g = torch.Generator(device=DEV).manual_seed(11)
    k, v, grad = (torch.randn(n, HC, device=DEV, generator=g) for _ in range(3))
    q = torch.zeros(n, HC, device=DEV)
    q[:, ::C] = 8.0
    k0 = np.zeros((n - R, heads), np.float32)
    equal = np.zeros((R, heads), bool)
    for r, d in enumerate(ORDERED_DEGS):
        for h in range(heads):
            name = PATTERNS[(r + h) % 5]
            k0[ptr[r]:ptr[r + 1], h] = _pattern(name, d)
            equal[r, h] = name == "equal"
    assert np.abs(k0).max() == 16 and np.array_equal(k0, np.round(k0))
    k[R:, ::C] = torch.from_numpy(k0).to(DEV)
    c = dict(heads=heads, C=C, R=R, q=q, k=k, v=v, g=grad, ptr=torch.from_numpy(ptr).to(DEV),
             col=torch.from_numpy(col).to(DEV), equal=torch.from_numpy(equal).to(DEV))
    c["ref"] = gnn.attn_aggregate_ref(q.double(), k.double(), v.double(), c["ptr"], c["col"], heads=heads, scale=1.0)
    _ORDERED[(heads, C)] = c
    return c


@pytest.mark.parametrize("heads,C", ORDERED_SHAPES)
def test_extreme_and_ordered_scores(heads, C):
    c = ordered_case(heads, C)
    R, ptr, ref = c["R"], c["ptr"], c["ref"]
    out = gnn.attn_aggregate(c["q"], c["k"], c["v"], ptr, c["col"], heads=heads, scale=1.0)
    err = (out.double() - ref).abs()
    print(f"H{heads} C{C} ordered scores: worst normalised error {float((err / (1 + ref.abs())).max()):.3e}")
    assert torch.all(err <= 2e-5 * (1 + ref.abs())), float(err.max())
    assert torch.count_nonzero(out[R:]) == 0                # the sources' own rows are empty
    # equal scores: the plain mean of the row's v
    means = torch.stack([c["v"][int(ptr[r]) + R:int(ptr[r + 1]) + R].double().mean(0) for r in range(R)])
    eq = c["equal"][:, :, None].expand(R, heads, C).reshape(R, heads * C)
    assert int(c["equal"].sum()) >= 3 * heads
    assert float((ref[:R] - means).abs()[eq].max()) <= 1e-12
    assert torch.all(((out[:R].double() - means).abs() <= 2e-5 * (1 + means.abs()))[eq])


def test_env_graph_headline_size():
    """Message passing over the env's own COO output (symmetric, row-major =
    CSR over targets) at 24 agents x 8192 envs."""
    from gsmarl_amd import EnvConfig, GpuBatchEnv
    env = GpuBatchEnv(EnvConfig(n_agents=24, n_envs=8192, seed=1), DEV)
    out = env.reset(seed=1)
    n = env.B * env.E
    ptr = gnn.env_csr(out["edge_index"], n)
    col = out["edge_index"][1].contiguous()
    conv = gnn.TransformerConv(7, 16, heads=3, concat=True).to(DEV)
    x = out["node_feat"].reshape(n, 7)
    with torch.no_grad():
        y = conv(x, ptr, col, out["edge_attr"].reshape(-1, 1))
        conv.use_kernel = False
        y_ref = conv(x, ptr, col, out["edge_attr"].reshape(-1, 1))
    assert y.shape == (n, 48)
    assert torch.allclose(y, y_ref, rtol=2e-5, atol=2e-5), float((y - y_ref).abs().max())
    env.close()


def test_rejects_unsupported_shapes():
    from gsmarl_amd._lib import GsmError
    q = torch.zeros(4, 48, device=DEV)
    ptr = torch.zeros(5, dtype=torch.int64, device=DEV)
    col = torch.zeros(0, dtype=torch.int32, device=DEV)
    with pytest.raises(GsmError):
        gnn.attn_aggregate(q, q, q, ptr, col, heads=1)        # C = 48: not a power of two
    with pytest.raises(GsmError):
        gnn.attn_aggregate(torch.zeros(4, 128, device=DEV), torch.zeros(4, 128, device=DEV),
                           torch.zeros(4, 128, device=DEV), ptr, col, heads=2)   # H*C > 64
