"""gsm_env_conv (the fused first GNN layer, gsm_gnn.hip) through
TransformerConv.forward_env / gnn.env_conv, against gnn.env_conv_ref in fp64 on
the GPU. Bound |err| <= 2e-5 * (1 + |ref|), the aggregation's own; on the spread
layout (entities at |x| >= 8, scores growing with |x|^2) the bound is four
times the error of the fp32 torch formulation on the same inputs. Exact
properties (reproducibility, agent rows, row offsets, empty rows, sliced against
unsliced edge arrays) are compared bit for bit; corrupt offsets and ids, all
pointing inside the allocations, have to come back as status bits and edgeless
envs."""
import pytest
import torch

import roll_states
from gsmarl_amd import _lib, gnn

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
HEADS = [(3, 16), (4, 16), (1, 64), (2, 8), (1, 1)]
# (N, B): E = 9 (several envs a workgroup, a partial last group), 18, 72 (more
# rows than a wave has lanes), 288 (the recompute form from HC = 24 up)
SHAPES = {"n3": (3, 5), "n6": (6, 40), "n24": (24, 3), "n96": (96, 2)}
_CACHE = {}


def _snapshot(env, out=None):
    """The env's current graph as clones: the unsliced edge arrays and the total."""
    torch.cuda.synchronize()
    t = env.t if out is None else out
    g = dict(node_feat=t["node_feat"].clone(), edge_ptr=t["edge_ptr"].clone(), edge_index=t["edge_index"].clone(),
             edge_attr=t["edge_attr"].clone())
    g["total"] = int(g["edge_ptr"][-1])
    g["N"], g["E"], g["B"] = env.N, env.E, env.B
    return g


def _graph(kind):
    """Graphs come from GpuBatchEnv after a reset and three steps (or an
    injected state); built once and left unchanged."""
    if kind in _CACHE:
        return _CACHE[kind]
    from gsmarl_amd import EnvConfig, GpuBatchEnv
    if kind in SHAPES:
        N, B = SHAPES[kind]
        cfg = EnvConfig(n_agents=N, n_envs=B, seed=11)
    elif kind == "mixed":
        cfg = EnvConfig(scenario="mixed", n_agents=12, n_envs=48, seed=4)
    else:
        cfg = EnvConfig(n_agents=24, n_obstacles=24, n_envs=5, seed=11)
    env = GpuBatchEnv(cfg, DEV)
    env.reset(seed=cfg.seed)
    if kind in ("crowd", "spread"):
        st = getattr(roll_states, kind)(24, 24, 5)
        env.set_state({k: torch.from_numpy(st[k]) for k in ("pos", "vel", "step_count")})
    else:
        g = torch.Generator(device=DEV).manual_seed(5)
        for _ in range(3):
            env.step(torch.randint(0, 5, (env.B, env.N), dtype=torch.int32, device=DEV, generator=g))
    _CACHE[kind] = _snapshot(env)
    env.close()
    return _CACHE[kind]


def _sliced(g):
    d = dict(g)
    d["edge_index"], d["edge_attr"] = g["edge_index"][:, :g["total"]], g["edge_attr"][:g["total"]]
    return d


def _conv(heads, C, skip=True, edge=True, seed=0):
    torch.manual_seed(seed)
    return gnn.TransformerConv(7, C, heads=heads, edge_dim=1 if edge else None, root_weight=skip).to(DEV)


def _ref64(g, conv, R=None):
    w, w_e = gnn.pack_conv_params(conv)
    with torch.no_grad():
        return gnn.env_conv_ref(g["node_feat"].double(), g["edge_ptr"], g["edge_index"], g["edge_attr"].double(),
                                w.double(), w_e.double() if w_e is not None else None, conv.heads,
                                g["E"] if R is None else R, conv.lin_skip is not None)


def _nerr(out, ref):
    """Largest err / (1 + |ref|)."""
    return float(((out.double() - ref).abs() / (1 + ref.abs())).max())


def _bits(x):
    return x.view(torch.int32) if x.dtype == torch.float32 else x


def _same(a, b, what=""):
    assert a.shape == b.shape and a.dtype == b.dtype, what
    assert torch.equal(_bits(a), _bits(b)), what


@pytest.mark.parametrize("heads,C", HEADS)
@pytest.mark.parametrize("kind", list(SHAPES) + ["mixed", "crowd"])
def test_matches_fp64_reference(kind, heads, C):
    g = _graph(kind)
    if kind == "crowd":
        deg = gnn.env_csr(g["edge_index"][:, :g["total"]], g["B"] * g["E"]).diff()
        assert g["total"] > 5 * 1800 and int(deg.max()) >= 40    # most of the 2304 an env can hold, long rows
    if kind == "mixed":
        assert bool((g["node_feat"][..., 6] == -1).any())     # padding rows
    for skip, edge in ((True, True), (False, False), (True, False), (False, True)):
        conv = _conv(heads, C, skip, edge, seed=heads * 100 + C)
        with torch.no_grad():
            out = conv.forward_env(g)
        ref = _ref64(g, conv)
        assert out.shape == (g["B"], g["E"], heads * C) and out.dtype == torch.float32
        e = _nerr(out, ref)
        print(f"{kind} {heads}x{C} skip={skip} edge={edge}: worst normalised error {e:.3e}")
        assert e <= 2e-5


def test_spread_against_the_fp32_torch_formulation():
    """Entities at |x| >= 8: E_fused <= 4 * E_torch, E_torch the error of
    env_conv_ref in fp32 on the same inputs (both against fp64)."""
    g = _graph("spread")
    assert float(g["node_feat"][..., 2:4].abs().max()) >= 8.0
    conv = _conv(3, 16)
    w, w_e = gnn.pack_conv_params(conv)
    ref = _ref64(g, conv)
    with torch.no_grad():
        out = conv.forward_env(g)
        tor = gnn.env_conv_ref(g["node_feat"], g["edge_ptr"], g["edge_index"], g["edge_attr"], w, w_e, 3, g["E"], True)
    e_fused, e_torch = _nerr(out, ref), _nerr(tor, ref)
    print(f"spread: E_fused {e_fused:.3e}  E_torch {e_torch:.3e}")
    assert e_fused <= 4 * e_torch


@pytest.mark.parametrize("kind", ["n3", "n6", "n24", "n96", "mixed"])
def test_exact_properties(kind):
    g = _graph(kind)
    B, E, N = g["B"], g["E"], g["N"]
    for heads, C in ((3, 16), (1, 64), (1, 1)):
        conv = _conv(heads, C, skip=False)
        with torch.no_grad():
            out, ptr = conv.forward_env(g, row_ptr=True)
            again = conv.forward_env(g)
            agents = conv.forward_env(g, rows="agents", n_agents=N)
            view = conv.forward_env(_sliced(g))
        _same(out, again, "two calls")
        assert agents.shape == (B, N, heads * C)
        _same(agents, out[:, :N].contiguous(), "agent rows")
        csr = gnn.env_csr(g["edge_index"][:, :g["total"]], B * E)
        _same(ptr, csr, "row_ptr_out")
        empty = (csr.diff() == 0).view(B, E)
        assert bool(empty.any()) and bool((_bits(out[empty]) == 0).all())   # exactly +0 without skip
        _same(view, out, "sliced view")
        # with skip, an empty row is the skip projection alone, in the contract's order
        conv = _conv(heads, C, skip=True)
        w, _ = gnn.pack_conv_params(conv)
        with torch.no_grad():
            out = conv.forward_env(g)
        x = g["node_feat"][empty]
        acc = w[3, :, 7].expand(x.shape[0], -1).clone()
        for f in range(7):
            acc = acc + w[3, :, f] * x[:, f:f + 1]
        _same(out[empty], acc, "skip of empty rows")


def _buffer(B, N, per_env, state=None):
    from gsmarl_amd import EnvConfig, GpuBatchEnv, GraphRolloutBuffer
    env = GpuBatchEnv(EnvConfig(n_agents=N, n_envs=B, seed=8, n_obstacles=N), DEV)
    buf = GraphRolloutBuffer(env, episode_length=2, edges_per_env=per_env)
    buf.reset(seed=8)
    if state is not None:
        env.set_state({k: torch.from_numpy(state[k]) for k in ("pos", "vel", "step_count")})
        env.observe(out=buf.slot(0))
    return env, buf


def test_rollout_buffer_slots():
    env, buf = _buffer(40, 6, None)
    g = torch.Generator(device=DEV).manual_seed(5)
    for _ in range(2):
        buf.insert(torch.randint(0, 5, (env.B, env.N), dtype=torch.int32, device=DEV, generator=g))
    torch.cuda.synchronize()
    conv = _conv(3, 16)
    for t in (0, 2):
        slot = buf.slot(t)
        gr = dict(slot, E=buf.E)
        with torch.no_grad():
            out = conv.forward_env(slot, rows="agents", n_agents=env.N)
        assert _nerr(out, _ref64(gr, conv, R=env.N)) <= 2e-5
    env.close()


def test_truncated_slot():
    """A crowd needs about 2000 entries an env; a buffer sized for 1000 an env
    keeps the first two envs whole and truncates the other three."""
    st = roll_states.crowd(24, 24, 5)
    env, buf = _buffer(5, 24, 1000, st)
    torch.cuda.synchronize()
    slot = buf.slot(0)
    assert bool(buf.overflowed()) and buf.cap == 5000
    conv = _conv(3, 16)
    w, w_e = gnn.pack_conv_params(conv)
    with torch.no_grad():
        with pytest.raises(ValueError, match="capacity"):
            conv.forward_env(slot)
        args = (slot["node_feat"], slot["edge_ptr"], slot["edge_index"], slot["edge_attr"], w.detach(), w_e.detach(),
                3, buf.E, True)
        out, ptr, status = gnn.env_conv(*args, row_ptr=True, check=False)
        assert int(status.item()) == _lib.BATCH_TRUNCATED
        full = _graph("crowd")                               # the same state with room for every entry
        _same(slot["node_feat"], full["node_feat"], "the injected state")
        whole = conv.forward_env(full)
        none = dict(full, edge_ptr=torch.zeros_like(full["edge_ptr"]))
        edgeless = conv.forward_env(none)
    _same(out[:2], whole[:2], "envs inside the capacity")
    _same(out[2:], edgeless[2:], "truncated envs: the edgeless value")
    E, fp = buf.E, full["edge_ptr"].tolist()
    assert fp[2] <= 5000 < fp[3] and slot["edge_ptr"].tolist() == fp
    assert bool((ptr[2 * E:3 * E] == fp[2]).all()) and bool((ptr[3 * E:] == 5000).all())   # start, clamped start
    env.close()


def _corrupt(g, what):
    """A copy of the 6 x 40 graph with in-bounds corruptions; returns it and the
    envs that have to come out edgeless."""
    E = g["E"]
    c = dict(g, edge_ptr=g["edge_ptr"].clone(), edge_index=g["edge_index"].clone())
    ptr = g["edge_ptr"].tolist()
    rows = g["edge_index"][0].tolist()
    bad = []
    if "offsets" in what:                                    # end < start for env 10; its neighbours overlap it
        assert ptr[9] < ptr[10] < ptr[11] < ptr[12]
        c["edge_ptr"][10], c["edge_ptr"][11] = ptr[11], ptr[10]
        bad += [9, 10, 11]
    if "col" in what:                                        # a col pointing into the next env
        assert ptr[20] < ptr[21]
        c["edge_index"][1, ptr[20]] += E
        bad += [20]
    if "order" in what:                                      # the last entry's row below its predecessor's
        lo, hi = ptr[30], ptr[31]
        assert hi - lo >= 2 and rows[lo] < rows[hi - 2]
        c["edge_index"][0, hi - 1] = rows[lo]
        bad += [30]
    if "limit" in what:                                      # the last env runs past the entry bound
        assert ptr[40] - ptr[39] > 3
        c["edge_index"] = c["edge_index"][:, :g["total"] - 3]
        bad += [39]
    return c, bad


@pytest.mark.parametrize("what,bits", [
    (("offsets",), _lib.BATCH_BAD_OFFSETS | _lib.BATCH_OUT_OF_ENV), (("col",), _lib.BATCH_OUT_OF_ENV),
    (("order",), _lib.BATCH_OUT_OF_ENV), (("limit",), _lib.BATCH_TRUNCATED),
    (("offsets", "col", "order", "limit"), _lib.BATCH_BAD_OFFSETS | _lib.BATCH_OUT_OF_ENV | _lib.BATCH_TRUNCATED)])
def test_bad_data_is_reported_not_trusted(what, bits):
    g = _graph("n6")
    B, E = g["B"], g["E"]
    c, bad = _corrupt(g, what)
    conv = _conv(3, 16)
    w, w_e = (t.detach() for t in gnn.pack_conv_params(conv))
    with torch.no_grad():
        good = conv.forward_env(g)
        edgeless = conv.forward_env(dict(g, edge_ptr=torch.zeros_like(g["edge_ptr"])))
        out, ptr, status = gnn.env_conv(c["node_feat"], c["edge_ptr"], c["edge_index"], c["edge_attr"], w, w_e, 3, E,
                                        True, row_ptr=True, check=False)
        with pytest.raises(ValueError if bits & _lib.BATCH_TRUNCATED else RuntimeError):
            conv.forward_env(c)
    assert int(status.item()) == bits
    keep = torch.ones(B, dtype=torch.bool, device=DEV)
    keep[bad] = False
    _same(out[~keep], edgeless[~keep], "corrupt envs are edgeless")
    _same(out[keep], good[keep], "every other env unchanged")
    limit = c["edge_index"].shape[1]
    for b in bad:                                            # their offsets repeat the checked start
        start = min(max(int(c["edge_ptr"][b]), 0), limit)
        assert bool((ptr[b * E:(b + 1) * E] == start).all()), b
    csr = gnn.env_csr(g["edge_index"][:, :g["total"]], B * E)
    rows = keep.repeat_interleave(E)
    _same(ptr[:-1][rows], csr[:-1][rows], "offsets of the other envs")


def test_headline_size():
    """24 x 8192 after a reset, 3 x 16: the fused call and the existing
    TransformerConv.forward kernel path, both against fp64."""
    from gsmarl_amd import EnvConfig, GpuBatchEnv
    env = GpuBatchEnv(EnvConfig(n_agents=24, n_envs=8192, seed=1), DEV)
    out = env.reset(seed=1)
    n = env.B * env.E
    conv = _conv(3, 16)
    with torch.no_grad():
        fused = conv.forward_env(out)
        ptr = gnn.env_csr(out["edge_index"], n)
        composed = conv(out["node_feat"].reshape(n, 7), ptr, out["edge_index"][1].contiguous(),
                        out["edge_attr"].reshape(-1, 1))
    ref = _ref64(dict(out, E=env.E), conv).reshape(n, 48)
    e_fused, e_comp = _nerr(fused.reshape(n, 48), ref), _nerr(composed, ref)
    print(f"headline: fused {e_fused:.3e}  composed {e_comp:.3e}")
    assert e_fused <= 2e-5 and e_comp <= 2e-5
    env.close()


def test_rejections():
    nf = torch.zeros(2, 9, 7, device=DEV)
    ei = torch.zeros(2, 4, dtype=torch.int32, device=DEV)
    ea = torch.zeros(4, device=DEV)

    def call(nf, HC, heads):
        return gnn.env_conv(nf, torch.zeros(nf.shape[0] + 1, dtype=torch.int64, device=DEV), ei, ea,
                            torch.zeros(4, HC, 8, device=DEV), torch.zeros(HC, device=DEV), heads, nf.shape[1], True)
    assert call(nf, 48, 3).shape == (2, 9, 48)
    with pytest.raises(_lib.GsmError):
        call(nf, 48, 1)                                      # C = 48: not a power of two
    with pytest.raises(_lib.GsmError):
        call(nf, 128, 2)                                     # heads * channels > 64
    assert call(torch.zeros(1, 288, 7, device=DEV), 48, 3).shape == (1, 288, 48)
    with pytest.raises(_lib.GsmError):
        call(torch.zeros(1, 289, 7, device=DEV), 48, 3)      # E = 289


@pytest.mark.parametrize("kw,feats", [(dict(concat=False), 7), (dict(), 5)])
def test_other_layers_take_the_fallback(kw, feats):
    g = _graph("n6")
    B, E = g["B"], g["E"]
    gr = dict(g, node_feat=g["node_feat"][..., :feats].contiguous())
    torch.manual_seed(3)
    conv = gnn.TransformerConv(feats, 16, heads=3, **kw).to(DEV)
    with torch.no_grad():
        out = conv.forward_env(gr)
        csr = gnn.env_csr(g["edge_index"][:, :g["total"]], B * E)
        ref = conv(gr["node_feat"].reshape(B * E, feats), csr, g["edge_index"][1, :g["total"]].contiguous(),
                   g["edge_attr"][:g["total"]].reshape(-1, 1))
    assert out.shape == (B, E, ref.shape[1])
    assert torch.allclose(out.reshape(B * E, -1), ref, rtol=2e-5, atol=2e-5)
