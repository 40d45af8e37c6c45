"""Guard bands around the env itself: every tensor a GpuBatchEnv binds
(gsm_bind) moved into an arena of tests/guard.py and bound again, and an
ordinary twin env that runs the same calls. After every call (a) no band has
changed and every tensor of env.t has the twin's bits (the edge arrays up to
edge_ptr[B]).

A bound buffer is read and written by the kernels, so its bands hold legal
values, not a byte pattern: NaN around float arrays (a stray read shows in the
twin comparison), 0 around the integer arrays and masks, -1 around assign and
lsa_col (the "no slot" / "no column" values of include/gsm.h). Actions, the
reset mask and the state handed to set_state come from arenas under fill A
and fill B (index actions 0 / 4, mask 0 / 1, floats NaN / 1e30); get_state's
outputs are the wrapper's own torch.empty_like under guarded_allocations and
are held to (a), (b) and the twin's bits from both prefills.

test_env_calls, per shape: reset(seed); reset(env_mask) of the last env
alone; in each action format the K action rows stepped eagerly under fill A
and again under fill B (2K steps a format); observe; set_state; get_state; a
captured per-step chain and a fused rollout launch of K steps (no such launch
exists for the tile row sweep: there the capture has to be refused). Shapes: the
seven of roll_states.SHAPES, (70, 9) (a tile shape with no compiled rollout
size of its own), (200, 2) (the tile row sweep) and ragged_states.CONFIGS with
and without lsa_warm_start. The episode length is 4, so envs re-lay out inside
the launches.

test_redirected_outputs: step(out=), observe(out=) and GraphRolloutBuffer
capture / replay into rollout-buffer fields held in arenas, at the full
capacity and at edges_per_env=2, where every slot is truncated: the band after
the last slot's edge_attr and after row 1 of its edge_index shows that the
truncation holds at the end of the buffer as it does between slots.

Exceptions of (b): the edge arrays past min(edge_ptr[B], capacity).
include/gsm.h: "edges past edge_capacity are not written, while edge_ptr keeps
the true offsets", and edge_index / edge_attr are arrays of edge_capacity of
which a step fills edge_ptr[B] entries."""
import ctypes as C

import pytest
import torch

import guard as G
import ragged_states as gs
import roll_states as rs
from gsmarl_amd import EnvConfig, GpuBatchEnv, GraphRolloutBuffer, _lib

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
K = rs.K
EL = 4
SEED = 29
NAV = dict(rs.SHAPES, tile70=(70, 9), tile_rows=(200, 2))
NAV_KW = {"generic": dict(shared_reward=True)}
CASES = [(name, None) for name in NAV] + [(name, warm) for name in sorted(gs.CONFIGS) for warm in (True, False)]
MINUS_ONE = ("assign", "lsa_col")
NO_ROLL = ("tile_rows",)         # the tile path's row sweep has no fused rollout kernel (gsm.h, GSM_GRAPH_ROLL)


def _cfg(name, warm):
    if name in NAV:
        N, B = NAV[name]
        return EnvConfig(n_agents=N, n_envs=B, seed=SEED, episode_length=EL, **NAV_KW.get(name, {}))
    return EnvConfig(**dict(gs.CONFIGS[name], episode_length=EL, lsa_warm_start=warm))


def _band(name, t):
    if t.dtype.is_floating_point:
        return float("nan"), float("nan")
    return (-1, -1) if name in MINUS_ONE else (0, 0)


def _guarded_env(cfg):
    """A GpuBatchEnv whose bound tensors all live in arenas; (env, guard)."""
    env = GpuBatchEnv(cfg, DEV)
    g = G.Guard()
    env.t = {k: g.state(t, _band(k, t), k) for k, t in env.t.items()}
    ptrs = {k: env.t[k].data_ptr() for k in _lib.BUFFER_FIELDS}
    if not cfg.lsa_warm_start:
        ptrs["lsa_v"] = ptrs["lsa_col"] = None
    bufs = _lib.GsmBuffers(**ptrs)
    _lib.check(env.lib, env.lib.gsm_bind(env._h, C.byref(bufs)), env._h, "gsm_bind")
    assert all(t.data_ptr() % 256 == 0 for t in env.t.values())
    return env, g


def _same(env, twin, g, what):
    torch.cuda.synchronize()
    g.check()
    n = int(twin.t["edge_ptr"][-1])
    assert n == int(env.t["edge_ptr"][-1]) and n <= env.t["edge_attr"].numel(), what
    for k, b in twin.t.items():
        a = env.t[k]
        if k == "edge_index":
            a, b = a[:, :n], b[:, :n]
        elif k == "edge_attr":
            a, b = a[:n], b[:n]
        assert G.same_bits(a, b), f"{what}: {k} differs from the twin's"


def _actions(env, st_hold, fmt, seed):
    idx = torch.from_numpy(rs.actions(K, env.B, env.N, seed=seed, hold=st_hold)).to(DEV)
    if fmt == "index":
        return idx.contiguous(), lambda f: G.actions(f, 5)
    if fmt == "onehot":
        return torch.nn.functional.one_hot(idx.long(), 5).to(torch.float32).contiguous(), G.floats
    u = torch.rand(K, env.B, env.N, 2, device=DEV, generator=torch.Generator(device=DEV).manual_seed(seed)) * 2 - 1
    u[idx == 0] = 0.0
    return u.contiguous(), G.floats


def _state(name, env):
    if name in NAV:
        No = env.E - 2 * env.N
        return rs.crowd(env.N, No, env.B, L=rs.CROWD_L.get(env.N, 0.3), seed=env.N + env.B)
    return gs.crowd(gs.make_cfg(name))


@pytest.mark.parametrize("name,warm", CASES,
                         ids=[n if w is None else f"{n}-{'warm' if w else 'cold'}" for n, w in CASES])
def test_env_calls(name, warm):
    """gsm_reset, gsm_step, gsm_observe, gsm_set_state, gsm_get_state, gsm_graph_capture and
    gsm_graph_launch on bound buffers in arenas."""
    cfg = _cfg(name, warm)
    env, g = _guarded_env(cfg)
    twin = GpuBatchEnv(_cfg(name, warm), DEV)
    _same(env, twin, g, "bind")
    B = env.B
    for e in (env, twin):
        e.reset(seed=SEED)
    _same(env, twin, g, "reset(seed)")
    mask = torch.zeros(B, dtype=torch.uint8, device=DEV)
    mask[B - 1] = 1
    for fill in "AB":
        env.reset(env_mask=g.input(mask, G.flags(fill), f"mask {fill}"))
        twin.reset(env_mask=mask)
        _same(env, twin, g, f"reset(env_mask), fill {fill}")
    st = _state(name, env)
    for f_i, fmt in enumerate(("index", "onehot", "cont")):
        seq, fills = _actions(env, st["hold"], fmt, seed=f_i)
        for fill in "AB":
            for j in range(K):
                env.step(g.input(seq[j], fills(fill), f"{fmt} actions {j} {fill}"), sync_edges=False)
                twin.step(seq[j], sync_edges=False)
                _same(env, twin, g, f"step {j}, {fmt} actions, fill {fill}")
    for e in (env, twin):
        e.observe(sync_edges=False)
    _same(env, twin, g, "observe")
    # set_state from arenas, get_state into arenas
    src = {k: torch.from_numpy(st[k]).to(DEV) for k in ("pos", "vel", "step_count")}
    for fill in "AB":
        band = {k: (G.floats(fill) if v.dtype.is_floating_point else G.counts(fill, EL - 1)) for k, v in src.items()}
        env.set_state({k: g.input(v, band[k], f"state {k} {fill}") for k, v in src.items()}, sync_edges=False)
        twin.set_state(src, sync_edges=False)
        _same(env, twin, g, f"set_state, fill {fill}")
    want = twin.get_state()
    for prefill in (0, 1):
        g2 = G.Guard(prefill)
        with G.guarded_allocations(g2):
            got = env.get_state()
        torch.cuda.synchronize()
        g2.check()
        assert set(got) == set(want)
        for k, v in got.items():
            assert g2.owns(v) and not bool(g2.unwritten(v).any()), (k, prefill)
            assert G.same_bits(v, want[k]), (k, prefill)
    _same(env, twin, g, "get_state")
    # a captured per-step chain, then one fused rollout launch, the action rows in an arena
    seq, fills = _actions(env, st["hold"], "index", seed=7)
    for fill in "AB":
        rows = g.input(seq, fills(fill), f"action rows {fill}")
        for slot, kernels in ((0, "both"), (1, "roll")):
            if kernels == "roll" and name in NO_ROLL:
                with pytest.raises(_lib.GsmError, match="no fused rollout kernel"):
                    env.capture(rows, K, slot=slot, kernels=kernels)
                continue
            for e, a in ((env, rows), (twin, seq)):
                e.capture(a, K, slot=slot, kernels=kernels)
                assert e.graph_is_rollout(slot) == (kernels == "roll")
                e.replay(slot)
            torch.cuda.synchronize()
            assert env.roll_gave_up() == 0 and twin.roll_gave_up() == 0
            _same(env, twin, g, f"captured {kernels}, fill {fill}")
    env.close()
    twin.close()


def _guarded_buffer(env, g, T, per_env):
    buf = GraphRolloutBuffer(env, episode_length=T, edges_per_env=per_env)
    for k in buf.FIELDS + (("assign",) if buf.ragged else ()):
        t = getattr(buf, k)
        setattr(buf, k, g.state(t, _band(k, t), f"buffer {k}"))
    return buf


def _same_buffer(buf, ref, g, what):
    torch.cuda.synchronize()
    g.check()
    for k in buf.FIELDS + (("assign",) if buf.ragged else ()):
        a, b = getattr(buf, k), getattr(ref, k)
        if k in ("edge_index", "edge_attr"):
            for t in range(buf.T + 1):
                n = min(int(ref.edge_ptr[t, buf.B]), buf.cap)
                assert G.same_bits(a[t][..., :n], b[t][..., :n]), f"{what}: slot {t} of {k} differs from the twin's"
        else:
            assert G.same_bits(a, b), f"{what}: {k} differs from the twin's"


@pytest.mark.parametrize("per_env", ["max", 2], ids=["full", "truncated"])
@pytest.mark.parametrize("name,warm", [("pair", None), ("pack", None), ("tile", None), ("M24", True)])
def test_redirected_outputs(name, warm, per_env):
    """gsm_observe_into and gsm_step_into (GraphRolloutBuffer.reset / insert), gsm_graph_capture_into and its
    launch (capture / replay) writing rollout-buffer fields in arenas."""
    T = 3
    env, g = _guarded_env(_cfg(name, warm))
    twin = GpuBatchEnv(_cfg(name, warm), DEV)
    per_env = int(env.sizes.max_edges_per_env) if per_env == "max" else per_env
    buf, ref = _guarded_buffer(env, g, T, per_env), GraphRolloutBuffer(twin, episode_length=T, edges_per_env=per_env)
    acts = torch.from_numpy(rs.actions(T, env.B, env.N, seed=3)).to(DEV)
    st = _state(name, env)
    src = {k: torch.from_numpy(st[k]).to(DEV) for k in ("pos", "vel", "step_count")}
    for b, e in ((buf, env), (ref, twin)):
        b.reset(seed=SEED)
        e.set_state(src, sync_edges=False)                   # a crowd: long edge lists
        e.observe(out=b.slot(0))
    _same_buffer(buf, ref, g, "observe(out=)")
    if per_env == 2:
        assert int(ref.edge_ptr[0, env.B]) > ref.cap == 2 * env.B                        # slot 0 is truncated
    else:
        assert not bool(ref.overflowed())
    for t in range(T):
        for b in (buf, ref):
            b.insert(acts[t])
        _same_buffer(buf, ref, g, f"step(out=) into slot {t + 1}")
    _same(env, twin, g, "eager steps into the buffer")
    if per_env == 2:
        assert bool((ref.edge_ptr[:, env.B] > ref.cap).all())                            # and so is every other slot
    # the same episode again as one captured launch from the same start
    for b, e in ((buf, env), (ref, twin)):
        b.step = 0
        e.set_state(src, sync_edges=False)
        e.observe(out=b.slot(0))
        b.capture(acts)
        b.replay()
    torch.cuda.synchronize()
    assert env.graph_is_rollout(0) == twin.graph_is_rollout(0)
    assert env.roll_gave_up() == 0 and twin.roll_gave_up() == 0
    _same_buffer(buf, ref, g, "capture / replay")
    _same(env, twin, g, "capture / replay")
    env.close()
    twin.close()
