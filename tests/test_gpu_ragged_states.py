"""The ragged kernels (polygon / line / mixed) from injected states
(tests/ragged_states.py), not from a reset layout. The family implements one
env step three times — the eager kernels (gsm_step_ragged_kernel<false> +
gsm_emit_ragged_kernel), the lagged chain (gsm_step_ragged_kernel<true>) and
the fused rollout (gsm_roll_ragged_kernel) — over one sweep that forms every
predicate by integer arithmetic on the bits of d2 in two 32-column words. The
states put the work where a reset layout has none:

 crowd      edge lists on both sides of the rollout's LDS cap (its long-list
            branch, straight into the slab), long rows in ragged_expand and its
            walk over the obstacle columns of word 1, several contacts per
            agent in both column words, overflowing rollout-buffer slots;
 lattice    pairs of every kind at d2 == R2 bit for bit and one ulp to either
            side, across the word boundary, at M = 32, 34 and 64;
 touching   d2 == dmin2 (no collision: strict) and one ulp inside;
 coincident an agent on an agent and on an obstacle of word 1, in a navigation,
            a polygon and a line env, the last env and a partial workgroup;
            strict mode's NaN envs and their -1 assignments;
 staggered  envs that re-lay out on the first, a middle and the last step;
 padding    positions planted in the unused rows of an env with n < Nmax.

tests/test_ragged_states_ref.py shows with the oracle alone that the states are
these cases. Eager steps are held to oracle/ragged_ref.py at test_gpu_ragged's
bars (no new tolerance); the chain and the rollout to the eager steps bit for
bit, every buffer, the degenerate flags and contact_mask included; and the
last step of a crowd's launch to the fp64 oracle directly, so that an error
shared by the three cannot hide."""
import os

import numpy as np
import pytest
import torch

import ragged_states as gs
from oracle import ragged_ref as rr
from parity_tol import check_state
from test_gpu_ragged import _ostate, check_observation, check_reward_cost
from test_gpu_roll_ragged import KEYS as ROLL_KEYS

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
# every state and output buffer of the env; contact_mask is never written on the
# ragged path (gsm_internal.h: segmented path only) and must stay as allocated
KEYS = tuple(ROLL_KEYS) + tuple(k for k in ("degenerate", "contact_mask") if k not in ROLL_KEYS)
NAMES = sorted(gs.CONFIGS)
FMT_CODE = {"onehot": 0, "index": 1, "cont": 2}


def _cases(name):
    """The injected states of a config: (case id, builder arguments)."""
    out = ["crowd", "lattice0", "lattice+", "lattice-", "touching", "staggered"]
    seen = []
    for w in gs.wheres(name):
        envs = gs.where_envs(gs.make_cfg(name), w)
        if envs not in seen:        # (`partial` is `last` where the last workgroup is full or holds one env)
            seen.append(envs)
            out.append("coincident-" + w)
    return out


ALL = [(n, c) for n in NAMES for c in _cases(n)]


def _build(name, case):
    """(state, K, episode length) of a case."""
    cfg = gs.make_cfg(name)
    if case == "crowd":
        return gs.crowd(cfg), gs.K, 1000
    if case.startswith("lattice"):
        return gs.lattice(cfg, {"0": 0, "+": 1, "-": -1}[case[-1]]), gs.K, 1000
    if case == "touching":
        return gs.touching(cfg), gs.K, 1000
    if case.startswith("coincident-"):
        return gs.coincident(cfg, case.split("-")[1]), gs.K, 1000
    if case == "staggered":
        return gs.staggered(gs.crowd(cfg), gs.EL_STAG, gs.K_STAG), gs.K_STAG, gs.EL_STAG
    raise ValueError(case)


def _env(name, **kw):
    from gsmarl_amd import EnvConfig, GpuBatchEnv
    cfg = EnvConfig(**dict(gs.CONFIGS[name], **kw))
    keys = set(rr.br.DEFAULTS) | set(rr.RAGGED_DEFAULTS)
    rcfg = rr.make_cfg(**{k: v for k, v in cfg.to_dict().items() if k in keys})
    return GpuBatchEnv(cfg, DEV), rcfg


def _np(t):
    return t.detach().cpu().numpy()


def _actions(st, T, fmt="index", seed=1):
    """(device action rows [T,B,N(,k)], the same rows in numpy); the held
    agents' action is the no-op in each format."""
    B, N = st["hold"].shape
    idx = gs.actions(T, B, N, seed=seed, hold=st["hold"])
    if fmt == "index":
        a = idx
    elif fmt == "onehot":
        a = np.eye(5, dtype=np.float32)[idx]
    else:
        a = np.random.default_rng(7).uniform(-1.0, 1.0, (T, B, N, 2)).astype(np.float32)
        a[:, st["hold"]] = 0.0
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV), a


def _pad_mask(env):
    """[B,E] bool: the rows no entity of the env uses."""
    sh = _np(env.t["env_shape"])
    n, scn = sh & 0xFF, sh >> 8
    rs = rr.RSpec(rr.make_cfg(scenario=env.cfg.scenario, n_agents=env.N, n_envs=env.B))
    m = np.ones((env.B, env.E), bool)
    for b in range(env.B):
        m[b, rr.store_index(rs, int(scn[b]), int(n[b]))] = False
    return m


def _inject(env, st, plant=False):
    """reset, an empty assignment warm-start cache (equal runs start from equal
    caches), then the state through set_state. plant: the state's padding rows
    written into the bound position buffer afterwards (set_state's observation
    writes zeros there, as a reset does)."""
    env.reset(seed=env.cfg.seed)
    env.t["lsa_v"].zero_()
    env.t["lsa_col"].fill_(-1)
    env.t["lsa_stats"].zero_()
    out = env.set_state({k: torch.from_numpy(st[k]) for k in ("pos", "vel", "step_count")})
    torch.cuda.synchronize()
    if plant:
        m = torch.from_numpy(_pad_mask(env)).to(DEV)
        assert bool(m.any()) and not bool(env.t["pos"][m].any())
        env.t["pos"][m] = torch.from_numpy(st["pos"]).to(DEV)[m]
        torch.cuda.synchronize()
    return out


def _bits(t):
    return t.view(torch.int32) if t.dtype == torch.float32 else t


def _snapshot(env):
    torch.cuda.synchronize()
    out = {k: env.t[k].clone() for k in KEYS}
    n = int(out["edge_ptr"][-1])
    out["edge_index"] = env.t["edge_index"][:, :n].clone()
    out["edge_attr"] = env.t["edge_attr"][:n].clone()
    return out


def _run_eager(env, st, acts, T, replays=1, plant=False):
    _inject(env, st, plant)
    for t in range(replays * T):
        env.step(acts[(t % T) % acts.shape[0]], sync_edges=False)
    return _snapshot(env)


def _run_graph(env, st, acts, T, kernels, replays=1, plant=False):
    _inject(env, st, plant)
    slot = 1 if kernels == "roll" else 0
    env.capture(acts, T, slot=slot, kernels=kernels)
    assert env.graph_is_rollout(slot) == (kernels == "roll")
    env.t["edge_index"].fill_(-7)
    for _ in range(replays):
        env.replay(slot)
    torch.cuda.synchronize()
    assert env.roll_gave_up() == 0
    return _snapshot(env)


def _same(ref, got, what):
    for k in ref:
        assert torch.equal(_bits(ref[k]), _bits(got[k])), (what, k)


def _paths_equal(name, st, T, EL, fmt="index", replays=1, plant=False, **kw):
    """The lagged chain and the rollout launch against eager steps from the
    same injected state: every buffer bit for bit. Returns the rollout's."""
    env, _ = _env(name, episode_length=EL, **kw)
    acts, _ = _actions(st, T, fmt)
    ref = _run_eager(env, st, acts, T, replays, plant)
    for kernels in ("both", "roll"):
        got = _run_graph(env, st, acts, T, kernels, replays, plant)
        _same(ref, got, (name, kernels, fmt, replays))
    env.close()
    return got


def _check_degenerate(env, rcfg, out, ost):
    rs = rr.RSpec(rcfg)
    want = np.zeros(env.B, np.uint8)
    for b in range(env.B):
        n, scn, pc = rr._compact(rs, ost, b)
        want[b] = rr.degenerate_env(scn, n, pc)
    assert np.array_equal(_np(out["degenerate"]), want), "degenerate"
    return want


def _eager_against_oracle(name, st, T, EL, fmt="index", plant=False):
    """set_state's observation and every one of T eager steps against
    oracle/ragged_ref.py from the kernel's own fp32 state before the step."""
    env, rcfg = _env(name, episode_length=EL)
    acts, acts_np = _actions(st, T, fmt)
    out = _inject(env, st, plant)
    ost = check_observation(env, rcfg, out)
    check_reward_cost(env, rcfg, out)
    deg = _check_degenerate(env, rcfg, out, ost)
    flagged = deg.copy()
    for t in range(T):
        prev = _ostate(env, rcfg)
        out = env.step(acts[t])
        torch.cuda.synchronize()
        st64, ob64 = rr.step(rcfg, prev, acts_np[t], FMT_CODE[fmt], np.float64)
        check_state(_np(env.t["pos"]), st64["pos"], f"pos {name}")
        check_state(_np(env.t["vel"]), st64["vel"], f"vel {name}")
        done = _np(out["done"])
        assert np.array_equal(done, ob64["done"]), t
        assert np.array_equal(_np(env.t["step_count"]), st64["step"]), t
        assert np.array_equal(_np(env.t["episode"]), st64["episode"]), t
        ost = check_observation(env, rcfg, out)
        check_reward_cost(env, rcfg, out, envs=np.nonzero(done == 0)[0])
        flagged |= _check_degenerate(env, rcfg, out, ost)
    env.close()
    return flagged, _np(out["cost"])


# ------------------------------------------------- eager against the oracle
@pytest.mark.parametrize("name,case", ALL)
def test_eager_against_the_oracle(name, case):
    st, T, EL = _build(name, case)
    flagged, cost = _eager_against_oracle(name, st, T, EL)
    if case.startswith("coincident-"):
        envs = gs.where_envs(gs.make_cfg(name), case.split("-")[1])
        assert flagged[envs].all() and not np.delete(flagged, envs).any()
    else:
        assert not flagged.any()
    if case.startswith("lattice"):
        assert not cost.any()


@pytest.mark.parametrize("fmt", ["onehot", "cont"])
def test_eager_action_formats_against_the_oracle(fmt):
    st, T, EL = _build("M24", "crowd")
    _eager_against_oracle("M24", st, T, EL, fmt=fmt)


# ---------------------------------- lagged chain and rollout against eager
@pytest.mark.parametrize("name,case", ALL)
def test_chain_and_rollout_equal_eager(name, case):
    st, T, EL = _build(name, case)
    got = _paths_equal(name, st, T, EL)
    if case.startswith("lattice"):
        # a fixed point: the injected positions unmoved (live rows)
        cfg = gs.make_cfg(name)
        n_b, scn_b, rs = gs.shapes(cfg)
        p = _np(got["pos"])
        for b in range(len(n_b)):
            idx = rr.store_index(rs, scn_b[b], n_b[b])
            assert np.array_equal(p[b, idx].view(np.int32), st["pos"][b, idx].view(np.int32)), b
        assert not bool(got["cost"].any())
    if case.startswith("coincident-"):
        envs = gs.where_envs(gs.make_cfg(name), case.split("-")[1])
        deg = _np(got["degenerate"])
        assert (deg[envs] == 1).all() and not np.delete(deg, envs).any()
    if case == "staggered":
        assert bool(got["done"][2]) and not bool(got["done"].all())   # a re-layout on the launch's last step
        assert len(np.unique(_np(got["episode"]))) >= 2


@pytest.fixture
def depth(request):
    old = os.environ.get("GSM_ROLL_DEPTH")
    if request.param is not None:
        os.environ["GSM_ROLL_DEPTH"] = str(request.param)
    yield request.param
    if old is None:
        os.environ.pop("GSM_ROLL_DEPTH", None)
    else:
        os.environ["GSM_ROLL_DEPTH"] = old


@pytest.mark.parametrize("depth", [2, 8], indirect=True)
def test_crowd_pack_depths(depth):
    """Pack depths 2 and 8 (8 > K: every step's edges packed by the tail)."""
    st, T, EL = _build("M24", "crowd")
    _paths_equal("M24", st, T, EL)


@pytest.mark.parametrize("name", ["M24", "M32"])
def test_crowd_two_replays_back_to_back(name):
    st, T, EL = _build(name, "crowd")
    _paths_equal(name, st, T, EL, replays=2)


@pytest.mark.parametrize("fmt", ["onehot", "cont"])
def test_crowd_action_formats(fmt):
    st, T, EL = _build("M24", "crowd")
    _paths_equal("M24", st, T, EL, fmt=fmt)


@pytest.mark.parametrize("name", ["M24", "M32"])
def test_crowd_shared_reward(name):
    st, T, EL = _build(name, "crowd")
    _paths_equal(name, st, T, EL, shared_reward=True)


# ------------------------------------------------------------ padding rows
@pytest.mark.parametrize("name", ["M24", "M17"])
def test_planted_padding_rows_are_ignored(name):
    """set_state's observation leaves zeros in the rows no entity uses
    (_inject asserts it); crowd positions written there afterwards change
    nothing the sweep, the expansion, the emission or the assignment compute:
    eager steps against the oracle, the chain and the rollout against eager."""
    st, T, EL = _build(name, "crowd")
    _eager_against_oracle(name, st, T, EL, plant=True)
    _paths_equal(name, st, T, EL, plant=True)


# ------------------------------------------------------------ oracle parity
@pytest.mark.parametrize("name", ["M24", "M32"])
def test_crowd_last_step_against_the_oracle(name):
    """The last step of a crowd's rollout launch against the fp64 oracle
    stepped from the eager fp32 state after K - 1 steps: positions and
    velocities within the 1e-6 bar, counters exact; edges, assignments, node
    features, costs and flags exact against the fp32-mode oracle on the
    rollout's own positions."""
    st, T, EL = _build(name, "crowd")
    env, rcfg = _env(name, episode_length=EL)
    acts, acts_np = _actions(st, T)
    _inject(env, st)
    for t in range(T - 1):
        env.step(acts[t], sync_edges=False)
    torch.cuda.synchronize()
    prev = _ostate(env, rcfg)
    nst, ob64 = rr.step(rcfg, prev, acts_np[T - 1], 1, np.float64)
    _run_graph(env, st, acts, T, "roll")
    for what in ("pos", "vel"):
        e64 = np.abs(_np(env.t[what]).astype(np.float64) - nst[what]).max()
        print(f"{name}: {what} max |rollout - fp64 oracle| {e64:.3e}")
    check_state(_np(env.t["pos"]), nst["pos"], f"pos roll {name}")
    check_state(_np(env.t["vel"]), nst["vel"], f"vel roll {name}")
    assert np.array_equal(_np(env.t["step_count"]), nst["step"])
    assert np.array_equal(_np(env.t["episode"]), nst["episode"])
    assert np.array_equal(_np(env.t["done"]), ob64["done"])
    out = env.outputs()
    ost = check_observation(env, rcfg, out)
    check_reward_cost(env, rcfg, out)
    _check_degenerate(env, rcfg, out, ost)
    env.close()


# -------------------------------------------------------------- strict mode
@pytest.mark.parametrize("name,where", [(n, w) for n in ("M24", "P10") for w in gs.wheres(n)])
def test_coincident_strict_mode_nan_bits(name, where):
    """strict_degenerate: MPE's NaN for the coincident pairs, spreading to
    the env's agents; a polygon / line env with a NaN agent has no assignment
    (-1) and a NaN reward. The chain's and the rollout's NaN bits and
    assignments are the eager steps'; NaN only in the chosen envs."""
    cfg = gs.make_cfg(name)
    n_b, scn_b, _ = gs.shapes(cfg)
    st = gs.coincident(cfg, where)
    envs = gs.where_envs(cfg, where)
    got = _paths_equal(name, st, gs.K, 1000, strict_degenerate=True)
    p, asg, rew = _np(got["pos"]), _np(got["assign"]), _np(got["reward"])
    for b in range(len(n_b)):
        n = int(n_b[b])
        if b in envs:
            assert np.isnan(p[b, :n]).all(), b
            if scn_b[b] != rr.SCN_NAV:
                assert (asg[b, :n] == -1).all() and np.isnan(rew[b, :n]).all(), b
        else:
            assert np.isfinite(p[b]).all() and np.isfinite(rew[b]).all(), b
            if scn_b[b] != rr.SCN_NAV:
                assert sorted(asg[b, :n].tolist()) == list(range(n)), b
    deg = _np(got["degenerate"])
    assert (deg[envs] & 2).all() and not np.delete(deg, envs).any()


# ------------------------------------------------- slots smaller than a step
@pytest.mark.parametrize("name,small", [("M24", True), ("M24", False), ("M17", False), ("M32", False)])
def test_crowd_into_buffer_slots(name, small):
    """A rollout buffer on the M24 crowd with the default slot (8 edges per
    entity: the crowd's first slots overflow it) and with the worst case (none
    does), filled by one rollout launch (roll_edge_sink<true>, pack's guard)
    and by eager step_into on a twin env: every slot the same true offsets,
    counts, node features, rewards, costs, done flags and assignments, the
    same first min(edges, cap) edges, and nothing written past them (the rest
    of each slot, which borders the next slot's, keeps its fill). The slots
    keep the edges of every step of the launch, not only the last one's: the
    M17 crowd's lists exceed the LDS cap in its first steps only."""
    from gsmarl_amd import GraphRolloutBuffer
    T = gs.K
    env, rcfg = _env(name, episode_length=1000)
    ref, _ = _env(name, episode_length=1000)
    st = gs.crowd(gs.make_cfg(name), L=gs.SLOT_L if name == "M24" else None)
    acts, _ = _actions(st, T)
    per = None if small else int(env.sizes.max_edges_per_env)
    gb = GraphRolloutBuffer(env, episode_length=T, edges_per_env=per)
    eb = GraphRolloutBuffer(ref, episode_length=T, edges_per_env=per)
    for buf, e in ((gb, env), (eb, ref)):
        buf.edge_index.fill_(-7)
        buf.edge_attr.fill_(-7.0)
        _inject(e, st)
        e.observe(out=buf.slot(0))
        buf.step = 0
    gb.capture(acts)
    assert env.graph_is_rollout(0)
    gb.replay()
    gb.validate()
    for t in range(T):
        eb.insert(acts[t])
    torch.cuda.synchronize()
    for k in ("edge_ptr", "edge_count", "node_feat", "reward", "cost", "done", "assign"):
        assert torch.equal(_bits(getattr(gb, k)), _bits(getattr(eb, k))), k
    cap = gb.cap
    over = []
    for t in range(T + 1):
        total = int(gb.edge_ptr[t, env.B])
        n = min(total, cap)
        over.append(total > cap)
        assert torch.equal(gb.edge_index[t][:, :n], eb.edge_index[t][:, :n]), t
        assert torch.equal(_bits(gb.edge_attr[t][:n]), _bits(eb.edge_attr[t][:n])), t
        for buf in (gb, eb):
            assert bool((buf.edge_index[t][:, n:] == -7).all()), t
            assert bool((buf.edge_attr[t][n:] == -7.0).all()), t
    # the true offsets are the oracle's (a truncated slot keeps them)
    ob = rr.observe(rcfg, gs.ostate(rcfg, st))
    assert np.array_equal(_np(gb.edge_ptr[0]), ob["edge_ptr"])
    assert bool(gb.overflowed()) == small and bool(eb.overflowed()) == small
    assert (over[0] and over[1] and not all(over)) if small else not any(over)
    env.close()
    ref.close()
