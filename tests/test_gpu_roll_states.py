"""The fused rollout kernels from injected states (tests/roll_states.py), not
from a reset layout: crowds (nearly every agent in several contacts, edge
lists near their capacity: the contact walk with many candidates, the first
step's candidate list, the list scans and the staging fallback of a long
list), spread states with entities at |x| >= 8, a lattice with every kind of
pair exactly at d2 == R2 and one ulp to either side, coincident agent-agent
and agent-obstacle pairs in either half of a wave, in both, in a lone last env
and in a partial workgroup (the kernels' coincident fallbacks; strict mode's
NaNs), and crowds whose envs re-lay out on different steps of the launch, the
first and the last included. tests/test_roll_states_ref.py shows with the
oracle alone that the states are these cases.

Every case runs one rollout launch and compares every state and output buffer
(the degenerate flags included; floats by their bits, so NaNs compare) with
the per-step chain of the same actions from the same injected state, and
requires the roll status to be 0. Kernels: the two-envs-per-wave kernel (24
agents, plain config), the generic kernel (shared reward, speed clamp, strict
mode), the plain kernel at 12 and 6 agents, the packed kernels at 3 agents
(the split one, and past its 8192 envs the unsplit one: pack_big) and the tile
rollout (96 agents). So that an error shared by the
chain and the rollout cannot hide, the last step of a crowd's launch is also
compared with the fp64 oracle stepped from the chain's state before it."""
import numpy as np
import pytest
import torch

import roll_states as rs
from oracle import batch_ref as br
from parity_tol import check_state

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
KEYS = ("pos", "vel", "step_count", "episode", "node_feat", "reward", "cost", "done", "edge_count",
        "edge_ptr", "ep_acc", "ep_last", "row_mask", "contact_mask", "degenerate")
SEED = 29
K = rs.K
MAX_SPEED = 0.3
GENERIC = {"shared_reward": dict(shared_reward=True), "max_speed": dict(max_speed=MAX_SPEED),
           "strict": dict(strict_degenerate=True)}


def _env(N, B, **kw):
    from gsmarl_amd import EnvConfig, GpuBatchEnv
    cfg = EnvConfig(n_agents=N, n_envs=B, seed=SEED, **kw)
    return GpuBatchEnv(cfg, DEV), cfg


def _ocfg(N, B, **kw):
    from gsmarl_amd import EnvConfig
    cfg = EnvConfig(n_agents=N, n_envs=B, seed=SEED, **kw)
    return br.make_cfg(**{k: v for k, v in cfg.to_dict().items() if k in br.DEFAULTS})


def _dev_actions(idx, hold, fmt):
    """The action rows on the device in one of the three formats; the held
    agents' is the no-op in each."""
    a = torch.from_numpy(idx).to(DEV)
    if fmt == "index":
        return a.contiguous()
    if fmt == "onehot":
        return torch.nn.functional.one_hot(a.long(), 5).to(torch.float32).contiguous()
    T, B, N = idx.shape
    u = np.random.default_rng(7).uniform(-1.0, 1.0, (T, B, N, 2)).astype(np.float32)
    u[:, hold] = 0.0
    return torch.from_numpy(u).to(DEV).contiguous()


def _inject(env, st):
    env.reset(seed=SEED)
    env.set_state({k: torch.from_numpy(st[k]) for k in ("pos", "vel", "step_count")})
    torch.cuda.synchronize()


def _bits(t):
    return t.view(torch.int32) if t.dtype == torch.float32 else t


def _snapshot(env):
    out = {k: env.t[k].clone() for k in KEYS}
    n = int(out["edge_ptr"][-1])
    out["edge_index"] = env.t["edge_index"][:, :n].clone()
    out["edge_attr"] = env.t["edge_attr"][:n].clone()
    return out


def _run(env, st, acts, T, kernels, replays=1):
    _inject(env, st)
    slot = 1 if kernels == "roll" else 0
    env.capture(acts, T, slot=slot, kernels=kernels)
    assert env.graph_is_rollout(slot) == (kernels == "roll")
    for _ in range(replays):
        env.replay(slot)
    torch.cuda.synchronize()
    assert env.roll_gave_up() == 0
    return _snapshot(env)


def _check(N, B, st, T=K, fmt="index", replays=1, seed=0, **kw):
    """Rollout launch == per-step chain from the injected state, every buffer."""
    env, _ = _env(N, B, **kw)
    acts = _dev_actions(rs.actions(T, B, N, seed=seed, hold=st["hold"]), st["hold"], fmt)
    ref = _run(env, st, acts, T, "both", replays)
    got = _run(env, st, acts, T, "roll", replays)
    for k in ref:
        assert torch.equal(_bits(ref[k]), _bits(got[k])), (k, N, B, T, fmt, kw)
    env.close()
    return got


def _crowd(shape):
    N, B = rs.SHAPES[shape]
    return N, B, rs.crowd(N, N, B, seed=N + B)


# ------------------------------------------------------------------ crowds
@pytest.mark.parametrize("shape", ["pair", "seg12", "seg6", "pack", "pack_big", "tile"])
def test_crowd_equals_chain(shape):
    N, B, st = _crowd(shape)
    _check(N, B, st, seed=N + B, episode_length=1000)


@pytest.mark.parametrize("flag", sorted(GENERIC))
def test_crowd_generic_kernel_equals_chain(flag):
    N, B, st = _crowd("generic")
    if flag == "max_speed":
        # the clamp fires with the contact forces present: unclamped, the
        # oracle's first step exceeds the limit (as test_roll_flag_equals_chain)
        acts = rs.actions(K, B, N, seed=N + B)
        _, v1 = br.physics(_ocfg(N, B, max_speed=0.0), st["pos"].astype(np.float64), st["vel"].astype(np.float64),
                           acts[0], 1, np.float64)
        assert (np.hypot(v1[..., 0], v1[..., 1]) > MAX_SPEED).mean() > 0.5
    got = _check(N, B, st, seed=N + B, episode_length=1000, **GENERIC[flag])
    if flag == "max_speed":
        assert float(torch.linalg.norm(got["vel"], dim=-1).max()) <= MAX_SPEED + 1e-6


@pytest.mark.parametrize("fmt", ["onehot", "cont"])
@pytest.mark.parametrize("shape", ["pair", "pack", "pack_big"])
def test_crowd_action_formats(shape, fmt):
    N, B, st = _crowd(shape)
    _check(N, B, st, fmt=fmt, seed=N + B, episode_length=1000)


@pytest.mark.parametrize("shape", ["pair", "pack", "pack_big", "tile"])
def test_spread_equals_chain(shape):
    N, B = rs.SHAPES[shape]
    _check(N, B, rs.spread(N, N, B, seed=N), seed=N, episode_length=1000)


@pytest.mark.parametrize("shape", ["pair", "pack", "pack_big", "seg12"])
def test_staggered_crowd_equals_chain(shape):
    N, B, st = _crowd(shape)
    got = _check(N, B, rs.staggered(st, rs.EL_STAG, rs.K_STAG), T=rs.K_STAG, seed=N + B,
                 episode_length=rs.EL_STAG)
    ep = got["episode"].cpu().numpy()
    assert (ep[0:B - 1:2] != ep[1:B:2]).any()   # a wave's two envs re-laid out on different steps
    assert bool(got["done"][2]) and not bool(got["done"].all())   # a re-layout on the launch's last step


# ------------------------------------------------------------------ lattice
@pytest.mark.parametrize("kernel", ["pair", "generic"])
@pytest.mark.parametrize("nudge", [0, 1, -1])
def test_lattice_ties_equal_chain_and_oracle(nudge, kernel):
    """Pairs of every kind at d2 == R2 (inclusive), one ulp outside and one
    inside, at every step of the launch: the chain's bytes, the fp32 oracle's
    edges, and the injected positions unmoved."""
    N, B = rs.SHAPES[kernel]
    kw = dict(shared_reward=True) if kernel == "generic" else {}
    st = rs.lattice(N, N, B, nudge)
    got = _check(N, B, st, episode_length=1000, **kw)
    assert torch.equal(_bits(got["pos"].cpu()), _bits(torch.from_numpy(st["pos"])))
    ptr, ei, _ = br.edges(_ocfg(N, B, **kw), st["pos"], np.float32)
    assert np.array_equal(got["edge_ptr"].cpu().numpy(), ptr)
    assert np.array_equal(got["edge_index"].cpu().numpy(), ei)
    assert not bool(got["cost"].any())


# --------------------------------------------------------------- coincident
def _coincident(shape, where, strict=False):
    N, B = rs.SHAPES[shape]
    if shape == "pair" and where == "partial":
        B = rs.B_PARTIAL
    epb = 1 if shape == "tile" else 8 if shape == "pair" else 4
    return N, B, rs.coincident(N, N, B, where, seed=N, envs_per_block=epb), rs.where_envs(where, B, epb)


def _assert_still_coincident(got, st, envs, N):
    p = got["pos"].cpu().numpy()
    assert np.isfinite(p).all()
    rest = np.setdiff1d(np.arange(p.shape[0]), envs)
    for b in envs:
        assert np.array_equal(p[b, 7], p[b, 3]) and np.array_equal(p[b, 5], p[b, 2 * N + 2])
        assert np.array_equal(p[b, [3, 5]], st["pos"][b, [3, 5]])
    deg = got["degenerate"].cpu().numpy()
    assert (deg[envs] == 1).all() and not deg[rest].any()


@pytest.mark.parametrize("where", rs.WHERE)
@pytest.mark.parametrize("shape", ["pair", "tile"])
def test_coincident_pairs_equal_chain(shape, where):
    """The coincident fallback of the rollout's sweep at every step of the
    launch: counted collisions, no radius edge, no contact force."""
    N, B, st, envs = _coincident(shape, where)
    got = _check(N, B, st, seed=N, episode_length=1000)
    _assert_still_coincident(got, st, envs, N)
    pos = got["pos"].cpu().numpy()
    ptr, ei, _ = br.edges(_ocfg(N, B), pos, np.float32)
    assert np.array_equal(got["edge_ptr"].cpu().numpy(), ptr)
    assert np.array_equal(got["edge_index"].cpu().numpy(), ei)
    _, c = br.reward_cost(_ocfg(N, B), pos, np.float32)
    assert np.array_equal(got["cost"].cpu().numpy(), c)
    assert (c[envs][:, [3, 7, 5]] == 1.0).all()


@pytest.mark.parametrize("where", rs.WHERE)
def test_coincident_pairs_strict_mode_nan_bits_equal_chain(where):
    """strict_degenerate: MPE's NaN for the coincident pairs, spreading to the
    env's agents; the rollout's NaN bits are the chain's. (A reset layout
    holds no coincident pair: there strict mode equals the default.)"""
    N, B, st, envs = _coincident("generic", where)
    got = _check(N, B, st, seed=N, episode_length=1000, strict_degenerate=True)
    p = got["pos"].cpu().numpy()
    rest = np.setdiff1d(np.arange(B), envs)
    assert np.isnan(p[envs][:, :N]).all() and np.isfinite(p[rest]).all()


@pytest.mark.parametrize("where", ["both", "last"])
def test_coincident_pairs_two_replays_back_to_back(where):
    N, B, st, envs = _coincident("pair", where)
    got = _check(N, B, st, replays=2, seed=N, episode_length=1000)
    _assert_still_coincident(got, st, envs, N)


# ------------------------------------------------------------ oracle parity
@pytest.mark.parametrize("shape", ["pair", "pack", "seg12", "tile"])
def test_crowd_last_step_against_the_oracle(shape):
    """The last step of a crowd's rollout launch against the fp64 oracle
    stepped from the chain's fp32 state after K - 1 steps (test_gpu_roll's
    test_roll_oracle_direct, from a crowd several steps old): positions and
    velocities within the 1e-6 bar, counters and done exact, the CSR edges and
    the costs exact against the fp32-mode oracle on the kernel's positions."""
    N, B, st = _crowd(shape)
    env, _ = _env(N, B, episode_length=1000)
    ocfg = _ocfg(N, B, episode_length=1000)
    idx = rs.actions(K, B, N, seed=N + B)
    acts = _dev_actions(idx, st["hold"], "index")
    _inject(env, st)
    env.capture(acts, K - 1, slot=0, kernels="both")
    env.replay(0)
    torch.cuda.synchronize()
    s = {k: v.detach().cpu().numpy() for k, v in env.get_state().items()}
    ref_st = dict(pos=s["pos"].astype(np.float64), vel=s["vel"].astype(np.float64), step=s["step_count"],
                  episode=s["episode"], ep_acc=s["ep_acc"].astype(np.float64), ep_last=s["ep_last"].astype(np.float64))
    nst, ob = br.step(ocfg, ref_st, idx[K - 1], 1, np.float64, seed=SEED)
    c = br.reward_cost(ocfg, s["pos"], np.float32)[1]
    print(f"{shape}: agents in a collision before the last step {float((c > 0).mean()):.2f}")
    got = _run(env, st, acts, K, "roll")
    got = {k: v.cpu().numpy() for k, v in got.items()}
    for what in ("pos", "vel"):
        e64 = np.abs(got[what].astype(np.float64) - nst[what]).max()
        print(f"{shape}: {what} max |rollout - fp64 oracle| {e64:.3e}")
    check_state(got["pos"], nst["pos"], "pos roll")
    check_state(got["vel"], nst["vel"], "vel roll")
    assert np.array_equal(got["step_count"], nst["step"])
    assert np.array_equal(got["episode"], nst["episode"])
    assert np.array_equal(got["done"].astype(bool), ob["done"].astype(bool))
    print(f"{shape}: reward max |rollout - fp64 oracle| {np.abs(got['reward'] - ob['reward']).max():.3e}")
    assert np.allclose(got["reward"], ob["reward"], rtol=3e-7, atol=2e-6)
    ptr, ei, _ = br.edges(ocfg, got["pos"], np.float32)
    assert np.array_equal(got["edge_ptr"], ptr)
    assert np.array_equal(got["edge_index"], ei)
    keep = ~ob["done"].astype(bool)
    _, c32 = br.reward_cost(ocfg, got["pos"][keep], np.float32)
    assert np.array_equal(got["cost"][keep], c32)
    env.close()

