"""The assignment kernel (gsm_ragged_kernels.hip: wave_lsa) started from caches
that do not belong to the state: tests/lsa_warm_cases.py, one env per case.

Through observe, step, a mixed batch and the fused rollout launch the kernel's
assignment must be scipy's on its own fp32 positions, and the kernel must do
what the CPU restatement (oracle/lsa_ref.py: warm_start_assignment) does, env
by env: the same certificate decision (lsa_stats) and the same column duals
written back, value for value. Caches in which several rows claim one column
are the exception (the kernel keeps one claimant, unspecified): for those only
scipy's assignment, a finite cache and a permutation are asserted.
"""
import collections
import functools

import numpy as np
import pytest
import torch
from scipy.optimize import linear_sum_assignment as scipy_lsa

import lsa_warm_cases as lc
from oracle import ragged_ref as rr
from oracle.lsa_ref import warm_start_assignment

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
# every buffer a rollout launch must leave as the eager steps do (test_gpu_roll_ragged.KEYS)
KEYS = ("pos", "vel", "step_count", "episode", "node_feat", "reward", "cost", "done", "edge_count",
        "edge_ptr", "ep_acc", "ep_last", "row_mask", "assign", "env_shape", "lsa_v", "lsa_col", "lsa_stats")
CACHE_KEYS = ("lsa_v", "lsa_col", "lsa_stats")
SCENARIOS = ("polygon", "line")


def _np(t):
    return t.detach().cpu().numpy()


@functools.lru_cache(maxsize=None)
def _cases(scenario, N):
    cs = lc.cases(scenario, N)
    cs["dup"] = np.array([lc.has_duplicate(c, N) for c in cs["col0"]])
    return cs


def _env(scenario, N, B, **kw):
    from gsmarl_amd import EnvConfig, GpuBatchEnv
    return GpuBatchEnv(EnvConfig(scenario=scenario, n_agents=N, n_envs=B, seed=1, **kw), DEV)


def _write_cache(env, v0, col0):
    env.t["lsa_v"].copy_(torch.from_numpy(v0))
    env.t["lsa_col"].copy_(torch.from_numpy(col0))
    env.t["lsa_stats"].zero_()


def _inject(env, cs):
    """The case layouts at rest, then the case caches (set_state observes, and
    so rewrites the cache: the cache is written after it)."""
    out = env.set_state(dict(pos=cs["pos"], vel=np.zeros_like(_np(env.t["vel"]))))
    if env.cfg.lsa_warm_start:
        _write_cache(env, cs["v0"], cs["col0"])
    return out


def _costs(scenario, N, pos):
    rcfg = lc.rcfg_for(scenario, N)
    return [rr.assignment(rcfg, lc.SCN[scenario], N, p)[1] for p in pos]


def _check_envs(env, Cs, v0, col0, dup, names, what):
    """Every env of a batch whose cache was (v0, col0) before ONE assignment
    on the cost matrices Cs. Returns certified counts by cache kind."""
    torch.cuda.synchronize()
    assign, v, colb, stats = (_np(env.t[k]) for k in ("assign", "lsa_v", "lsa_col", "lsa_stats"))
    bad = []
    cert_by = collections.Counter()
    for b, C32 in enumerate(Cs):
        n = C32.shape[0]
        C = C32.astype(np.float64)
        tag = (what, b) + tuple(names[b])
        if not np.array_equal(assign[b, :n], scipy_lsa(C)[1]):
            bad.append(tag + ("assign != scipy", assign[b, :n].tolist()))
        if not np.array_equal(colb[b, :n], assign[b, :n]):
            bad.append(tag + ("lsa_col != assign",))
        if dup[b]:
            if not (np.isfinite(v[b, :n]).all() and np.array_equal(np.sort(colb[b, :n]), np.arange(n))
                    and stats[b, 1] == 1):
                bad.append(tag + ("duplicate-cache invariants",))
            continue
        col, cert, v_out, _ = warm_start_assignment(C, v0[b, :n], col0[b, :n])
        cert_by[names[b][1]] += cert
        if not np.array_equal(assign[b, :n], col):
            bad.append(tag + ("assign != restatement",))
        if stats[b].tolist() != [int(cert), 1]:
            bad.append(tag + ("lsa_stats", stats[b].tolist(), "restatement certified", cert))
        if not np.array_equal(v[b, :n], v_out):
            bad.append(tag + ("lsa_v != restatement", float(np.abs(v[b, :n] - v_out).max())))
    assert not bad, (len(bad), bad[:12])
    return cert_by


def _names(cs):
    return list(zip(cs["state"], cs["cache"]))


def _report(what, cs, cert_by):
    tot = collections.Counter(c for c, d in zip(cs["cache"], cs["dup"]) if not d)
    print(f"{what} certified by cache:", {k: f"{cert_by[k]}/{tot[k]}" for k in tot})


@pytest.mark.parametrize("scenario", SCENARIOS)
@pytest.mark.parametrize("N", lc.N_LIST)
def test_observe_from_hostile_cache(scenario, N):
    cs = _cases(scenario, N)
    B = len(cs["state"])
    env = _env(scenario, N, B)
    env.reset(seed=1)
    _inject(env, cs)
    out = env.observe()
    assert np.array_equal(_np(env.t["pos"]), cs["pos"])
    Cs = _costs(scenario, N, _np(env.t["pos"]))
    assert all(np.array_equal(a, b) for a, b in zip(Cs, cs["C"]))
    cert_by = _check_envs(env, Cs, cs["v0"], cs["col0"], cs["dup"], _names(cs), f"observe {scenario} {N}")
    _report(f"observe {scenario} N={N}", cs, cert_by)
    if scenario == "polygon" and N == 2:
        assert cs["state"][-1] == "example" and np.array_equal(Cs[-1], lc.EXAMPLE_C)
        assert _np(out["assign"])[-1].tolist() == [0, 1] and _np(env.t["lsa_stats"])[-1].tolist() == [0, 1]
    # the written-back cache is the state's own: the same assignment again
    first = _np(out["assign"]).copy()
    out = env.observe()
    torch.cuda.synchronize()
    assert np.array_equal(_np(out["assign"]), first)
    assert np.array_equal(_np(env.t["lsa_stats"])[:, 1], np.full(B, 2))
    env.close()


def _actions(cs, N, seed):
    """Random action indices; the 2 x 2 example's agents hold still (index 0
    from rest: its cost matrix is the same after the step)."""
    a = np.random.default_rng(seed).integers(0, 5, (len(cs["state"]), N)).astype(np.int32)
    a[np.array(cs["state"]) == "example"] = 0
    return a


@pytest.mark.parametrize("scenario", SCENARIOS)
@pytest.mark.parametrize("N", lc.N_LIST)
def test_step_from_hostile_cache(scenario, N):
    cs = _cases(scenario, N)
    env = _env(scenario, N, len(cs["state"]))
    env.reset(seed=1)
    _inject(env, cs)
    out = env.step(torch.from_numpy(_actions(cs, N, N)).to(DEV))
    torch.cuda.synchronize()
    assert not _np(out["done"]).any()
    Cs = _costs(scenario, N, _np(env.t["pos"]))      # the kernel's own post-step fp32 positions
    _check_envs(env, Cs, cs["v0"], cs["col0"], cs["dup"], _names(cs), f"step {scenario} {N}")
    if scenario == "polygon" and N == 2:
        assert np.array_equal(Cs[-1], lc.EXAMPLE_C) and _np(out["assign"])[-1].tolist() == [0, 1]
    env.close()


@pytest.mark.parametrize("scenario", SCENARIOS)
@pytest.mark.parametrize("N", lc.N_LIST)
def test_cold_control(scenario, N):
    """lsa_warm_start=False: the same states give scipy's assignment with no
    cache bound, and nothing is counted."""
    cs = _cases(scenario, N)
    env = _env(scenario, N, len(cs["state"]), lsa_warm_start=False)
    env.reset(seed=1)
    _write_cache(env, cs["v0"], cs["col0"])          # unbound: must stay as written
    out = _inject(env, cs)
    torch.cuda.synchronize()
    assign = _np(out["assign"])
    for b, C32 in enumerate(cs["C"]):
        assert np.array_equal(assign[b], scipy_lsa(C32.astype(np.float64))[1]), (b, cs["state"][b])
    assert env.lsa_warm_stats() == (0, 0) and not _np(env.t["lsa_stats"]).any()
    assert np.array_equal(_np(env.t["lsa_v"]), cs["v0"], equal_nan=True)
    assert np.array_equal(_np(env.t["lsa_col"]), cs["col0"])
    env.close()


@pytest.mark.parametrize("fill", [23, 24, 31])
def test_mixed_batch_stale_columns(fill):
    """A mixed batch (N_env in 3..24) whose whole lsa_col rows hold one
    column, at or past most envs' own N (all rows claiming column 23 in an env
    of 24 is a duplicate cache). Navigation envs solve no assignment: their
    cache rows and counters stay as written."""
    from gsmarl_amd import EnvConfig, GpuBatchEnv
    B, N = 96, 24
    cfg = EnvConfig(scenario="mixed", n_agents=N, n_agents_min=3, n_envs=B, seed=6)
    keys = set(rr.br.DEFAULTS) | set(rr.RAGGED_DEFAULTS)
    rcfg = rr.make_cfg(**{k: v for k, v in cfg.to_dict().items() if k in keys})
    env = GpuBatchEnv(cfg, DEV)
    env.reset(seed=6)
    v0 = np.random.default_rng(fill).normal(size=(B, N))
    col0 = np.full((B, N), fill, np.int32)
    _write_cache(env, v0, col0)
    env.observe()
    torch.cuda.synchronize()
    sh = _np(env.t["env_shape"])
    n_b, scn_b = sh & 0xFF, sh >> 8
    assert len(set(n_b.tolist())) > 5 and (n_b == 24).any() and set(scn_b.tolist()) == {0, 1, 2}
    rs = rr.RSpec(rcfg)
    pos = _np(env.t["pos"])
    nav = scn_b == rr.SCN_NAV
    v, colb, stats = (_np(env.t[k]) for k in CACHE_KEYS)
    assert np.array_equal(v[nav], v0[nav]) and np.array_equal(colb[nav], col0[nav]) and not stats[nav].any()
    idx = np.flatnonzero(~nav)
    Cs = [rr.assignment(rcfg, scn_b[b], n_b[b], pos[b, rr.store_index(rs, scn_b[b], n_b[b])])[1] for b in idx]
    sub = _SubEnv(env, idx)
    _check_envs(sub, Cs, v0[idx], col0[idx], np.array([fill < n_b[b] for b in idx]),
                [(f"scn{scn_b[b]} n{n_b[b]}", "stale") for b in idx], f"mixed fill {fill}")
    for b in idx:                                     # past the env's own N: untouched
        assert np.array_equal(v[b, n_b[b]:], v0[b, n_b[b]:]) and np.all(colb[b, n_b[b]:] == fill), b
    env.close()


class _SubEnv:
    """the rows `idx` of an env's assignment buffers, for _check_envs"""

    def __init__(self, env, idx):
        sel = torch.from_numpy(idx).to(DEV)
        self.t = {k: env.t[k][sel] for k in ("assign",) + CACHE_KEYS}


@pytest.mark.parametrize("scenario,N", [("polygon", 2), ("polygon", 9), ("polygon", 17), ("polygon", 32),
                                        ("line", 8), ("line", 25)])
def test_rollout_launch_from_hostile_cache(scenario, N):
    """wave_lsa<true> (the rollout kernel's instantiation: cost column in LDS,
    pass chunks of 4): a 2-step rollout launch from the case states and caches
    leaves every buffer as two eager steps from the same states and caches do,
    the cache and its counters included."""
    cs = _cases(scenario, N)
    B, T = len(cs["state"]), 2
    env = _env(scenario, N, B)
    env.reset(seed=1)
    acts = torch.from_numpy(np.stack([_actions(cs, N, 100 + N), _actions(cs, N, 200 + N)])).to(DEV)
    _inject(env, cs)
    st0 = env.get_state()
    for t in range(T):
        env.step(acts[t], sync_edges=False)
    torch.cuda.synchronize()
    ref = {k: v.clone() for k, v in env.t.items()}
    assert not _np(ref["done"]).any()
    env.set_state(st0)
    _write_cache(env, cs["v0"], cs["col0"])
    env.capture(acts, T, slot=0, kernels="roll")
    assert env.graph_is_rollout(0)
    env.t["edge_index"].fill_(-7)
    env.replay(0)
    torch.cuda.synchronize()
    assert not env.roll_gave_up()
    keep = torch.from_numpy(~cs["dup"]).to(DEV)
    for k in KEYS:
        if k in CACHE_KEYS:
            assert torch.equal(ref[k][keep], env.t[k][keep]), k
        else:
            assert torch.equal(ref[k], env.t[k]), k
    n = int(ref["edge_ptr"][-1])
    assert torch.equal(ref["edge_index"][:, :n], env.t["edge_index"][:, :n])
    assert torch.equal(ref["edge_attr"][:n], env.t["edge_attr"][:n])
    # and the second step's assignment is scipy's on the final positions
    assign = _np(env.t["assign"])
    for b, C32 in enumerate(_costs(scenario, N, _np(env.t["pos"]))):
        assert np.array_equal(assign[b], scipy_lsa(C32.astype(np.float64))[1]), (b, cs["state"][b], cs["cache"][b])
    assert np.array_equal(_np(env.t["lsa_stats"])[:, 1], np.full(B, T))
    if scenario == "polygon" and N == 2:              # the example: cold, then certified from the healed cache
        assert assign[-1].tolist() == [0, 1] and _np(env.t["lsa_stats"])[-1].tolist() == [1, 2]
    env.close()
