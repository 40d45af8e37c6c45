"""Assignment states and warm-start caches for the wave_lsa tests (numpy only).

The assignment kernel starts from a per-env cache (gsm.h lsa_v / lsa_col: the
column duals and matching of the env's last assignment). The cases here pair
agent layouts of a polygon or line env with caches that do not belong to the
layout: what a checkpoint restore, an uninitialised buffer or an auto-reset
leaves behind. tests/test_lsa_warm_ref.py runs them through the CPU
restatement (oracle/lsa_ref.py: warm_start_assignment) against scipy;
tests/test_gpu_lsa_warm.py runs the same cases through the kernel, one env per
case. Every case is deterministic from (scenario, N, rep).

State kinds (compact positions [N + T, 2] fp32: agents, then the T targets):
  generic       agents uniform over the layout square
  near_slot     agents within ~1e-6 of the slots (matched costs ~1e-6, their
                float64 ulps far below the certificate's 1e-11 / 1e-9)
  half_stacked  the first N // 2 agents at one point, some copies one fp32 ulp off
  grid          agents on a grid of pitch 1/4, nudged by 0 or +-2^-24
  stacked       all agents at one point                    (identical rows)
  centre        all agents on the polygon centre / line midpoint (identical rows)
  on_slots      agents exactly on the slots, permuted: a unique optimum of
                cost 0 (zeros on the matching, slot distances elsewhere)
  example       N = 2 polygon only: the 2 x 2 matrix of the wrong certificate
                (EXAMPLE_C), with its cache v0 = [1e16, 0]

Cache kinds: no cache (zero), N(0, 1) duals, the duals and matching of a
neighbouring problem (costs perturbed by 1e-3) as written, with a common offset
inside the kernel's dual bound (+100) and outside it (+2^27), and staggered by
1e-10 per column; a random permutation, scipy's answer, out-of-range and
duplicate columns for lsa_col; duals with +-1e6 .. 1e16 on some columns, a
common 1e9, +-1e308, inf, NaN, and all duals exactly at the bound.
"""
import numpy as np

from oracle import ragged_ref as rr
from oracle.lsa_ref import DUAL_MAX, warm_start_assignment

N_LIST = (1, 2, 7, 8, 9, 16, 17, 24, 25, 32)
STATE_KINDS = ("generic", "near_slot", "half_stacked", "grid", "stacked", "centre", "on_slots")
TIE_KINDS = ("stacked", "centre")            # every row of C identical: no unique optimum for N >= 2
# caches: zero .. neighbour are the ones a certified warm start is expected from
CACHE_KINDS = ("zero", "normal", "neighbour", "neighbour_off", "neighbour_2p27", "perm", "scipy", "out_of_range",
               "duplicate", "stagger", "mixed_1e6", "mixed_1e9", "mixed_1e12", "mixed_1e16", "common_1e9",
               "huge", "inf", "nan", "at_bound")
BAR_STATES, BAR_CACHES = ("generic", "near_slot"), ("zero", "normal", "neighbour")
NONFINITE = ("inf", "nan")
SCN = {"polygon": rr.SCN_POLYGON, "line": rr.SCN_LINE}

EXAMPLE_C = np.array([[0.35355347, 0.79056942], [1.0, 1.41421354]], np.float32)
EXAMPLE_POS = np.array([[0.25, 0.25 + 2.0 ** -23], [0.5, 1.0], [0.0, 0.0]], np.float32)   # two agents, the centre
EXAMPLE_V0 = np.array([1e16, 0.0])


def rcfg_for(scenario, N, n_envs=1):
    return rr.make_cfg(scenario=scenario, n_agents=N, n_envs=n_envs)


def cost_matrix(rcfg, scn, N, pos_c):
    """C [N, N] fp32 as the kernel forms it (oracle.ragged_ref.assignment)."""
    pa = np.asarray(pos_c[:N], np.float32)
    s = rr.slots(rcfg, scn, N, pos_c[N:])
    dx = pa[:, None, 0] - s[None, :, 0]
    dy = pa[:, None, 1] - s[None, :, 1]
    return np.sqrt(dx * dx + dy * dy).astype(np.float32)


def state(rcfg, scn, N, kind, rng):
    T = rr.n_targets(scn, N)
    L = float(rr.half_width(rcfg, N))
    tg = rng.uniform(-L, L, (T, 2)).astype(np.float32)
    p = rng.uniform(-L, L, (N, 2)).astype(np.float32)
    sl = rr.slots(rcfg, scn, N, tg)
    if kind == "near_slot":
        p = (sl[rng.permutation(N)] + (rng.normal(size=(N, 2)) * 1e-6).astype(np.float32)).astype(np.float32)
    elif kind == "half_stacked":
        p[: N // 2] = p[0]
        for i in range(1, N // 2):
            if rng.random() < 0.5:
                p[i, 0] = np.nextafter(p[i, 0], np.float32(4), dtype=np.float32)
    elif kind == "grid":
        p = (np.round(p * 4) / 4).astype(np.float32)
        p = (p + rng.integers(-1, 2, p.shape).astype(np.float32) * np.float32(2.0 ** -24)).astype(np.float32)
    elif kind == "stacked":
        p[:] = p[0]
    elif kind == "centre":
        p[:] = tg[0] if T == 1 else ((tg[0] + tg[1]) * np.float32(0.5)).astype(np.float32)
    elif kind == "on_slots":
        p = sl[rng.permutation(N)].copy()
    elif kind == "example":
        return EXAMPLE_POS.copy()
    elif kind != "generic":
        raise ValueError(kind)
    return np.concatenate([p, tg]).astype(np.float32)


def _mixed(rng, N, mag):
    """N(0, 1) duals with +-mag added to about two columns of three"""
    s = rng.choice([-1.0, 0.0, 1.0], size=N)
    if not s.any():
        s[rng.integers(N)] = 1.0
    return rng.normal(size=N) + s * mag


def cache(kind, C, rng):
    """(v0 [N] float64, col0 [N] int32) of one kind for the fp32 matrix C."""
    N = C.shape[0]
    c64 = C.astype(np.float64)
    none = np.full(N, -1, np.int32)
    if kind in ("neighbour", "neighbour_off", "neighbour_2p27", "scipy", "duplicate", "stagger"):
        c2 = (C + (rng.normal(size=C.shape) * 1e-3).astype(np.float32)).astype(np.float32)
        _, _, nv, ncol = warm_start_assignment(np.abs(c2).astype(np.float64), np.zeros(N), none)
    if kind == "zero":
        return np.zeros(N), none
    if kind == "normal":
        return rng.normal(size=N), none
    if kind == "neighbour":
        return nv, ncol.astype(np.int32)
    if kind == "neighbour_off":                     # a common offset inside the bound
        return nv + 100.0, ncol.astype(np.int32)
    if kind == "neighbour_2p27":                    # and one far outside
        return nv + 2.0 ** 27, ncol.astype(np.int32)
    if kind == "perm":
        return np.zeros(N), rng.permutation(N).astype(np.int32)
    if kind == "scipy":
        from scipy.optimize import linear_sum_assignment as scipy_lsa
        return nv, scipy_lsa(c64)[1].astype(np.int32)
    if kind == "out_of_range":                      # negative, >= N, >= 32, the int32 extremes
        pool = np.array([-5, -1, N, N + 1, 32, 33, 1000, 2 ** 31 - 1, -2 ** 31], np.int64)
        col = rng.permutation(N).astype(np.int64)
        bad = rng.random(N) < 0.6
        bad[rng.integers(N)] = True
        col[bad] = rng.choice(pool, size=int(bad.sum()))
        return rng.normal(size=N), col.astype(np.int32)
    if kind == "duplicate":                         # several rows claim one column
        col = ncol.copy()
        if N >= 2:
            k = rng.permutation(N)
            col[k[1:1 + max(1, N // 3)]] = col[k[0]]
        return nv, col.astype(np.int32)
    if kind == "stagger":                           # duals 1e-10 apart, on equal rows too
        return nv + 1e-10 * np.arange(N), ncol.astype(np.int32)
    if kind.startswith("mixed_"):
        return _mixed(rng, N, float(kind[6:])), rng.permutation(N).astype(np.int32)
    if kind == "common_1e9":
        return 1e9 + rng.normal(size=N), none
    if kind == "huge":
        v = rng.choice([-1e308, 1e308, 0.0, 1e16], size=N)
        v[rng.integers(N)] = 1e308
        return v, rng.permutation(N).astype(np.int32)
    if kind == "at_bound":                          # passes the gate; the duals it leads to need not
        return np.full(N, DUAL_MAX), none
    if kind in NONFINITE:
        v = rng.normal(size=N)
        v[rng.integers(N)] = np.inf if kind == "inf" else np.nan
        if kind == "inf" and N > 1:
            v[(int(np.flatnonzero(~np.isfinite(v))[0]) + 1) % N] = -np.inf
        return v, rng.permutation(N).astype(np.int32)
    raise ValueError(kind)


def cases(scenario, N, reps=1, state_kinds=STATE_KINDS, cache_kinds=CACHE_KINDS, seed=0):
    """Every state kind x cache kind, `reps` times, as arrays over the cases:
    pos [B, N + T, 2] f32, C [B, N, N] f32, v0 [B, N] f64, col0 [B, N] i32, and
    the lists state / cache (kind names). The polygon N = 2 list ends with the
    2 x 2 example."""
    scn = SCN[scenario]
    rcfg = rcfg_for(scenario, N)
    out = dict(pos=[], C=[], v0=[], col0=[], state=[], cache=[])

    def add(sk, ck, pos_c, v0, col0):
        out["pos"].append(pos_c)
        out["C"].append(cost_matrix(rcfg, scn, N, pos_c))
        out["v0"].append(v0)
        out["col0"].append(col0)
        out["state"].append(sk)
        out["cache"].append(ck)

    for rep in range(reps):
        for sk in state_kinds:
            rng = np.random.default_rng([seed, scn, N, rep, STATE_KINDS.index(sk)])
            pos_c = state(rcfg, scn, N, sk, rng)
            C = cost_matrix(rcfg, scn, N, pos_c)
            for ck in cache_kinds:
                v0, col0 = cache(ck, C, np.random.default_rng([seed, scn, N, rep, STATE_KINDS.index(sk),
                                                               CACHE_KINDS.index(ck)]))
                add(sk, ck, pos_c, v0, col0)
    if scenario == "polygon" and N == 2:
        add("example", "example", EXAMPLE_POS.copy(), EXAMPLE_V0.copy(), np.full(2, -1, np.int32))
    for k in ("pos", "C", "v0", "col0"):
        out[k] = np.stack(out[k])
    out["col0"] = out["col0"].astype(np.int32)
    return out


def exceeds_bound(v0):
    """the cached duals fail the kernel's gate (non-finite, or beyond DUAL_MAX)"""
    return not bool(np.all(np.abs(v0) <= DUAL_MAX))


def has_equal_rows(C):
    """two agents with the same cost row: swapping their slots costs nothing,
    so no optimum is unique"""
    return len(np.unique(C, axis=0)) < C.shape[0]


def has_duplicate(col0, N):
    c = col0[(col0 >= 0) & (col0 < N)]
    return len(np.unique(c)) < len(c)
