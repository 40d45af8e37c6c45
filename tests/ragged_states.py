"""Injected start states for the ragged kernels (polygon / line / mixed; numpy
and oracle/ragged_ref.py only), in the style of tests/roll_states.py.

A reset layout plus a few random steps is sparse: about 100 edges in an env
that can hold 2304, a few percent of the agents in a collision, no pair at the
sensing radius, no two entities in one place. The builders here give the
states where the ragged sweep (two 32-column words), the candidate walk, the
edge expansion (long rows, the obstacle columns of word 1, lists past the
assignment's LDS) and the coincident fallback do the most work. Each takes a
config of CONFIGS (by name) and returns padded ``pos`` [B,Emax,2] f32, ``vel``
[B,Nmax,2] f32, ``step_count`` [B] i32 (what set_state takes) and ``hold``
[B,Nmax] bool: agents whose action has to be the no-op in every action row.
Every builder is deterministic from its seed. Padding rows (an env with n <
Nmax agents) are filled with positions among the env's live entities, so a
kernel that read one would find neighbours there.
tests/test_ragged_states_ref.py shows with the oracle alone that the states are
the cases they claim to be.

Storage rows of an env (oracle/ragged_ref.py): agents [0, Nmax), targets
[Nmax, Nmax + Tmax), obstacles [Nmax + Tmax, Emax). Collider column c of an env
with n agents: agent c for c < n, obstacle c - n otherwise.
"""
import numpy as np

from oracle import ragged_ref as rr

# name -> config (seed: the one that draws the shapes below; seeds 0..39 were
# searched with find_seed and the first hit kept)
CONFIGS = {
    # n = [22, 18, 24, 16, 20, 22, 22, 20, 22, 4, 22, 17, 5, 8], scenario = env id mod 3: navigation envs of
    # 22, 16, 22, 4 and 5 agents (M = 44, 32, 44, 8, 10); 14 envs: the last workgroup of four waves half full
    "M24": dict(scenario="mixed", n_agents=24, n_agents_min=3, seed=0, n_envs=14),
    # navigation 16, 16, 17 (M = 32, 32, 34: word 1 empty, empty, two columns), polygon 16, 16, 17, line 17, 17, 17
    "M17": dict(scenario="mixed", n_agents=17, n_agents_min=16, seed=1, n_envs=9),
    # all 32: navigation envs of M = 64 (every lane a row, both words full)
    "M32": dict(scenario="mixed", n_agents=32, n_agents_min=31, seed=0, n_envs=6),
    "P10": dict(scenario="polygon", n_agents=10, n_agents_min=10, seed=0, n_envs=5),
    "L7": dict(scenario="line", n_agents=7, n_agents_min=7, seed=0, n_envs=5),
}
SHAPES = {   # what the seeds above give (test_ragged_states_ref checks)
    "M24": [22, 18, 24, 16, 20, 22, 22, 20, 22, 4, 22, 17, 5, 8],
    "M17": [16, 16, 17, 16, 16, 17, 17, 17, 17],
    "M32": [32] * 6,
    "P10": [10] * 5,
    "L7": [7] * 5,
}
MIXED = ("M24", "M17", "M32")
K = 5                           # steps of a launch
K_STAG, EL_STAG = 10, 4         # the staggered cases: launch and episode length
# half-widths of the crowd by Nmax (0.3 gives the mixed batches lists on both sides of the LDS cap, at least
# half the agents in a collision and a quarter in several; a 10-agent polygon and a 7-agent line have no
# obstacles and need a smaller box for that: chosen with the oracle, test_ragged_states_ref)
CROWD_L = {24: 0.3, 17: 0.3, 32: 0.3, 10: 0.2, 7: 0.12}
CROWD_SEED = 1
# the M24 crowd whose first slots overflow a rollout buffer's default slot (8 edges per entity: 8064 at 14
# envs; L = 0.3 stays just under it with 7950 edges, 0.2 starts with 8904 and 8160)
SLOT_L = 0.2
PITCH = 0.5                     # lattice pitch = the sensing radius: R2 = 0.25 exactly
WAVES_PER_BLOCK = 4             # one env per wave, four waves per workgroup
WHERE = ("nav", "polygon", "line", "last", "partial")


def make_cfg(name, **kw):
    """oracle config of CONFIGS[name] (episode_length etc. through kw)."""
    return rr.make_cfg(**dict(CONFIGS[name], **kw))


def shapes(cfg):
    """(n [B], scn [B], RSpec) of the batch."""
    n, scn = rr.env_shapes(cfg, int(cfg.seed))
    return n.astype(np.int64), scn.astype(np.int64), rr.RSpec(cfg)


def find_seed(base, want, seeds=range(40)):
    """The first seed whose mixed batch has the per-env agent counts `want`."""
    for s in seeds:
        cfg = rr.make_cfg(**dict(base, seed=s))
        if rr.env_shapes(cfg, s)[0].tolist() == list(want):
            return s
    return None


def lsa_lds_bytes(nmax):
    """gsm_internal.h: the assignment's LDS per wave (cost rows at an odd
    stride, padded to 16 bytes; column duals, row duals, a column scratch)."""
    n8 = (nmax + 7) & ~7
    stride = n8 | 1
    cost = 4 * n8 * stride
    return ((cost + 15) & ~15) + 16 * 32 + 4 * 32


def lds_edge_cap(nmax):
    """The longest edge list the rollout expands in LDS; longer ones go straight
    into the slab (gsm_roll_ragged_kernel, publish). 759 at Nmax = 24 and 17,
    1215 at 32, 431 at 10, 231 at 7."""
    return lsa_lds_bytes(nmax) // 4 - 1


def collider_rows(rs, scn, n):
    """Storage rows of the env's colliders in column order."""
    return np.concatenate([np.arange(n), rs.Nmax + rs.Tmax + np.arange(rr.n_obstacles(scn, n))]).astype(np.int64)


def target_rows(rs, scn, n):
    return (rs.Nmax + np.arange(rr.n_targets(scn, n))).astype(np.int64)


def padding_rows(rs, scn, n):
    return np.setdiff1d(np.arange(rs.Emax), rr.store_index(rs, scn, n))


def _state(pos, vel, B, Nmax):
    return dict(pos=np.ascontiguousarray(pos, np.float32), vel=np.ascontiguousarray(vel, np.float32),
                step_count=np.zeros(B, np.int32), hold=np.zeros((B, Nmax), bool))


def _plant_padding(cfg, pos, seed):
    """Padding rows uniform in the bounding box of the env's live rows."""
    n_b, scn_b, rs = shapes(cfg)
    rng = np.random.default_rng(10_000 + seed)
    for b in range(pos.shape[0]):
        live = pos[b, rr.store_index(rs, scn_b[b], n_b[b])]
        pad = padding_rows(rs, scn_b[b], n_b[b])
        pos[b, pad] = rng.uniform(live.min(0), live.max(0), (len(pad), 2)).astype(np.float32)


def crowd(cfg, L=None, seed=CROWD_SEED):
    """Every row (padding included) uniform in [-L, L]^2, velocities standard
    normal: every entity of an env inside a box of a few contact distances."""
    _, _, rs = shapes(cfg)
    L = CROWD_L[rs.Nmax] if L is None else L
    B = int(cfg.n_envs)
    rng = np.random.default_rng(seed)
    pos = rng.uniform(-L, L, size=(B, rs.Emax, 2)).astype(np.float32)
    vel = rng.normal(size=(B, rs.Nmax, 2)).astype(np.float32)
    return _state(pos, vel, B, rs.Nmax)


# ------------------------------------------------------------------ lattice
# The env's colliders fill a grid row by row, collider c in cell (c mod W,
# c div W). Grid columns stand in pairs (2k, 2k + 1) one pitch apart, the
# pairs three pitches from each other: a horizontal neighbour pair is always
# (even, odd), and nudging the odd columns moves every such pair the same way.
# Vertical neighbours are one pitch apart and are never nudged. With W = 9 the
# colliders 31 and 32 form a horizontal pair (cells 4 and 5 of row 3), and the
# colliders 23..31 stand above 32..40: tied pairs across the two column words.
def lattice_width(M):
    return 9 if M >= 18 else 3


def lattice_cells(M):
    """(grid column, grid row) of every collider column."""
    W = lattice_width(M)
    c = np.arange(M)
    return np.stack([c % W, c // W], -1)


def lattice_pairs(M):
    """(nudged, fixed): collider column pairs (i, j), i < j, one pitch apart
    horizontally (moved by a nudge) and vertically (never moved)."""
    W = lattice_width(M)
    nudged = [(c, c + 1) for c in range(M - 1) if (c % W) % 2 == 0 and (c + 1) % W != 0]
    fixed = [(c, c + W) for c in range(M - W)]
    return nudged, fixed


def lattice(cfg, nudge=0):
    """Live colliders on a grid of pitch 0.5 = sense_radius at coordinates that
    are multiples of 0.5 (env b shifted by a multiple of the pitch): neighbours
    at d2 == R2 bit for bit, diagonals outside, nobody in contact; zero
    velocity and the no-op for everyone, so every step sees the same ties.
    nudge = +1 / -1 moves the odd grid columns by one ulp in x away from /
    toward their even partner: every horizontal pair just outside / just
    inside. Targets lie off the grid lines."""
    assert nudge in (0, 1, -1)
    n_b, scn_b, rs = shapes(cfg)
    B = int(cfg.n_envs)
    pos = np.zeros((B, rs.Emax, 2), np.float32)
    for b in range(B):
        n, scn = int(n_b[b]), int(scn_b[b])
        rows = collider_rows(rs, scn, n)
        cells = lattice_cells(len(rows))
        xu = 3 * (cells[:, 0] // 2) + cells[:, 0] % 2
        x = (PITCH * (xu + 1 + b % 3)).astype(np.float32)
        y = (PITCH * (cells[:, 1] + 1 + (2 * b) % 3)).astype(np.float32)
        if nudge:
            odd = cells[:, 0] % 2 == 1
            x[odd] = np.nextafter(x[odd], np.float32(np.inf if nudge > 0 else -np.inf))
        pos[b, rows, 0], pos[b, rows, 1] = x, y
        tr = target_rows(rs, scn, n)
        if scn == rr.SCN_NAV:       # goal i beside agent i, off the grid
            pos[b, tr] = pos[b, :n] + np.float32([0.13, 0.21])
        else:                       # the centre / the line's ends inside the grid
            pos[b, tr] = (np.float32([[1.37, 1.12], [3.61, 2.83]]) + np.float32(0.5 * (b % 3)))[:len(tr)]
    _plant_padding(cfg, pos, 1)
    st = _state(pos, np.zeros((B, rs.Nmax, 2), np.float32), B, rs.Nmax)
    st["hold"][:] = True
    return st


# ----------------------------------------------------------------- touching
def touching(cfg):
    """Per env: agents 0, 1 exactly at d == fl32(s_i + s_j) (d2 == dmin2: not a
    collision, the test is strict) and agents 2, 3 one ulp inside (a collision
    each). Navigation envs: obstacle 0 exactly at the agent-obstacle distance
    from agent 0 and obstacle 1 one ulp inside it from agent 2. One member of
    each pair has x = 0 and both the same y, so dx is the planted value and dy
    is 0 exactly. Everyone else a unit grid away, zero velocity, held."""
    n_b, scn_b, rs = shapes(cfg)
    B = int(cfg.n_envs)
    sa, so = np.float32(cfg.agent_size), np.float32(cfg.obstacle_size)
    d_aa, d_ao = np.float32(sa + sa), np.float32(sa + so)
    zero = np.float32(0)
    pos = np.zeros((B, rs.Emax, 2), np.float32)
    for b in range(B):
        n, scn = int(n_b[b]), int(scn_b[b])
        assert n >= 4
        rows = collider_rows(rs, scn, n)
        k = np.arange(len(rows))
        pos[b, rows, 0] = 3.0 + (k % 8)           # the others: a unit grid far from x = 0
        pos[b, rows, 1] = -4.0 + (k // 8)
        y0, y1 = np.float32(1.0 + b), np.float32(-2.0 - b)
        pos[b, 0], pos[b, 1] = (zero, y0), (d_aa, y0)
        pos[b, 2], pos[b, 3] = (zero, y1), (np.nextafter(d_aa, zero), y1)
        if scn == rr.SCN_NAV:
            o = rs.Nmax + rs.Tmax
            pos[b, o], pos[b, o + 1] = (-d_ao, y0), (-np.nextafter(d_ao, zero), y1)
        tr = target_rows(rs, scn, n)
        if scn == rr.SCN_NAV:
            pos[b, tr] = pos[b, :n] + np.float32([0.31, 0.27])
        else:
            pos[b, tr] = np.float32([[1.5, 0.3], [-1.2, -0.7]])[:len(tr)]
    _plant_padding(cfg, pos, 2)
    st = _state(pos, np.zeros((B, rs.Nmax, 2), np.float32), B, rs.Nmax)
    st["hold"][:] = True
    return st


# --------------------------------------------------------------- coincident
def where_envs(cfg, where):
    """The envs of a `where`: the first navigation / polygon / line env, the
    batch's last env, the first env of the last workgroup where that one is
    partial (else the last env)."""
    _, scn_b, _ = shapes(cfg)
    B = int(cfg.n_envs)
    by = {"nav": rr.SCN_NAV, "polygon": rr.SCN_POLYGON, "line": rr.SCN_LINE}
    if where in by:
        envs = np.nonzero(scn_b == by[where])[0]
        if not len(envs):
            raise ValueError(f"no {where} env in this batch")
        return [int(envs[0])]
    if where == "last":
        return [B - 1]
    if where == "partial":
        return [(B // WAVES_PER_BLOCK) * WAVES_PER_BLOCK if B % WAVES_PER_BLOCK else B - 1]
    raise ValueError(where)


def wheres(name):
    """The `where`s that exist in a config."""
    cfg = make_cfg(name)
    out = []
    for w in WHERE:
        try:
            where_envs(cfg, w)
            out.append(w)
        except ValueError:
            pass
    return out


def coincident_plan(scn, n):
    """(agent a on agent b, agent c on obstacle k or None) for an env: agent 7
    on agent 3 and agent 5 on an obstacle (roll_states.coincident's pairs)
    where the env has eight agents, else its last agent on agent 0 and agent 1
    on the obstacle; the obstacle's collider column n + k is >= 32 where the
    env has such a column (M > 32), else obstacle 2."""
    a, b_, c = (7, 3, 5) if n >= 8 else (n - 1, 0, 1)
    if scn != rr.SCN_NAV:
        return a, b_, None, None
    k = 32 - n if 2 * n > 32 else 2
    return a, b_, c, k


def coincident(cfg, where, seed=0):
    """A jittered grid of pitch 0.45 over each env's live entities (neighbours
    0.39 to 0.51 apart: radius edges, no contacts). In the envs of `where` an
    agent sits exactly on another agent and, in a navigation env, one exactly
    on an obstacle (coincident_plan); the three agents have zero velocity and
    are held, so each pair shares every force and stays coincident."""
    n_b, scn_b, rs = shapes(cfg)
    B = int(cfg.n_envs)
    rng = np.random.default_rng(seed)
    pos = np.zeros((B, rs.Emax, 2), np.float32)
    for b in range(B):
        idx = rr.store_index(rs, scn_b[b], n_b[b])
        E = len(idx)
        side = int(np.ceil(np.sqrt(E)))
        gx, gy = np.meshgrid(np.arange(side), np.arange(side))
        grid = np.stack([gx.ravel(), gy.ravel()], -1).astype(np.float64) * 0.45 - 0.45 * (side - 1) / 2
        cell = rng.permutation(side * side)[:E]
        pos[b, idx] = (grid[cell] + rng.uniform(-0.03, 0.03, (E, 2))).astype(np.float32)
    vel = (0.3 * rng.normal(size=(B, rs.Nmax, 2))).astype(np.float32)
    _plant_padding(cfg, pos, 3)
    st = _state(pos, vel, B, rs.Nmax)
    for b in where_envs(cfg, where):
        a, b_, c, k = coincident_plan(int(scn_b[b]), int(n_b[b]))
        pos[b, a] = pos[b, b_]
        held = [a, b_]
        if c is not None:
            pos[b, c] = pos[b, rs.Nmax + rs.Tmax + k]
            held.append(c)
        st["vel"][b, held] = 0.0
        st["hold"][b, held] = True
    st["pos"] = pos
    return st


def staggered(state, EL, K):
    """step_count planted so that the envs re-lay out on different steps of a
    K-step launch with episode length EL: env 0 on the first step (EL - 1),
    env 2 on the last ((EL - K) mod EL: the count an env can reach that ends an
    episode on step K), the others spread over the steps between."""
    st = {k: v.copy() for k, v in state.items()}
    B = st["step_count"].shape[0]
    sc = (EL - 1 - np.arange(B)) % EL
    sc[0] = EL - 1
    if B > 2:
        sc[2] = (EL - K) % EL
    st["step_count"] = sc.astype(np.int32)
    return st


def actions(T, B, N, seed=0, hold=None):
    """Random index actions [T,B,N] int32, the held agents' the no-op (0)."""
    a = np.random.default_rng(1000 + seed).integers(0, 5, (T, B, N)).astype(np.int32)
    if hold is not None:
        a[:, hold] = 0
    return a


def ostate(cfg, st):
    """The oracle's state dict (oracle.ragged_ref.new_state's keys) of an
    injected state: episode 0, nothing accumulated."""
    n_b, scn_b, _ = shapes(cfg)
    B = st["pos"].shape[0]
    return dict(pos=st["pos"].copy(), vel=st["vel"].copy(), step=st["step_count"].copy(),
                episode=np.zeros(B, np.int32), ep_acc=np.zeros((B, 2)), ep_last=np.zeros((B, 2)),
                n=n_b.astype(np.int32), scn=scn_b.astype(np.int32), seed=int(cfg.seed))
