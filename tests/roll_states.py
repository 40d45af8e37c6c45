"""Injected start states for the fused rollout tests (numpy only).

A reset layout plus a few random steps is sparse: a few percent of the agents
in a collision, about 100 edges in a 24-agent env that can hold 2304, no two
entities at one position and no pair exactly at the sensing radius. The
builders here give the states where a rollout kernel's sweep, contact walk,
edge lists and coincident fallback do the most work. Each returns a dict with
``pos`` [B,E,2] f32, ``vel`` [B,N,2] f32 and ``step_count`` [B] i32 (what
set_state takes), and ``hold`` [B,N] bool: agents whose action has to be the
no-op (index 0, oracle.batch_ref.action_force) in every action row; hold_still
applies it. Every builder is deterministic from its seed. tests/
test_roll_states_ref.py checks with the oracle alone that the states are what
they claim to be.

Entity order: agents [0,N), goals [N,2N), obstacles [2N,2N+No).
"""
import numpy as np

# half-widths of the crowd by agent count: nearly every agent in contact, most
# in several (6 and 96 chosen with the oracle: test_roll_states_ref)
CROWD_L = {24: 0.3, 12: 0.2, 6: 0.15, 3: 0.15, 96: 0.3}
# the smallest batch that keeps each rollout kernel's layout edges: (N, B)
# (pack_big: the unsplit packed kernel runs past the split one's 8192 envs;
# the smallest such batch whose last workgroup is half empty, 8 of 16 envs)
SHAPES = {"pair": (24, 9), "generic": (24, 5), "seg12": (12, 5), "seg6": (6, 5), "pack": (3, 37),
          "pack_big": (3, 8200), "tile": (96, 3)}
B_PARTIAL = 11                  # pair: a second workgroup of three envs, its first no lone half
K = 5                           # steps of a launch
K_STAG, EL_STAG = 10, 4         # the staggered cases: launch and episode length
SPREAD_L, SPREAD_VEL = 2.83, 2.0
PITCH = 0.5                     # lattice pitch = the sensing radius: R2 = 0.25 exactly
# lattice columns by kind (9 columns of 8 rows): A-A, A-O, O-O, O-A, A-G ... side by side
LATTICE_COLS = {"agent": (0, 1, 4), "obstacle": (2, 3, 8), "goal": (5, 6, 7)}
WHERE = ("lo", "hi", "both", "last", "partial")


def _state(pos, vel, B, N):
    return dict(pos=np.ascontiguousarray(pos, np.float32), vel=np.ascontiguousarray(vel, np.float32),
                step_count=np.zeros(B, np.int32), hold=np.zeros((B, N), bool))


def crowd(N, No, B, L=None, vel_scale=1.0, seed=0):
    """pos ~ uniform(-L, L), vel ~ vel_scale * normal (test_gpu_parity's
    _inject_random): every entity of an env inside a box of a few contact
    distances."""
    L = CROWD_L[N] if L is None else L
    rng = np.random.default_rng(seed)
    E = 2 * N + No
    pos = rng.uniform(-L, L, size=(B, E, 2)).astype(np.float32)
    vel = (vel_scale * rng.normal(size=(B, N, 2))).astype(np.float32)
    return _state(pos, vel, B, N)


def spread(N, No, B, seed=0):
    """The headline half-width with fast agents, and three entities of each
    env (an agent, a goal, an obstacle) at |x| >= 8, where parity_tol adds its
    ulp term."""
    st = crowd(N, No, B, SPREAD_L, SPREAD_VEL, seed)
    rng = np.random.default_rng(seed + 1)
    pos = st["pos"]
    for b in range(B):
        for e in (b % N, N + (b + 1) % N, 2 * N + (b + 2) % No):
            far = rng.uniform(8.0, 9.5) * (1.0 if (b + e) % 2 else -1.0)
            pos[b, e, (b + e) % 2] = np.float32(far)
    return st


def lattice_cells(N, No):
    """(col, row) of every entity on the 9 x 8 grid."""
    assert N <= 24 and No <= 24
    cells = np.zeros((2 * N + No, 2), np.int64)
    for kind, first, n in (("agent", 0, N), ("goal", N, N), ("obstacle", 2 * N, No)):
        cols = LATTICE_COLS[kind]
        for k in range(n):
            cells[first + k] = (cols[k % 3], k // 3)
    return cells


def lattice(N, No, B, nudge=0, seed=0):
    """Entities on a grid of pitch 0.5 = R at coordinates that are multiples of
    0.5 (env b shifted by a multiple of the pitch): neighbours at d2 == R2 bit
    for bit, diagonals outside, nobody in contact; zero velocity and the no-op
    for everyone, so every step of a launch sees the same ties. nudge = +1 / -1
    moves the odd columns by one ulp in x away from / toward the column on
    their left (so toward / away from the one on their right): just outside,
    just inside."""
    assert nudge in (0, 1, -1)
    cells = lattice_cells(N, No)
    pos = np.zeros((B, 2 * N + No, 2), np.float32)
    for b in range(B):
        x = (PITCH * (cells[:, 0] + 1 + (b + seed) % 3)).astype(np.float32)
        y = (PITCH * (cells[:, 1] + 1 + (2 * b + seed) % 3)).astype(np.float32)
        if nudge:
            odd = cells[:, 0] % 2 == 1
            x[odd] = np.nextafter(x[odd], np.float32(np.inf if nudge > 0 else -np.inf))
        pos[b, :, 0], pos[b, :, 1] = x, y
    st = _state(pos, np.zeros((B, N, 2), np.float32), B, N)
    st["hold"][:] = True
    return st


def where_envs(where, B, envs_per_block=8):
    """The envs of a `where`: wave 1's low half, its high half, both, the last
    env (a lone half where B is odd), the first env of the last workgroup
    where that one is partial (else the last env)."""
    w = 1 if B >= 4 else 0
    if where == "lo":
        return [2 * w]
    if where == "hi":
        return [2 * w + 1]
    if where == "both":
        return [2 * w, 2 * w + 1]
    if where == "last":
        return [B - 1]
    if where == "partial":
        return [(B // envs_per_block) * envs_per_block if B % envs_per_block else B - 1]
    raise ValueError(where)


def coincident(N, No, B, where, seed=0, envs_per_block=8):
    """A jittered grid of pitch 0.45 (neighbours 0.39 to 0.51 apart: radius
    edges, no contacts). In the envs of `where`, agent 7 sits exactly on agent
    3 and agent 5 exactly on obstacle 2 (test_coincident_pairs_one_env_per_
    wave's pairs); the three agents have zero velocity and are held, so each
    pair shares every force and stays coincident."""
    rng = np.random.default_rng(seed)
    E = 2 * N + No
    side = int(np.ceil(np.sqrt(E)))
    gx, gy = np.meshgrid(np.arange(side), np.arange(side))
    grid = np.stack([gx.ravel(), gy.ravel()], -1).astype(np.float64) * 0.45 - 0.45 * (side - 1) / 2
    pos = np.zeros((B, E, 2), np.float32)
    for b in range(B):
        cell = rng.permutation(side * side)[:E]
        pos[b] = (grid[cell] + rng.uniform(-0.03, 0.03, (E, 2))).astype(np.float32)
    vel = (0.3 * rng.normal(size=(B, N, 2))).astype(np.float32)
    st = _state(pos, vel, B, N)
    for b in where_envs(where, B, envs_per_block):
        pos[b, 7] = pos[b, 3]
        pos[b, 5] = pos[b, 2 * N + 2]
        st["vel"][b, [3, 7, 5]] = 0.0
        st["hold"][b, [3, 7, 5]] = True
    return st


def staggered(state, EL, K):
    """step_count planted so that the two envs of a wave (2w, 2w + 1) re-lay
    out on different steps of a K-step launch with episode length EL: env 0
    on the first step (EL - 1), env 2 on the last ((EL - K) mod EL: the count
    an env can reach that ends an episode on step K)."""
    st = {k: v.copy() for k, v in state.items()}
    B = st["step_count"].shape[0]
    w = np.arange(B) // 2
    sc = np.where(np.arange(B) % 2 == 0, (EL - 1 - w) % EL, (EL - 3 - w) % EL)
    sc[0] = EL - 1
    if B > 2:
        sc[2] = (EL - K) % EL
    st["step_count"] = sc.astype(np.int32)
    return st


def hold_still(actions, hold):
    """Index actions [T,B,N] (numpy) with the held agents' set to the no-op."""
    a = np.array(actions, copy=True)
    a[:, hold] = 0
    return a


def actions(T, B, N, seed=0, hold=None):
    """Random index actions [T,B,N] int32, the held agents' the no-op."""
    a = np.random.default_rng(1000 + seed).integers(0, 5, (T, B, N)).astype(np.int32)
    return a if hold is None else hold_still(a, hold)


def max_edges(N, No):
    """An env's edge capacity: every radius list full, and the goal edges."""
    M = N + No
    return M * (M - 1) + 2 * N
