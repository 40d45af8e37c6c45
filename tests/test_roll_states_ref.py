"""The injected states of tests/roll_states.py are the hard cases they claim to
be: conditions on the inputs of test_gpu_roll_states.py, checked with the CPU
oracle alone (no kernel runs here). Crowds: nearly every agent in contact,
most in several, edge lists near their capacity at the first emitted step, no
coincident pair and finite positions over the launch. Lattice: a fixed point
with every kind of pair exactly at d2 == R2, a one-ulp nudge moving exactly
the nudged pairs across the predicate. Coincident: the planted pairs stay
coincident for the whole launch (two launches for the back-to-back case), and
strict mode turns them into NaNs that spread. Staggered: the envs of a wave
re-lay out on different steps, one on the first and one on the last."""
import numpy as np
import pytest

import roll_states as rs
from oracle import batch_ref as br


def _ocfg(N, B, **kw):
    return br.make_cfg(n_agents=N, n_envs=B, **kw)


def _ostate(st, dtype=np.float32):
    B = st["pos"].shape[0]
    return dict(pos=st["pos"].astype(dtype), vel=st["vel"].astype(dtype), step=st["step_count"].copy(),
                episode=np.zeros(B, np.int32), ep_acc=np.zeros((B, 2)), ep_last=np.zeros((B, 2)))


def _contacts(ocfg, pos):
    """Contacts of every agent, d < dmin in fp32: [B,N]."""
    sp = br.Spec(ocfg, np.float32)
    pa, pc = pos[:, :sp.N], pos[:, sp.cidx]
    d = np.sqrt(br._pair_d2(pa[:, :, None, :], pc[:, None, :, :]))
    return ((d < sp.dmin[None, None, :]) & ~np.eye(sp.N, sp.M, dtype=bool)[None]).sum(-1)


def _edge_set(ocfg, pos):
    _, ei, _ = br.edges(ocfg, pos, np.float32)
    return set(zip(ei[0].tolist(), ei[1].tolist()))


@pytest.mark.parametrize("shape", sorted(rs.SHAPES))
def test_crowd_is_crowded(shape):
    N, B = rs.SHAPES[shape]
    ocfg = _ocfg(N, B, episode_length=1000)
    st = rs.crowd(N, N, B, seed=N + B)
    c = _contacts(ocfg, st["pos"])
    in_contact, multi = float((c > 0).mean()), float((c > 1).mean())
    s = _ostate(st)
    acts = rs.actions(rs.K, B, N, seed=N + B)
    fill = []
    for k in range(rs.K):
        s, ob = br.step(ocfg, s, acts[k], 1, np.float32, seed=0)
        fill.append(ob["edge_ptr"][-1] / B / rs.max_edges(N, N))
        assert not ob["degenerate"].any(), k          # no coincident pair, nothing non-finite
        assert np.isfinite(s["pos"]).all() and np.isfinite(s["vel"]).all(), k
    start = br.edges(ocfg, st["pos"], np.float32)[0][-1] / B / rs.max_edges(N, N)
    print(f"crowd {shape} N={N} B={B} L={rs.CROWD_L[N]}: in contact {in_contact:.2f}, two or more {multi:.2f}, "
          f"most {int(c.max())}; edge fill start {start:.2f}, steps {np.round(fill, 2).tolist()}")
    assert in_contact >= 0.8 and multi >= 0.5
    if N == 24:
        assert c.max() >= 8
    if N <= 24:
        assert fill[0] >= 0.75
    else:
        # 96 agents: a quarter of the capacity are obstacle-obstacle and goal
        # edges, which stay; every agent starts with 20 and more contacts and
        # is thrown out of the box by its first step, at every half-width (at
        # most 0.65 of the capacity after a step, for L from 0.2 to 0.6). The
        # lists are near full in the injected state, which the launch's first
        # step reads, and still hold most of the capacity when first emitted.
        assert start >= 0.75 and fill[0] >= 0.5


def test_spread_reaches_the_ulp_term():
    for shape in ("pair", "pack", "pack_big", "tile"):
        N, B = rs.SHAPES[shape]
        st = rs.spread(N, N, B, seed=N)
        far = np.abs(st["pos"]) >= 8.0
        assert far[:, :N].any(1).any(1).all() and far[:, N:2 * N].any() and far[:, 2 * N:].any()
        assert np.isfinite(st["pos"]).all()


def _lattice_ties(N, No):
    """Grid neighbours (a, b, horizontal, column of the left one) by entity."""
    cells = rs.lattice_cells(N, No)
    at = {tuple(c): e for e, c in enumerate(cells.tolist())}
    out = []
    for (cx, cy), e in at.items():
        for dx, dy in ((1, 0), (0, 1)):
            o = at.get((cx + dx, cy + dy))
            if o is not None:
                out.append((e, o, dx == 1, cx))
    return out


@pytest.mark.parametrize("nudge", [0, 1, -1])
def test_lattice_ties_and_fixed_point(nudge):
    N, B = rs.SHAPES["pair"]
    E = 3 * N
    ocfg = _ocfg(N, B, episode_length=1000)
    st = rs.lattice(N, N, B, nudge)
    assert st["hold"].all() and not st["vel"].any()
    acts = rs.actions(rs.K, B, N, hold=st["hold"])
    assert not acts.any()
    for dtype in (np.float32, np.float64):
        s = _ostate(st, dtype)
        for k in range(rs.K):
            s, _ = br.step(ocfg, s, acts[k], 1, dtype, seed=0)
        assert np.array_equal(s["pos"].astype(np.float32).view(np.int32), st["pos"].view(np.int32)), dtype
    kind = lambda e: "a" if e < N else "g" if e < 2 * N else "o"   # noqa: E731
    ties = _lattice_ties(N, N)
    R2 = br.Spec(ocfg, np.float32).R2
    assert R2 == np.float32(0.25)
    kinds_at_tie = set()
    base = _edge_set(ocfg, rs.lattice(N, N, B, 0)["pos"])
    got = _edge_set(ocfg, st["pos"])
    for b in range(B):
        p = st["pos"][b]
        for a, o, horiz, col in ties:
            d2 = br._pair_d2(p[a], p[o])
            radius_pair = kind(a) != "g" and kind(o) != "g"
            edge = (b * E + a, b * E + o)
            # odd columns moved right (+1) or left (-1): the pair (even, odd)
            # grows with +1, the pair (odd, even) with -1
            grows = horiz and nudge != 0 and ((col % 2 == 0) == (nudge > 0))
            shrinks = horiz and nudge != 0 and not grows
            if grows:
                assert d2 > R2
            elif shrinks:
                assert d2 < R2
            else:
                assert d2 == R2
                kinds_at_tie.add("".join(sorted(kind(a) + kind(o))))
            if radius_pair:
                assert (edge in got) == (not grows) and edge in base
                assert ((edge[1], edge[0]) in got) == (not grows)
    if nudge == 0:
        assert {"aa", "ao", "oo", "ag"} <= kinds_at_tie
    # nothing else changes: the nudged state has the tie state's edges but the grown pairs'
    lost = {(b * E + a, b * E + o) for b in range(B) for a, o, hz, col in ties
            if hz and nudge != 0 and ((col % 2 == 0) == (nudge > 0)) and kind(a) != "g" and kind(o) != "g"}
    lost |= {(t, s_) for s_, t in lost}
    assert got == base - lost
    if nudge:
        lost_kinds = {"".join(sorted(kind(s_ % E) + kind(t % E))) for s_, t in lost}
        assert lost_kinds >= ({"aa", "oo"} if nudge > 0 else {"ao"})   # and the other nudge's stay just inside


@pytest.mark.parametrize("shape,strict", [("pair", False), ("pair", True), ("tile", False)])
@pytest.mark.parametrize("where", rs.WHERE)
def test_coincident_pairs_persist(shape, where, strict):
    N, B = rs.SHAPES[shape]
    if shape == "pair" and where == "partial":
        B = rs.B_PARTIAL
    K = 2 * rs.K   # the back-to-back case replays the launch twice
    ocfg = _ocfg(N, B, episode_length=1000, strict_degenerate=strict)
    st = rs.coincident(N, N, B, where, seed=N, envs_per_block=8 if N == 24 else 1)
    envs = rs.where_envs(where, B, 8 if N == 24 else 1)
    acts = rs.actions(rs.K, B, N, seed=N, hold=st["hold"])
    s = _ostate(st)
    rest = np.setdiff1d(np.arange(B), envs)
    for k in range(K):
        s, ob = br.step(ocfg, s, acts[k % rs.K], 1, np.float32, seed=0)
        if not strict:
            p = s["pos"]
            assert np.isfinite(p).all() and np.isfinite(s["vel"]).all()
            for b in envs:
                assert np.array_equal(p[b, 7], p[b, 3]) and np.array_equal(p[b, 5], p[b, 2 * N + 2]), (k, b)
                assert np.array_equal(p[b, [3, 5]], st["pos"][b, [3, 5]])   # and nothing pushed them
            assert (ob["degenerate"][envs] == 1).all() and not ob["degenerate"][rest].any()
    if strict:
        # MPE's 0/0 (test_oracle_kat.test_coincident_strict_is_mpe_nan_and_spreads):
        # every agent of a planted env, no other env
        assert np.isnan(s["pos"][envs, :N]).all() and np.isfinite(s["pos"][rest]).all()


@pytest.mark.parametrize("shape", ["pair", "pack", "pack_big", "seg12"])
def test_staggered_relayouts(shape):
    N, B = rs.SHAPES[shape]
    K, EL = rs.K_STAG, rs.EL_STAG
    ocfg = _ocfg(N, B, episode_length=EL)
    st = rs.staggered(rs.crowd(N, N, B, seed=N + B), EL, K)
    acts = rs.actions(K, B, N, seed=N + B)
    s = _ostate(st)
    first = last = None
    for k in range(K):
        s, ob = br.step(ocfg, s, acts[k], 1, np.float32, seed=0)
        first = ob["done"].copy() if k == 0 else first
        last = ob["done"]
    assert first[0] and first.sum() < B and last[2] and last.sum() < B
    ep = s["episode"]
    pairs = ep[:B - B % 2].reshape(-1, 2)
    assert (pairs[:, 0] != pairs[:, 1]).any() and len(np.unique(ep)) >= 2
    sc = st["step_count"]
    assert (sc[0:B - B % 2:2] != sc[1:B:2]).all()   # no wave's two envs re-lay out together
