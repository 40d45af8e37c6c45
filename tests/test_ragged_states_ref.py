"""The injected states of tests/ragged_states.py are the cases they claim to
be: conditions on the inputs of test_gpu_ragged_states.py, checked with
oracle/ragged_ref.py alone (no kernel runs here). The mixed configs hold the
env shapes at the sweep's edges (M = 32, 34, 64). Crowds: edge lists on both
sides of the rollout's LDS cap (over the whole launch at M24 and M32), at
least half the agents in a collision and a quarter in several, contacts in
both column words, nothing coincident or non-finite. Lattice: every intended
neighbour pair at d2 == R2 bit for bit and listed, a one-ulp nudge moving
exactly the horizontal pairs out or in, pairs of every kind and across the
word boundary, no cost, a fixed point. Touching: d2 == dmin2 costs nothing, one
ulp inside costs one. Coincident: flagged exactly in the chosen envs, for the
whole launch. Staggered: an env done on the first step, one on the last."""
import numpy as np
import pytest

import ragged_states as gs
from oracle import ragged_ref as rr

NAMES = sorted(gs.CONFIGS)


def _live_costs(cfg, s):
    """Collision counts of every live agent on the fp32 state: one array."""
    n_b, scn_b, rs = gs.shapes(cfg)
    out = []
    for b in range(len(n_b)):
        _, _, pc = rr._compact(rs, s, b)
        out.append(rr.reward_cost_env(cfg, int(scn_b[b]), int(n_b[b]), pc, np.float32)[1])
    return out


def _edge_set(cfg, st):
    ob = rr.observe(cfg, gs.ostate(cfg, st))
    return set(zip(ob["edge_index"][0].tolist(), ob["edge_index"][1].tolist())), ob


def test_configs_have_the_claimed_shapes():
    for name in NAMES:
        cfg = gs.make_cfg(name)
        n, scn, rs = gs.shapes(cfg)
        assert n.tolist() == gs.SHAPES[name], name
        if name in gs.MIXED:
            assert scn.tolist() == [b % 3 for b in range(len(n))]
            base = {k: v for k, v in gs.CONFIGS[name].items() if k != "seed"}
            assert gs.find_seed(base, gs.SHAPES[name]) == gs.CONFIGS[name]["seed"]
    nav = lambda name: [int(x) for x, s in zip(gs.SHAPES[name], range(99)) if s % 3 == 0]   # noqa: E731
    assert nav("M24") == [22, 16, 22, 4, 5] and len(gs.SHAPES["M24"]) % gs.WAVES_PER_BLOCK == 2
    assert nav("M17") == [16, 16, 17]      # M = 32 exactly, and 34: two columns in word 1
    assert nav("M32") == [32, 32]          # M = 64
    assert [gs.lds_edge_cap(n) for n in (24, 17, 32, 12, 10, 7)] == [759, 759, 1215, 431, 431, 231]


@pytest.mark.parametrize("name", NAMES)
def test_crowd_is_crowded(name):
    cfg = gs.make_cfg(name, episode_length=1000)
    n_b, scn_b, rs = gs.shapes(cfg)
    B = len(n_b)
    cap = gs.lds_edge_cap(rs.Nmax)
    st = gs.crowd(cfg)
    s = gs.ostate(cfg, st)
    c = np.concatenate(_live_costs(cfg, s))
    cnt = np.diff(rr.observe(cfg, s)["edge_ptr"])
    print(f"crowd {name}: edges {cnt.tolist()} (LDS cap {cap}); in a collision {float((c > 0).mean()):.2f}, "
          f"in two or more {float((c > 1).mean()):.2f}, most {int(c.max())}")
    assert (c > 0).mean() >= 0.5 and (c > 1).mean() >= 0.25
    split = lambda k: (k > cap).any() and (k <= cap).any()   # noqa: E731
    if name in gs.MIXED:
        assert split(cnt)
    acts = gs.actions(gs.K, B, rs.Nmax, seed=1)
    for k in range(gs.K):
        s, ob = rr.step(cfg, s, acts[k], 1, np.float32)
        assert not ob["degenerate"].any(), k
        assert np.isfinite(s["pos"]).all() and np.isfinite(s["vel"]).all(), k
        if name in ("M24", "M32"):
            assert split(np.diff(ob["edge_ptr"])), k
    if name == "M24":
        # the crowd that overflows a rollout buffer's default slot, in the
        # slot set_state's observation fills and in the launch's first
        sl = gs.ostate(cfg, gs.crowd(cfg, L=gs.SLOT_L))
        default = B * min(8 * rs.Emax, rs.Mmax * (rs.Mmax - 1) + 2 * rs.Nmax)
        tot = [int(rr.observe(cfg, sl)["edge_ptr"][-1])]
        for k in range(gs.K):
            sl, ob = rr.step(cfg, sl, acts[k], 1, np.float32)
            tot.append(int(ob["edge_ptr"][-1]))
        assert tot[0] > default and tot[1] > default and min(tot) < default, (tot, default)


def test_m32_crowd_contacts_in_both_column_words():
    """Some agent of a 64-collider env collides with a column below 32 and one
    from 32 up (collisions are a subset of the contact candidates)."""
    cfg = gs.make_cfg("M32", episode_length=1000)
    n_b, scn_b, rs = gs.shapes(cfg)
    s = gs.ostate(cfg, gs.crowd(cfg))
    sa, so = np.float32(cfg.agent_size), np.float32(cfg.obstacle_size)
    found = 0
    for b in np.nonzero(scn_b == rr.SCN_NAV)[0]:
        n = int(n_b[b])
        p = s["pos"][b, gs.collider_rows(rs, 0, n)]
        d = p[:n, None, :] - p[None, :, :]
        d2 = d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]
        dmin = np.where(np.arange(2 * n) < n, np.float32(sa + sa), np.float32(sa + so))
        hit = (d2 > 0) & (d2 < (dmin * dmin)[None, :])
        found += int((hit[:, :32].any(1) & hit[:, 32:].any(1)).sum())
    assert found >= 8


@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("nudge", [0, 1, -1])
def test_lattice_ties(name, nudge):
    cfg = gs.make_cfg(name, episode_length=1000)
    n_b, scn_b, rs = gs.shapes(cfg)
    B = len(n_b)
    st = gs.lattice(cfg, nudge)
    assert st["hold"].all() and not st["vel"].any()
    R2 = np.float32(np.float32(cfg.sense_radius) * np.float32(cfg.sense_radius))
    assert R2 == np.float32(0.25)
    got, ob = _edge_set(cfg, st)
    base, _ = _edge_set(cfg, gs.lattice(cfg, 0))
    kinds_fixed, kinds_nudged, lost = set(), set(), set()
    for b in range(B):
        n, scn = int(n_b[b]), int(scn_b[b])
        rows = gs.collider_rows(rs, scn, n)
        M = len(rows)
        nudged, fixed = gs.lattice_pairs(M)
        kind = lambda c: "a" if c < n else "o"   # noqa: E731
        cross = {"lo_hi": False}
        for pairs, moved in ((nudged, True), (fixed, False)):
            for i, j in pairs:
                p, q = st["pos"][b, rows[i]], st["pos"][b, rows[j]]
                for a, c in ((p, q), (q, p)):      # the sweep forms row - column, either way round
                    dx, dy = a[0] - c[0], a[1] - c[1]
                    d2 = np.float32(dx * dx + dy * dy)
                    if moved and nudge > 0:
                        assert d2 > R2
                    elif moved and nudge < 0:
                        assert d2 < R2
                    else:
                        assert d2.view(np.int32) == R2.view(np.int32)
                e = (b * rs.Emax + int(rows[i]), b * rs.Emax + int(rows[j]))
                listed = not (moved and nudge > 0)
                assert (e in got) == listed and ((e[1], e[0]) in got) == listed
                assert e in base
                if not listed:
                    lost |= {e, (e[1], e[0])}
                (kinds_nudged if moved else kinds_fixed).add("".join(sorted(kind(i) + kind(j))))
                if i < 32 <= j:
                    cross["lo_hi"] = True
                    cross["nudged" if moved else "fixed"] = True
        if scn == rr.SCN_NAV and M > 32:
            # a pair across the two column words, row in word 0 and column in
            # word 1 and (the same pair from the other row) the other way
            # round: a nudged one and a fixed one
            assert cross.get("nudged") and cross.get("fixed"), (name, b)
    # nothing else changes: the nudged state has the tie state's edges but the pairs moved out
    assert got == base - lost
    want = {"aa", "ao", "oo"} if name in gs.MIXED else {"aa"}
    assert kinds_fixed >= want and kinds_nudged >= want, (kinds_fixed, kinds_nudged)
    for c in _live_costs(cfg, gs.ostate(cfg, st)):
        assert not c.any()
    # a fixed point: nobody moves over a launch, in fp32 and in fp64
    acts = gs.actions(gs.K, B, rs.Nmax, hold=st["hold"])
    assert not acts.any()
    for dtype in (np.float32, np.float64):
        s = gs.ostate(cfg, st)
        for k in range(gs.K):
            s, o = rr.step(cfg, s, acts[k], 1, dtype)
            assert not o["cost"].any()
        assert np.array_equal(s["pos"].astype(np.float32).view(np.int32), st["pos"].view(np.int32)), dtype


@pytest.mark.parametrize("name", NAMES)
def test_touching_pairs(name):
    cfg = gs.make_cfg(name, episode_length=1000)
    n_b, scn_b, rs = gs.shapes(cfg)
    st = gs.touching(cfg)
    assert st["hold"].all() and not st["vel"].any()
    sa, so = np.float32(cfg.agent_size), np.float32(cfg.obstacle_size)
    d_aa, d_ao = np.float32(sa + sa), np.float32(sa + so)
    d2 = lambda p, q: np.float32((p[0] - q[0]) * (p[0] - q[0]) + (p[1] - q[1]) * (p[1] - q[1]))   # noqa: E731
    costs = _live_costs(cfg, gs.ostate(cfg, st))
    ob = rr.observe(cfg, gs.ostate(cfg, st))
    for b, c in enumerate(costs):
        n, scn = int(n_b[b]), int(scn_b[b])
        p = st["pos"][b]
        nav = scn == rr.SCN_NAV
        assert d2(p[0], p[1]) == d2(p[1], p[0]) == np.float32(d_aa * d_aa)
        assert d2(p[2], p[3]) < np.float32(d_aa * d_aa) and d2(p[3], p[2]) < np.float32(d_aa * d_aa)
        if nav:
            o = rs.Nmax + rs.Tmax
            assert d2(p[0], p[o]) == np.float32(d_ao * d_ao)
            assert d2(p[2], p[o + 1]) < np.float32(d_ao * d_ao)
        # d == dmin: no collision (strict); one ulp inside: one each
        assert c[0] == 0 and c[1] == 0 and c[3] == 1 and c[2] == (2 if nav else 1), (b, c[:4])
        assert not c[4:].any()
        # the pairs are radius edges and the only ones (the rest target edges);
        # in a navigation env each obstacle is also within R of its agent's partner
        cnt = int(ob["edge_ptr"][b + 1] - ob["edge_ptr"][b])
        assert cnt == 2 * n * (2 if scn == rr.SCN_LINE else 1) + 2 * (6 if nav else 2)


@pytest.mark.parametrize("strict", [False, True])
@pytest.mark.parametrize("name", NAMES)
def test_coincident_pairs(name, strict):
    for where in gs.wheres(name):
        cfg = gs.make_cfg(name, episode_length=1000, strict_degenerate=strict)
        n_b, scn_b, rs = gs.shapes(cfg)
        B = len(n_b)
        envs = gs.where_envs(cfg, where)
        rest = np.setdiff1d(np.arange(B), envs)
        st = gs.coincident(cfg, where)
        deg = rr.observe(cfg, gs.ostate(cfg, st))["degenerate"]
        assert (deg[envs] == 1).all() and not deg[rest].any(), (name, where)
        for b in envs:
            a, b_, c, k = gs.coincident_plan(int(scn_b[b]), int(n_b[b]))
            assert (c is not None) == (scn_b[b] == rr.SCN_NAV)
            if c is not None and 2 * n_b[b] > 32:
                assert n_b[b] + k >= 32      # the obstacle's collider column lies in word 1
        acts = gs.actions(gs.K, B, rs.Nmax, seed=3, hold=st["hold"])
        s = gs.ostate(cfg, st)
        with np.errstate(invalid="ignore"):
            for k in range(gs.K):
                s, ob = rr.step(cfg, s, acts[k], 1, np.float32)
                if not strict:
                    assert np.isfinite(s["pos"]).all() and np.isfinite(s["vel"]).all()
                    assert (ob["degenerate"][envs] == 1).all() and not ob["degenerate"][rest].any(), (name, where, k)
        if strict:
            # MPE's 0/0: every agent of a planted env, no other env
            for b in range(B):
                live = s["pos"][b, :n_b[b]]
                assert np.isnan(live).all() if b in envs else np.isfinite(s["pos"][b]).all(), (name, where, b)
            asg = ob["assign"]
            for b in envs:
                if scn_b[b] != rr.SCN_NAV:
                    assert (asg[b, :n_b[b]] == -1).all()


@pytest.mark.parametrize("name", NAMES)
def test_staggered_relayouts(name):
    K, EL = gs.K_STAG, gs.EL_STAG
    cfg = gs.make_cfg(name, episode_length=EL)
    n_b, _, rs = gs.shapes(cfg)
    B = len(n_b)
    st = gs.staggered(gs.crowd(cfg), EL, K)
    acts = gs.actions(K, B, rs.Nmax, seed=1)
    s = gs.ostate(cfg, st)
    done = []
    for k in range(K):
        s, ob = rr.step(cfg, s, acts[k], 1, np.float32)
        done.append(ob["done"].astype(bool))
    done = np.stack(done)
    assert done[0, 0] and done[K - 1, 2]                    # the first step, the last
    assert done[1:K - 1].any()                              # and steps between
    assert not done.all(1).any()                            # never all at once
    assert len(np.unique(s["episode"])) >= 2
