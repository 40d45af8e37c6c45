"""The restated warm start of the assignment kernel (oracle/lsa_ref.py:
warm_start_assignment, wave_lsa's steps in its order) against scipy on states
paired with caches that do not belong to them (tests/lsa_warm_cases.py).
tests/test_gpu_lsa_warm.py holds the kernel to the restatement on the same
cases, certificate decisions and written-back duals included.

A restatement that always fell to the cold recurrence would equal scipy
everywhere, so the share of certified warm starts is asserted too (the 90% of
test_gpu_ragged.test_warm_start_equals_cold), per class, and so is that the
"several near" branch of the column scan runs without an exact tie.
"""
import collections

import numpy as np
import pytest
from scipy.optimize import linear_sum_assignment as scipy_lsa

import lsa_warm_cases as lc
from oracle.lsa_ref import DUAL_MAX, linear_sum_assignment, warm_start_assignment

REPS = 2         # every state x cache class, per scenario and N
BAR_REPS = 10    # the classes with a certified-share bar


def _check_case(C32, v0, col0, sk, ck, **kw):
    """One case against scipy; returns (certified, near-branch scans)."""
    N = C32.shape[0]
    C = C32.astype(np.float64)
    ref = scipy_lsa(C)[1]
    what = (N, sk, ck)
    trace = {}
    col, cert, v_out, col_out = warm_start_assignment(C, v0, col0, trace=trace, **kw)
    assert np.array_equal(col, ref), what
    assert np.isfinite(v_out).all(), what
    assert np.array_equal(np.sort(col_out), np.arange(N)) and np.array_equal(col_out, col), what
    col2, cert2, v2, _ = warm_start_assignment(C, v_out, col_out, **kw)
    assert np.array_equal(col2, ref) and np.isfinite(v2).all(), what
    if lc.exceeds_bound(v0):                 # non-finite or oversized duals: never used
        assert not cert, what
    if N > 1 and lc.has_equal_rows(C32):     # no unique optimum: scipy's tie rule decides, not the cache's
        assert not cert and not cert2, what
    return cert, trace.get("near", 0)


@pytest.mark.parametrize("scenario", ["polygon", "line"])
@pytest.mark.parametrize("N", lc.N_LIST)
def test_hostile_caches_give_scipy(scenario, N):
    cs = lc.cases(scenario, N, reps=REPS)
    for b, (sk, ck) in enumerate(zip(cs["state"], cs["cache"])):
        _check_case(cs["C"][b], cs["v0"][b], cs["col0"][b], sk, ck)
        if ck == "duplicate":                # whichever claimant the kernel keeps
            _check_case(cs["C"][b], cs["v0"][b], cs["col0"][b], sk, ck, claimant="first")
        if N > 1 and sk in lc.TIE_KINDS:     # the tie classes are ties
            assert lc.has_equal_rows(cs["C"][b]), (N, sk)
        if N > 1 and ck == "duplicate":
            assert lc.has_duplicate(cs["col0"][b], N), (N, sk)
        if ck.startswith(("mixed_", "common_", "huge", "neighbour_2p27")) or ck in lc.NONFINITE:
            assert lc.exceeds_bound(cs["v0"][b]), (N, ck)


@pytest.mark.parametrize("scenario", ["polygon", "line"])
@pytest.mark.parametrize("N", lc.N_LIST)
def test_certified_share_per_class(scenario, N):
    """Generic and near-slot states from a zero, an N(0, 1) and a neighbouring
    problem's cache: at least 90% certified, class by class."""
    cs = lc.cases(scenario, N, reps=BAR_REPS, state_kinds=lc.BAR_STATES, cache_kinds=lc.BAR_CACHES)
    hits, total = collections.Counter(), collections.Counter()
    for b, (sk, ck) in enumerate(zip(cs["state"], cs["cache"])):
        if sk == "example":
            continue
        cert, _ = _check_case(cs["C"][b], cs["v0"][b], cs["col0"][b], sk, ck)
        hits[sk, ck] += cert
        total[sk, ck] += 1
    print(f"{scenario} N={N} certified:", {f"{s}/{c}": f"{hits[s, c]}/{total[s, c]}" for s, c in sorted(total)})
    assert len(total) == len(lc.BAR_STATES) * len(lc.BAR_CACHES)
    for k in total:
        assert total[k] == BAR_REPS and hits[k] >= 0.9 * total[k], (N, k, hits[k])


def test_near_key_branch_runs_without_exact_tie():
    """Scans of the warm path in which several columns share the smallest
    float32 key of spc while the float64 minimum is unique (the kernel's
    "several near" branch with no exact tie). N(0, 1) duals with no cached
    matching reach it on every spread-out state class: all rows are free and
    minVal grows to the size of the costs, so reduced costs a rounding apart
    share a key. Duals staggered by 1e-10 on identical rows do not: the column
    reduction v_j = min_i (C - u) sets the columns of identical rows to one
    common row's values and the stagger is gone before the first scan."""
    near = {sk: 0 for sk in ("generic", "half_stacked", "grid")}
    for N in (16, 17, 24, 25, 32):
        cs = lc.cases("polygon", N, state_kinds=tuple(near), cache_kinds=("normal",))
        for b, sk in enumerate(cs["state"]):
            near[sk] += _check_case(cs["C"][b], cs["v0"][b], cs["col0"][b], sk, "normal")[1]
    assert all(n > 0 for n in near.values()), near


def test_example_2x2():
    """The wrong certificate that the magnitude bound closes: with duals of
    1e16 every reduced cost is a multiple of 2, and the quantised problem has a
    unique optimum that is not the problem's."""
    cs = lc.cases("polygon", 2)
    assert cs["state"][-1] == "example"
    C32, v0, col0 = cs["C"][-1], cs["v0"][-1], cs["col0"][-1]
    assert np.array_equal(C32, lc.EXAMPLE_C) and np.array_equal(v0, [1e16, 0.0])
    C = C32.astype(np.float64)
    assert np.array_equal(scipy_lsa(C)[1], [0, 1])
    col, cert, _, _ = warm_start_assignment(C, v0, col0, dual_max=np.inf)   # the kernel before the bound
    assert cert and np.array_equal(col, [1, 0])
    col, cert, v_out, _ = warm_start_assignment(C, v0, col0)
    assert not cert and np.array_equal(col, [0, 1]) and np.abs(v_out).max() <= 2.0


def test_bound_edges():
    """Duals at the bound are used, one ulp beyond are not; the cold path
    writes back duals of the size of the costs, so the cache heals."""
    rng = np.random.default_rng(3)
    C = rng.random((9, 9)).astype(np.float32).astype(np.float64)
    none = np.full(9, -1)
    ref = scipy_lsa(C)[1]
    at = np.zeros(9)
    at[4] = -DUAL_MAX
    col, cert, _, _ = warm_start_assignment(C, at, none)
    assert cert and np.array_equal(col, ref)
    at[4] = np.nextafter(-DUAL_MAX, -np.inf)
    col, cert, v_out, col_out = warm_start_assignment(C, at, none)
    assert not cert and np.array_equal(col, ref) and np.abs(v_out).max() <= 1.0
    col, cert, _, _ = warm_start_assignment(C, v_out, col_out)
    assert cert and np.array_equal(col, ref)
    # a common offset at the bound: feasible duals of that size, rejected by the certificate's own test
    col, cert, _, _ = warm_start_assignment(C, np.full(9, DUAL_MAX), none)
    assert not cert and np.array_equal(col, ref)


def test_cold_equals_the_sequential_restatement():
    """Uncertified cases run the cold recurrence: the same assignment as the
    sequential restatement (itself pinned to scipy in test_lsa_ref)."""
    cs = lc.cases("polygon", 17, state_kinds=lc.TIE_KINDS + ("half_stacked",), cache_kinds=("zero", "nan"))
    for b in range(len(cs["state"])):
        C = cs["C"][b].astype(np.float64)
        col, cert, _, _ = warm_start_assignment(C, cs["v0"][b], cs["col0"][b])
        assert np.array_equal(col, linear_sum_assignment(C))


def test_rejects_bad_input():
    with pytest.raises(ValueError):
        warm_start_assignment(np.array([[np.inf]]), [0.0], [-1])
    with pytest.raises(ValueError):
        warm_start_assignment(np.zeros((2, 3)), [0.0, 0.0], [-1, -1])
