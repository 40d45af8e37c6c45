"""Linear sum assignment restated from scipy's shortest-augmenting-path solver.

TEST INFRASTRUCTURE ONLY (the checker); see oracle/batch_ref.py's header.

The reference's polygon/line scenarios (``simple_formation.py``,
``simple_line.py``: GSMARL.egg-info/SOURCES.txt:24-25; readme.md:89-90) call
``scipy.optimize.linear_sum_assignment`` every step (scipy pinned at 1.7.3,
requirements.txt:101). That solver is scipy's ``rectangular_lsap.cpp``
(Crouse, "On implementing 2D rectangular assignment algorithms", 2016), the
same algorithm in every release 1.4 .. 1.15 (this container ships 1.15.3).
This module restates its published algorithm step for step, including the
two details that decide ties:

* the column scan order of every augmenting-path search is the list
  ``remaining = [n-1, ..., 1, 0]``, from which the chosen column is removed by
  swapping in the list's last element;
* among columns of equal reduced cost the scan keeps the first minimum unless
  a later equal one is unassigned (``row4col == -1``), so the result is the
  LAST unassigned minimum in scan order if there is one, else the FIRST.

All arithmetic is float64 in scipy's operation order
(``r = minVal + C[i][j] - u[i] - v[j]`` evaluated left to right), so with the
same float64 cost matrix the assignment is identical, ties included.
``tests/test_lsa_ref.py`` pins this restatement against scipy itself on
random, integer (tie-heavy) and constant matrices; the HIP kernel
(gsm_ragged_kernels.hip) runs the same recurrence one column per lane.

``warm_start_assignment`` restates the rest of that kernel: the start from a
cached (duals, matching) state, the uniqueness certificate that decides
whether its result is used, and the cold recurrence otherwise, in the
lane-parallel formulation (exact minimum, then the position in ``remaining``).
tests/test_lsa_warm_ref.py holds it to scipy from caches that do not belong to
the state; tests/test_gpu_lsa_warm.py holds the kernel to it.
"""
from __future__ import annotations

import math

import numpy as np


def _augmenting_path(n, cost, u, v, path, row4col, spc, i, SR, SC, remaining):
    """One shortest augmenting path from free row i. Returns (sink, minVal)."""
    min_val = 0.0
    num_remaining = n
    for it in range(n):
        remaining[it] = n - it - 1
    for k in range(n):
        SR[k] = False
        SC[k] = False
        spc[k] = math.inf
    sink = -1
    while sink == -1:
        index = -1
        lowest = math.inf
        SR[i] = True
        for it in range(num_remaining):
            j = remaining[it]
            r = min_val + cost[i][j] - u[i] - v[j]
            if r < spc[j]:
                path[j] = i
                spc[j] = r
            if spc[j] < lowest or (spc[j] == lowest and row4col[j] == -1):
                lowest = spc[j]
                index = it
        min_val = lowest
        if min_val == math.inf:
            raise ValueError("cost matrix is infeasible")
        j = remaining[index]
        if row4col[j] == -1:
            sink = j
        else:
            i = row4col[j]
        SC[j] = True
        num_remaining -= 1
        remaining[index] = remaining[num_remaining]
    return sink, min_val


def linear_sum_assignment(cost):
    """Square float64 cost matrix -> col4row (int64 [n]): row i gets column
    col4row[i], minimising the total cost (scipy's tie-breaking)."""
    c = np.asarray(cost, dtype=np.float64)
    n = c.shape[0]
    if c.ndim != 2 or c.shape[1] != n:
        raise ValueError("square matrices only (the scenarios assign N agents to N slots)")
    if n == 0:
        return np.zeros(0, np.int64)
    if np.isnan(c).any() or (c == -np.inf).any():
        raise ValueError("cost matrix contains NaN or -inf")
    cost_l = c.tolist()          # Python floats are IEEE float64
    u = [0.0] * n
    v = [0.0] * n
    spc = [math.inf] * n
    path = [-1] * n
    col4row = [-1] * n
    row4col = [-1] * n
    SR = [False] * n
    SC = [False] * n
    remaining = [0] * n
    for cur in range(n):
        sink, min_val = _augmenting_path(n, cost_l, u, v, path, row4col, spc, cur, SR, SC, remaining)
        u[cur] += min_val
        for i in range(n):
            if SR[i] and i != cur:
                u[i] += min_val - spc[col4row[i]]
        for j in range(n):
            if SC[j]:
                v[j] -= min_val - spc[j]
        j = sink
        while True:
            i = path[j]
            row4col[j] = i
            col4row[i], j = j, col4row[i]
            if i == cur:
                break
    return np.asarray(col4row, dtype=np.int64)


# ---------------------------------------------------------------------------
# The kernel's warm start (gsm_ragged_kernels.hip: wave_lsa), restated
# ---------------------------------------------------------------------------
# Largest |column dual| the warm start works with (kLsaDualMax in the kernel,
# derived in the comment above wave_lsa): a cache with a larger dual is not
# used, and a matching whose final duals exceed it is not certified.
DUAL_MAX = 4096.0
_TAU = 1e-9          # tight threshold of the uniqueness certificate
_SLACK = 1e-11       # feasibility / complementary-slackness threshold


def _augment_lanes(c, u, v, col4row, row4col, cur, trace=None):
    """scipy's augmenting step for free row `cur` from the duals and partial
    matching given (updated in place), in the kernel's lane-parallel form:
    per scan the exact minimum over the remaining columns, then the last
    unassigned minimum in `remaining` order if any, else the first
    (tests/test_lsa_ref.py pins this formulation against scipy from the empty
    matching). Returns False, leaving the state untouched, if no free column
    is reached within n scans (the kernel's guard).

    trace["near"] counts the scans in which several remaining columns share
    the smallest float32 key of spc while the float64 minimum is unique (the
    kernel's "several near" branch taken without an exact tie)."""
    n = c.shape[0]
    idx = np.arange(n)
    spc = np.full(n, np.inf)
    path = np.full(n, -1)
    SR = np.zeros(n, bool)
    SC = np.zeros(n, bool)
    rpos = n - 1 - idx
    nrem = n
    min_val = 0.0
    i, sink, guard = cur, -1, 0
    while sink < 0:
        SR[i] = True
        rem = ~SC
        r = ((min_val + c[i]) - u[i]) - v
        upd = rem & (r < spc)
        path[upd] = i
        spc[upd] = r[upd]
        m = spc[rem].min()
        cand = rem & (spc == m)
        if trace is not None:
            with np.errstate(over="ignore"):
                k32 = spc.astype(np.float32)
            if (rem & (k32 == k32[rem].min())).sum() > 1 and cand.sum() == 1:
                trace["near"] = trace.get("near", 0) + 1
        fre = cand & (row4col == -1)
        if fre.any():
            j = int(np.flatnonzero(fre)[np.argmax(rpos[fre])])
        else:
            j = int(np.flatnonzero(cand)[np.argmin(rpos[cand])])
        min_val = m
        at = rpos[j]
        SC[j] = True
        nrem -= 1
        rpos[rem & (idx != j) & (rpos == nrem)] = at
        if row4col[j] < 0:
            sink = j
        else:
            i = int(row4col[j])
            guard += 1
            if guard >= n:
                return False
    spc_c = spc[np.maximum(col4row, 0)]
    for k in range(n):
        if k == cur:
            u[k] += min_val
        elif SR[k]:
            u[k] += min_val - spc_c[k]
    v[SC] -= min_val - spc[SC]
    j = sink
    for _ in range(n + 1):
        i = int(path[j])
        row4col[j] = i
        col4row[i], j = j, col4row[i]
        if i == cur:
            break
    return True


def _certified(c, u, v, col4row, row4col, dual_max):
    """The kernel's uniqueness certificate of a complete matching: duals within
    dual_max, r = (C - u_i) - v_j >= -1e-11 everywhere and |r| <= 1e-11 on the
    matching, and the tight unmatched pairs (r - succ(1e-9) < 0) close no
    alternating cycle (rows peeled sink by sink)."""
    n = c.shape[0]
    idx = np.arange(n)
    r = (c - u[:, None]) - v[None, :]
    rc = r[idx, col4row]
    if not (np.all(np.abs(v) <= dual_max) and np.all(r.min(1) >= -_SLACK) and np.all(np.abs(rc) <= _SLACK)):
        return False
    tight = np.signbit(r - np.nextafter(_TAU, 1.0))
    tight[idx, col4row] = False
    rows = np.ones(n, bool)
    cols = np.ones(n, bool)
    for _ in range(n):
        if not rows.any():
            break
        sinks = rows & ~(tight & cols[None, :]).any(1)
        if not sinks.any():
            break                         # every remaining row is on a cycle
        rows &= ~sinks
        cols &= ~((row4col >= 0) & sinks[np.maximum(row4col, 0)])
    return not rows.any()


def warm_start_assignment(cost, v0, col0, claimant="last", dual_max=DUAL_MAX, trace=None):
    """wave_lsa's assignment of a square float64 cost matrix (the fp32 matrix
    promoted) from a cached state: column duals v0 [n] float64 and matching
    col0 [n] (row -> column; any integers). Returns (col4row, certified,
    v_out, col_out): the assignment, whether the warm start was certified the
    unique optimum (else the cold recurrence ran), and the cache written back.

    Every step in the kernel's order: the gate on the cached duals (finite
    and within dual_max), u_i = min_j (C - v), one column reduction
    v_j = min_i (C - u), the row minima again, rows keeping their cached
    column when it attains the row minimum (rc == m, the same expression),
    the free rows augmented in ascending order, the certificate.

    claimant: which row keeps a column that several rows of col0 claim
    ("last" / "first" in row order); the kernel keeps one, unspecified.
    dual_max=inf restates the kernel without the magnitude bound."""
    c = np.ascontiguousarray(cost, dtype=np.float64)
    n = c.shape[0]
    if c.ndim != 2 or c.shape[1] != n or n == 0:
        raise ValueError("square, non-empty matrices only")
    if not np.isfinite(c).all():
        raise ValueError("non-finite cost: the kernel assigns nothing (-1) before any of this")
    v0 = np.asarray(v0, np.float64)
    c0 = np.asarray(col0, np.int64)
    idx = np.arange(n)
    solved = False
    with np.errstate(over="ignore", invalid="ignore"):
        if np.all(np.abs(v0) <= dual_max) and np.isfinite(v0).all():
            m = (c - v0[None, :]).min(1)
            v = (c - m[:, None]).min(0)
            cv = c - v[None, :]
            m = cv.min(1)
            inr = (c0 >= 0) & (c0 < n)
            rc = np.where(inr, cv[idx, np.where(inr, c0, 0)], np.inf)
            u = m.copy()
            want = inr & (rc == m)
            keep = np.full(n, -1)
            for i in (idx if claimant == "last" else idx[::-1]):
                if want[i]:
                    keep[c0[i]] = i
            kept = want & (keep[np.where(inr, c0, 0)] == idx)
            col4row = np.where(kept, c0, -1)
            row4col = keep.copy()
            ok = True
            for i in np.flatnonzero(~kept):
                ok = _augment_lanes(c, u, v, col4row, row4col, int(i), trace)
                if not ok:
                    break
            solved = bool(ok and _certified(c, u, v, col4row, row4col, dual_max))
    if not solved:
        u = np.zeros(n)
        v = np.zeros(n)
        col4row = np.full(n, -1)
        row4col = np.full(n, -1)
        for cur in range(n):
            if not _augment_lanes(c, u, v, col4row, row4col, cur):
                break
    return col4row.astype(np.int64), solved, v, col4row.astype(np.int64)
