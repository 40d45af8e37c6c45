"""The guard-band checker caught lying (tests/guard.py), on the CPU.

Each fault is planted by a fake "kernel" in Python on tensors from the
helper; the check meant for it has to fail and name it, every other check has
to pass, and the same fake without the fault passes all of them."""
import re
from pathlib import Path

import pytest
import torch

import guard as G
from gsmarl_amd import _lib, gnn, loss, policy

_EMPTY, _EMPTY_LIKE = torch.empty, torch.empty_like
N, F = 37, 5                                         # rows of 20 bytes: nothing is a multiple of anything


def _x():
    return torch.randn(N, F, generator=torch.Generator().manual_seed(0))


def _flat(t, extra_before=0, extra_after=0):
    """``t`` with neighbours: the elements around a contiguous tensor, as a kernel's pointer reaches them."""
    return t.as_strided((t.numel() + extra_before + extra_after,), (1,), t.storage_offset() - extra_before)


def fake(x, fault=None):
    """out = 2 x through a workspace: what a kernel and its wrapper do. (The
    workspace sum is scaled to 1e15 so that adding it to either prefill
    pattern, -4.3e8 or 4.0e18 as floats, changes the bits.)"""
    out, work = torch.empty_like(x), torch.empty(F)
    if fault == "adds":
        work += 1e15 * x.sum(0)                             # relies on what the workspace held
    else:
        work.copy_(1e15 * x.sum(0))
    rows = N - 1 if fault == "last row" else N
    out[:rows] = 2 * x[:rows]
    if fault == "past the end":
        _flat(out, 0, 1)[-1] = 1.0
    if fault == "before the start":
        _flat(out, 1, 0)[0] = 1.0
    total = torch.empty(F)
    total.copy_(work)
    if fault == "reads the band":
        total += _flat(x, 0, 1)[-1]                  # one element past the input
    return dict(out=out, total=total)


def _inputs(x):
    return dict(x=G.In(x, G.floats))


def _plain(x):
    """The plain call on a tensor with room around it, as an allocator's slack gives a kernel."""
    room = torch.zeros(x.numel() + 16)
    v = room[8:8 + x.numel()].view(x.shape)
    v.copy_(x)
    return {k: t.clone() for k, t in fake(v).items()}


def _run(fault):
    x = _x()
    return G.run_case(lambda x: fake(x, fault), _inputs(x), plain=_plain(x), device_types=("cpu",))


def test_the_honest_fake_passes_every_check():
    out = _run(None)
    assert torch.equal(out["out"], 2 * _x())


def test_a_named_workspace_has_to_come_from_a_guarded_allocation():
    x = _x()
    G.run_case(fake, _inputs(x), plain=_plain(x), device_types=("cpu",), work=[(F,)])
    with pytest.raises(AssertionError, match=r"no allocation under guard has the workspace shape \[\(6,\)\]"):
        G.run_case(fake, _inputs(x), plain=_plain(x), device_types=("cpu",), work=[(F + 1,)])


@pytest.mark.parametrize("fault,says", [
    ("past the end", r"guard bands changed:\s+alloc1\(37, 5\): 4 bytes changed after the end; first at byte \+740, "
                     r"last at byte \+743"),
    ("before the start", r"guard bands changed:\s+alloc1\(37, 5\): 4 bytes changed before the start; first at byte "
                         r"-4, last at byte -1"),
    ("last row", r"fill A, prefill 0: 5 elements of out never written, first at \[36, 0\]"),
    ("adds", r"\(e\) total depends on what an output or a workspace held before the call: fill A, prefill 0 and "
             r"fill A, prefill 1 differ"),
    ("reads the band", r"\(d\) total depends on memory outside an input: fill A, prefill 0 and fill B, prefill 0 "
                       r"differ"),
])
def test_planted_fault_is_reported(fault, says):
    with pytest.raises(AssertionError) as e:
        _run(fault)
    assert re.search(says, str(e.value)), str(e.value)


def _guarded_run(fault, fill, prefill):
    g = G.Guard(prefill)
    x = g.input(_x(), G.floats(fill), "x")
    with G.guarded_allocations(g, ("cpu",)):
        out = fake(x, fault)
    return g, out


@pytest.mark.parametrize("fault", ["past the end", "before the start", "last row", "adds", "reads the band"])
def test_each_fault_fails_its_own_check_and_no_other(fault):
    """(a) bands, (b) unwritten, (d) fill A against fill B, (e) prefill 0 against prefill 1, one at a time."""
    runs = {(f, p): _guarded_run(fault, f, p) for f, p in (("A", 0), ("B", 0), ("A", 1))}
    g, out = runs["A", 0]
    failed = set()
    if g.problems():
        failed.add("a")
    if any(bool(g.unwritten(t).any()) for t in out.values()):
        failed.add("b")
    if not all(G.same_bits(out[k], runs["B", 0][1][k]) for k in out):
        failed.add("d")
    if not all(G.same_bits(out[k], runs["A", 1][1][k]) for k in out):
        failed.add("e")
    want = {"past the end": {"a"}, "before the start": {"a"}, "last row": {"b", "e"}, "adds": {"e"},
            "reads the band": {"d"}}[fault]
    # an element never written also differs between the prefills: (e) sees what (b) names
    assert failed == want, (fault, failed)


def test_an_input_that_is_written_is_reported():
    g = G.Guard()
    x = g.input(_x(), G.floats("A"), "x")
    x[3, 2] = 0.0
    (line,) = g.problems()
    assert "x: 4 bytes changed inside the input" in line and "first at byte +68" in line


def test_band_fills_of_integer_arrays_are_legal_values():
    ptr = torch.tensor([3, 5, 5, 9], dtype=torch.int64)
    for fill in "AB":
        assert set(G.ids(fill, 10)) <= set(range(10)) and set(G.actions(fill, 5)) <= set(range(5))
        assert set(G.counts(fill, 24)) <= set(range(25)) and set(G.flags(fill)) <= {0, 1}
        assert G.offsets(fill, ptr) == (3, 9)
    assert G.ids("A", 10) != G.ids("B", 10) and G.counts("A", 3) != G.counts("B", 3)
    assert G.ids("B", 0) == (0, 0)                                   # no node: still no negative id
    g = G.Guard()
    for dtype, band in ((torch.int32, G.ids("B", 10)), (torch.int64, G.offsets("A", ptr)), (torch.uint8, G.flags("B")),
                        (torch.int32, G.counts("B", 24))):
        t = g.input(torch.zeros(11, dtype=dtype), band, str(dtype))
        before, after = _flat(t, 4, 0)[:4], _flat(t, 0, 4)[-4:]
        assert (before == band[0]).all() and (after == band[1]).all()
    a = g.input(torch.arange(11.0), G.floats("A"), "nan")
    assert torch.isnan(_flat(a, 1, 1)[[0, -1]]).all()
    b = g.input(torch.arange(11.0), G.floats("B"), "big")
    assert (_flat(b, 1, 1)[[0, -1]] == 1.0e30).all()
    g.check()


def test_strided_input_has_band_between_its_rows():
    g = G.Guard()
    x = torch.randn(6, 3, 52)
    v = g.input(x, G.floats("A"), "x", base_shape=(6, 3, 64), view=lambda t: t[:, :, :52])
    assert v.stride() == (192, 64, 1) and torch.equal(v, x) and v.data_ptr() % 256 == 0
    assert torch.isnan(v.as_strided((6, 3, 64), (192, 64, 1))[:, :, 52:]).all()
    v.as_strided((6, 3, 64), (192, 64, 1))[2, 1, 60] = 0.0           # a store into a gap
    assert "x: 2 bytes changed inside the input (or between its rows)" in g.problems()[0]   # NaN -> 0.0: two bytes


def test_alignment_and_patterns_of_the_views():
    g = G.Guard(1)
    for shape, dtype in (((7, 3), torch.float32), ((1,), torch.int32), ((1003, 48), torch.float32),
                         ((2, 40000), torch.int32), ((5,), torch.int64), ((61, 37, 4), torch.uint8)):
        t = g.guarded(shape, dtype, "cpu")
        assert t.data_ptr() % 256 == 0 and t.is_contiguous() and t.shape == shape
        assert bool(g.unwritten(t).all())
        row = t[0].numel() * t.element_size()
        flat = _flat(t.view(-1).view(torch.uint8), max(G.BAND_BYTES, row), max(G.BAND_BYTES, row))
        assert (flat[:max(G.BAND_BYTES, row)] == G.BAND).all() and (flat[-max(G.BAND_BYTES, row):] == G.BAND).all()
    m = g.guarded((9, 4), torch.float32, "cpu", misalign=4)
    assert m.data_ptr() % 256 == 4 and m.data_ptr() % 16 == 4
    assert G.guarded((3,), torch.float32, "cpu").data_ptr() % 256 == 0
    g.check()
    # neither pattern is a plausible value
    for byte in (G.BAND,) + G.UNWRITTEN:
        raw = torch.full((8,), byte, dtype=torch.uint8)
        assert abs(float(raw.view(torch.float32)[0])) > 1e8 and abs(int(raw.view(torch.int32)[0])) > 2 ** 28
        assert abs(int(raw.view(torch.int64)[0])) > 2 ** 60 and byte not in (0, 1, 255)
    assert len({G.BAND, *G.UNWRITTEN}) == 3


class _Square(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x):
        out, saved = torch.empty_like(x), torch.empty(x.shape)
        saved.copy_(2 * x)
        out.copy_(x * x)
        ctx.save_for_backward(saved)
        return out

    @staticmethod
    def backward(ctx, g):
        (saved,) = ctx.saved_tensors
        dx = torch.empty_like(g)
        dx.copy_(g * saved)
        return dx


def test_views_pass_through_an_autograd_function():
    g = G.Guard()
    x = _x().requires_grad_()
    with G.guarded_allocations(g, ("cpu",)):
        y = _Square.apply(x)
        y.sum().backward()
    assert len(g.arenas) == 3 and g.owns(y) and torch.equal(x.grad, 2 * x.detach())
    g.check()
    assert torch.empty is _EMPTY and torch.empty_like is _EMPTY_LIKE                # restored


def test_the_patch_is_inert_off_the_gpu():
    gen = torch.Generator().manual_seed(1)
    n, heads, C = 50, 2, 4
    deg = torch.randint(0, 5, (n,), generator=gen)
    ptr = torch.zeros(n + 1, dtype=torch.int64)
    ptr[1:] = deg.cumsum(0)
    col = torch.randint(0, n, (int(ptr[-1]),), generator=gen).to(torch.int32)
    q, k, v = (torch.randn(n, heads * C, generator=gen) for _ in range(3))
    logits = torch.randn(9, 3, 5, generator=gen)
    t = [torch.randn(6, 3, generator=gen) * 0.1 for _ in range(2)] + [torch.randn(2, 6, 3, generator=gen)] + \
        [torch.randn(6, 3, generator=gen) * 0.1] + [torch.randn(2, 6, 3, generator=gen) for _ in range(3)]

    def run():
        lp, ent = policy.actor_dist_ref(logits)
        ls, stats = loss.ppo_loss_ref(*t, None, None, 0.5)
        return [gnn.attn_aggregate_ref(q, k, v, ptr, col, heads=heads), lp, ent, ls, stats]

    want = run()
    g = G.Guard()
    with G.guarded_allocations(g):
        got = run()
        e = torch.empty(3, 4)
    assert not g.arenas and not g.owns(e)
    assert all(G.same_bits(a, b) for a, b in zip(got, want))


def test_every_kernel_entry_point_has_a_guarded_case():
    table = G.guarded_entry_points()
    assert not set(table) & G.NO_KERNEL
    assert set(table) | G.NO_KERNEL == set(_lib.SIGNATURES), set(_lib.SIGNATURES) ^ (set(table) | G.NO_KERNEL)
    here = Path(__file__).resolve().parent
    for entry, where in table.items():
        file, test = where.split("::")
        text = (here / file).read_text()
        assert re.search(rf"^def {test}\(", text, re.M), where
        assert entry in text, f"{where} does not name {entry}"
