"""Guard bands: where a kernel reads and writes, checked with plain tensors.

A guarded tensor is a view into a larger arena with a band on either side. A
stray store lands in a band, which the test owns and compares afterwards; a
stray load returns the band's contents, which the test chooses (two fills, A
and B, both legal for the array), so a result that depends on memory outside
an input differs between the fills. Outputs and workspaces start from an
*unwritten* byte pattern, so an element a kernel skipped is seen, and they
start from two different patterns, so a kernel that relies on what its
workspace held is seen too. No launch in csrc/ uses a float atomic: every
comparison here is bit for bit.

    g = Guard(prefill=0)
    x = g.input(values, floats("A"), "x")          # an input, band contents chosen
    with guarded_allocations(g):                    # the wrapper's own torch.empty
        out = wrapper(x)                            #   outputs, statistics and work buffers
    g.check()                                       # (a) no band changed, no input changed
    assert not g.unwritten(out).any()               # (b) every element written

``run_case`` makes the five assertions of a GPU case in three guarded runs:
(a) and (b) in each, (d) fill A against fill B, (e) prefill 0 against prefill
1, (c) the bits of the plain call, each named when it fails.

The byte patterns. BAND = 0xE9 (fp32 -3.5e25, int32 -370546199), UNWRITTEN =
0xCD (fp32 -4.3e8, int32 -842150451) and 0x5E (fp32 4.0e18, int32 1583242846):
none is a value a kernel here produces as fp32, int32, int64 or in all four
bytes of an rgba pixel, and both prefills are far from negligible as floats,
so a sum that starts from one does not round back to the right answer.

Entry points of include/gsm.h that launch a kernel, and the guarded case of
each (tests/test_guard_ref.py compares this list with ``_lib.SIGNATURES``):

    gsm_attn_aggregate          test_gpu_guard_attn.py::test_attention_forward
    gsm_attn_aggregate_fwd      test_gpu_guard_attn.py::test_attention_forward_backward
    gsm_attn_aggregate_bwd      test_gpu_guard_attn.py::test_attention_forward_backward
    gsm_env_conv                test_gpu_guard_env_conv.py::test_env_conv_forward
    gsm_env_conv_fwd            test_gpu_guard_env_conv.py::test_env_conv_forward_backward
    gsm_env_conv_bwd            test_gpu_guard_env_conv.py::test_env_conv_forward_backward
    gsm_actor_sample            test_gpu_guard_heads.py::test_actor_sample
    gsm_actor_eval              test_gpu_guard_heads.py::test_actor_eval_and_backward
    gsm_actor_eval_bwd          test_gpu_guard_heads.py::test_actor_eval_and_backward
    gsm_critic_eval             test_gpu_guard_heads.py::test_critic_eval
    gsm_critic_eval_bwd         test_gpu_guard_heads.py::test_critic_backward
    gsm_ppo_loss                test_gpu_guard_loss.py::test_ppo_loss
    gsm_gae                     test_gpu_guard_loss.py::test_gae
    gsm_graph_batch_ptr         test_gpu_guard_batch.py::test_graph_batch
    gsm_graph_batch_gather      test_gpu_guard_batch.py::test_graph_batch
    gsm_render                  test_gpu_guard_batch.py::test_render
    gsm_reset                   test_gpu_guard_env.py::test_env_calls
    gsm_step                    test_gpu_guard_env.py::test_env_calls
    gsm_observe                 test_gpu_guard_env.py::test_env_calls
    gsm_set_state               test_gpu_guard_env.py::test_env_calls
    gsm_get_state               test_gpu_guard_env.py::test_env_calls
    gsm_graph_capture           test_gpu_guard_env.py::test_env_calls
    gsm_graph_launch            test_gpu_guard_env.py::test_env_calls
    gsm_step_into               test_gpu_guard_env.py::test_redirected_outputs
    gsm_observe_into            test_gpu_guard_env.py::test_redirected_outputs
    gsm_graph_capture_into      test_gpu_guard_env.py::test_redirected_outputs
"""
from __future__ import annotations

import contextlib
import math

import torch

_EMPTY, _EMPTY_LIKE = torch.empty, torch.empty_like                  # the real ones, whatever is patched in
BAND = 0xE9
UNWRITTEN = (0xCD, 0x5E)
BAND_BYTES = 64 * 1024
ALIGN = 256

# entry points that launch nothing: host queries, handle management, readbacks of a status word
NO_KERNEL = {
    "gsm_abi_version", "gsm_query_sizes", "gsm_create", "gsm_bind", "gsm_destroy", "gsm_last_error",
    "gsm_graph_info", "gsm_graph_roll_status", "gsm_graph_roll_placement", "gsm_graph_kernel_ms",
    "gsm_debug_set_stamps", "gsm_attn_backward_work_floats", "gsm_env_conv_backward_work_floats",
    "gsm_actor_backward_work_floats", "gsm_critic_backward_work_floats", "gsm_ppo_loss_work_floats",
}


def guarded_entry_points() -> dict:
    """``{entry point: "file::test"}`` read off the module docstring."""
    table = {}
    for line in __doc__.splitlines():
        parts = line.split()
        if len(parts) == 2 and parts[0].startswith("gsm_") and "::" in parts[1]:
            table[parts[0]] = parts[1]
    return table


def _up(n, m=ALIGN):
    return -(-int(n) // m) * m


def _itemsize(dtype):
    return _EMPTY(0, dtype=dtype).element_size()


# ---- the two fills of an input's bands: (front value, back value), legal for the array --------------
def floats(fill):
    """NaN in fill A, a large finite value in fill B."""
    v = float("nan") if fill == "A" else 1.0e30
    return v, v


def ids(fill, n):
    """Node ids: 0 in A, n - 1 in B."""
    v = 0 if fill == "A" else max(int(n) - 1, 0)
    return v, v


def offsets(fill, t):
    """Offsets: the first value before the array and the last after it (a stray range is empty), both fills."""
    return int(t.reshape(-1)[0]), int(t.reshape(-1)[-1])


def actions(fill, n_actions):
    v = 0 if fill == "A" else int(n_actions) - 1
    return v, v


def counts(fill, n):
    v = 0 if fill == "A" else int(n)
    return v, v


def flags(fill):
    """``done`` and masks: 0 in A, 1 in B."""
    v = 0 if fill == "A" else 1
    return v, v


class _Arena:
    def __init__(self, name, role, store, span, view, snapshot, keep, prefill, lo, nbytes):
        self.name, self.role, self.store, self.span, self.lo, self.nbytes = name, role, store, span, lo, nbytes
        self.view, self.snapshot, self.keep, self.prefill = view, snapshot, keep, prefill

    def holds(self, t):
        lo = self.span.data_ptr()
        return lo <= t.data_ptr() < lo + self.span.numel()


class Guard:
    """The arenas of one guarded call. ``prefill`` picks the unwritten pattern (0 or 1)."""

    def __init__(self, prefill: int = 0):
        self.prefill = UNWRITTEN[prefill]
        self.arenas = []

    # -------------------------------------------------------------- building
    def _arena(self, base_shape, dtype, device, misalign):
        size = _itemsize(dtype)
        base_shape = tuple(int(s) for s in base_shape)
        nbytes = size * math.prod(base_shape)
        row = size * (math.prod(base_shape[1:]) if len(base_shape) > 1 else 1)
        band = _up(max(BAND_BYTES, row))
        if misalign % size:
            raise ValueError("misalign: a multiple of the element size")
        total = band + misalign + _up(nbytes + band)
        store = _EMPTY(total + ALIGN, dtype=torch.uint8, device=device)
        shift = (-store.data_ptr()) % ALIGN
        span = store[shift:shift + total]
        lo = band + misalign
        inner = span[lo:lo + nbytes].view(dtype).view(base_shape)
        assert (inner.data_ptr() - misalign) % ALIGN == 0 and inner.is_contiguous()
        return store, span, lo, nbytes, inner

    def guarded(self, shape, dtype, device, fill=None, *, name=None, misalign=0):
        """An output or workspace: bands of BAND bytes, the interior prefilled
        with the unwritten pattern (or ``fill``, a value of ``dtype``)."""
        store, span, lo, nbytes, inner = self._arena(shape, dtype, device, misalign)
        span.fill_(BAND)
        if fill is None:
            span[lo:lo + nbytes].fill_(self.prefill)
        else:
            inner.fill_(fill)
        keep = torch.ones_like(span, dtype=torch.bool)
        keep[lo:lo + nbytes] = False
        self.arenas.append(_Arena(name or f"alloc{len(self.arenas)}{tuple(inner.shape)}", "output", store, span,
                                  inner, span.clone(), keep, self.prefill if fill is None else None, lo, nbytes))
        return inner

    def input(self, values, band, name, *, misalign=0, base_shape=None, view=None):
        """An input: a copy of ``values`` inside an arena whose bands hold
        ``band = (front, back)``, values of the tensor's dtype. With
        ``base_shape`` and ``view`` the arena holds a wider tensor and the
        input is ``view(wider)``: the gaps between its rows are band too (they
        hold the front value). Nothing of an input's arena may change."""
        values = values.detach()
        dtype, device = values.dtype, values.device
        size = _itemsize(dtype)
        store, span, lo, nbytes, inner = self._arena(base_shape or values.shape, dtype, device, misalign)
        front, back = band
        span[:lo].view(dtype).fill_(front)
        tail = span[lo + nbytes:]
        tail[:tail.numel() // size * size].view(dtype).fill_(back)
        inner.fill_(front)
        t = view(inner) if view is not None else inner
        t.copy_(values)
        self.arenas.append(_Arena(name, "input", store, span, t, span.clone(), None, None, lo, nbytes))
        return t

    def state(self, values, band, name):
        """A buffer a kernel both reads and writes (a bound env buffer, a
        rollout-buffer field): a copy of ``values`` between bands that hold
        ``band = (front, back)``, legal values of the dtype as for an input;
        only the bands have to stay as they are."""
        t = self.input(values, band, name)
        a = self.arenas[-1]
        a.role = "state"
        a.keep = torch.ones_like(a.span, dtype=torch.bool)
        a.keep[a.lo:a.lo + a.nbytes] = False
        return t

    # -------------------------------------------------------------- checking
    def _of(self, t):
        for a in self.arenas:
            if a.holds(t):
                return a
        return None

    def owns(self, t) -> bool:
        return self._of(t) is not None

    def problems(self):
        """One line per arena with a changed band (or a changed input)."""
        out = []
        for a in self.arenas:
            diff = a.span != a.snapshot
            if a.keep is not None:
                diff &= a.keep
            if not bool(diff.any()):
                continue
            at = diff.nonzero()[:, 0]
            lo, hi = a.lo, a.lo + a.nbytes
            first, last = int(at[0]), int(at[-1])
            inside = a.role == "input" and bool(((at >= lo) & (at < hi)).any())
            sides = [s for s, hit in (("before the start", first < lo), ("after the end", last >= hi),
                                      ("inside the input (or between its rows)", inside)) if hit]
            out.append(f"{a.name}: {int(diff.sum())} bytes changed {' and '.join(sides)}; "
                       f"first at byte {first - lo:+d}, last at byte {last - lo:+d} relative to the tensor's start "
                       f"(its end: {hi - lo})")
        return out

    def check(self):
        """(a): every band of every arena still holds its pattern, and no input was written."""
        bad = self.problems()
        assert not bad, "guard bands changed:\n  " + "\n  ".join(bad)

    def unwritten(self, t):
        """bool, ``t``'s shape: the elements whose bytes are all still the unwritten pattern."""
        a = self._of(t)
        if a is None or a.prefill is None:
            raise ValueError("not a prefilled tensor of this guard")
        if t.numel() == 0:
            return torch.zeros(t.shape, dtype=torch.bool, device=t.device)
        b = t.contiguous().view(-1).view(torch.uint8).view(t.numel(), t.element_size())
        return (b == a.prefill).all(1).view(t.shape)


def guarded(shape, dtype, device, fill=None, *, guard=None, name=None, misalign=0):
    """``Guard.guarded`` on ``guard`` (a fresh one by default). Returns the tensor; with no ``guard`` passed
    the guard is reachable as ``tensor.guard``."""
    g = guard if guard is not None else Guard()
    t = g.guarded(shape, dtype, device, fill, name=name, misalign=misalign)
    if guard is None:
        t.guard = g
    return t


@contextlib.contextmanager
def guarded_allocations(guard: Guard, device_types=("cuda",)):
    """Replace ``torch.empty`` and ``torch.empty_like`` by the guarded form for
    tensors on ``device_types`` while the block runs; the arenas are recorded
    in ``guard``. Calls this cannot express (other keywords, no elements, other
    devices) go to the original, so off the GPU the patch is inert."""
    empty, empty_like = _EMPTY, _EMPTY_LIKE
    before = torch.empty, torch.empty_like

    def on(device):
        device = torch.device(device) if device is not None else empty(0).device
        return device.type in device_types

    def g_empty(*size, dtype=None, device=None, **kw):
        if kw or not on(device):
            return empty(*size, dtype=dtype, device=device, **kw)
        shape = tuple(size[0]) if len(size) == 1 and not isinstance(size[0], int) else tuple(size)
        if math.prod(shape) == 0:
            return empty(*size, dtype=dtype, device=device)
        return guard.guarded(shape, dtype or torch.get_default_dtype(), device if device is not None else "cpu")

    def g_empty_like(t, dtype=None, device=None, **kw):
        device = t.device if device is None else device
        if kw or not on(device) or t.numel() == 0:
            return empty_like(t, dtype=dtype, device=device, **kw)
        return guard.guarded(tuple(t.shape), dtype or t.dtype, device)

    torch.empty, torch.empty_like = g_empty, g_empty_like
    try:
        yield guard
    finally:
        torch.empty, torch.empty_like = before


def same_bits(a, b):
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    if a.numel() == 0:
        return True
    return torch.equal(a.contiguous().view(-1).view(torch.uint8), b.contiguous().view(-1).view(torch.uint8))


class In:
    """An input of ``run_case``: the values, ``fills(fill) -> (front, back)``,
    and the layout (``misalign`` bytes, or ``base_shape`` + ``view``)."""

    def __init__(self, values, fills, **layout):
        self.values, self.fills, self.layout = values, fills, layout


def run_case(call, inputs: dict, exceptions: dict = None, plain=None, device_types=("cuda",), work=()):
    """The five assertions of a case. ``call(**tensors)`` runs the product path
    and returns ``{name: output tensor or None}``; ``inputs`` maps its argument
    names to ``In`` (guarded) or anything else (passed as is). Three guarded
    runs: (fill A, prefill 0), (fill B, prefill 0), (fill A, prefill 1). Each is
    held to (a) and (b); then the first against the second is (d), the first
    against the third (e), and the first against the plain call (c), named in
    that order, so a failure says which dependence it is. ``exceptions``:
    ``{output name: f(outputs) -> bool mask}`` of the elements the contract
    leaves unwritten; they are left out of (b) and of the comparisons. What the
    wrapper allocated and did not return (saved statistics, workspaces) is
    held to (a), (b), (d) and (e); it has no plain twin. ``work``: the shapes of
    the workspaces. A workspace is sized for the largest launch (the grid cap,
    the edge limit), so any of its elements may stay unwritten; what two runs
    both wrote has the same bits, and that no output depends on the rest is
    what (e) shows. Every shape in ``work`` has to match an allocation made
    under guard in every run: a workspace that stops coming from torch.empty
    fails here instead of leaving the check. Returns the plain call's outputs."""
    exceptions = exceptions or {}
    work = {tuple(w) for w in work if math.prod(w)}
    raw = {k: (v.values if isinstance(v, In) else v) for k, v in inputs.items()}
    if plain is None:
        plain = call(**raw)
    zero = lambda t: torch.zeros((), dtype=t.dtype, device=t.device)
    runs = []
    for fill, prefill in (("A", 0), ("B", 0), ("A", 1)):
        g = Guard(prefill)
        args = {k: (g.input(v.values, v.fills(fill), k, **v.layout) if isinstance(v, In) else v)
                for k, v in inputs.items()}
        with guarded_allocations(g, device_types):
            outs = call(**args)
        if any(a.span.is_cuda for a in g.arenas):
            torch.cuda.synchronize()
        what = f"fill {fill}, prefill {prefill}"
        g.check()                                                                  # (a)
        assert set(outs) == set(plain), what
        named = {}
        for name, o in outs.items():
            if o is None:
                assert plain[name] is None, (what, name)
                continue
            assert o.shape == plain[name].shape and o.dtype == plain[name].dtype, (what, name)
            if o.numel() == 0:
                continue
            assert g.owns(o), f"{what}: output {name} was not allocated under guard"
            free = exceptions[name](outs) if name in exceptions else torch.zeros_like(o, dtype=torch.bool)
            left = g.unwritten(o) & ~free
            assert not bool(left.any()), (f"{what}: {int(left.sum())} elements of {name} never written, "     # (b)
                                          f"first at {left.nonzero()[0].tolist()} of {tuple(o.shape)}")
            named[name] = (o, free)
        rest, seen = [], set()
        for a in g.arenas:
            if a.role != "output" or any(a.holds(o) for o, _ in named.values()):
                continue
            left = g.unwritten(a.view)
            if tuple(a.view.shape) in work:
                seen.add(tuple(a.view.shape))
            else:
                assert not bool(left.any()), f"{what}: {int(left.sum())} elements of {a.name} never written"
            rest.append((a.name, a.view, left))
        assert seen == work, f"{what}: no allocation under guard has the workspace shape {sorted(work - seen)}"
        runs.append((what, named, rest))

    def differing(this, other):
        """The first tensor of run ``this`` whose bits are not those of run ``other``."""
        for name, (o, free) in this[1].items():
            p, free_p = other[1][name]
            skip = free | free_p
            if not same_bits(torch.where(skip, zero(o), o), torch.where(skip, zero(p), p)):
                return name
        assert [n for n, _, _ in this[2]] == [n for n, _, _ in other[2]], (this[0], other[0])
        for (name, v, left), (_, v0, left0) in zip(this[2], other[2]):
            skip = left | left0
            if not same_bits(torch.where(skip, zero(v), v), torch.where(skip, zero(v0), v0)):
                return f"{name} (not returned)"
        return None

    first, other_fill, other_prefill = runs
    bad = differing(first, other_fill)
    assert bad is None, f"(d) {bad} depends on memory outside an input: {first[0]} and {other_fill[0]} differ"
    bad = differing(first, other_prefill)
    assert bad is None, (f"(e) {bad} depends on what an output or a workspace held before the call: {first[0]} and "
                         f"{other_prefill[0]} differ")
    for name, (o, free) in first[1].items():
        p = plain[name]
        assert same_bits(torch.where(free, zero(o), o), torch.where(free, zero(p), p)), \
            f"(c) {first[0]}: {name} differs from the plain call"
    return plain
