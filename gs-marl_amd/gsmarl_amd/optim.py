"""The step after ``loss.backward()``: global-norm gradient clip and Adam.

``ClippedAdam`` does what ``torch.nn.utils.clip_grad_norm_`` followed by
``torch.optim.Adam.step`` does, for fp32 parameters on the GPU in one ABI call
(``gsm_adam_step`` in include/gsm_optim.h: two launches for up to 32 tensors),
with the learning rate and the step count on the device, so a step can be
captured into a graph and a schedule rewrites ``lr`` in place, as
``LagrangeMultiplier.lam`` is used by the loss. Two deliberate differences from
torch: a non-finite gradient norm (a NaN or an Inf in any gradient) *skips* the
update instead of overwriting every parameter with NaN, and ``.grad`` is not
rescaled in place (the clip is applied on the fly; gradients are never
written).

``clipped_adam_ref`` is the definition in plain torch (any device and dtype),
the kernel's reference and the fallback.
"""
from __future__ import annotations

import ctypes as C
import math

import torch

from . import _lib

_ptr, _stream = _lib.ptr, _lib.stream

N_STATS = 4     # norm, coef, the step count after the call, skipped


def clipped_adam_ref(params, grads, exp_avg, exp_avg_sq, step, lr, betas=(0.9, 0.999), eps: float = 1e-5,
                     max_grad_norm=10.0):
    """One ``gsm_adam_step`` in plain torch, in the dtype of ``params`` (any
    device), without a host read. ``params``, ``grads``, ``exp_avg``,
    ``exp_avg_sq``: lists of tensors of equal shapes; ``step``: the number of
    updates so far (an int or an integer tensor of one element); ``lr``: a
    float or a tensor of one element. With ``t = step``::

        norm = sqrt(sum g^2)         the squares and the sum in fp64, rounded once
        coef = min(1, max_grad_norm / (norm + 1e-6))      (None / inf: 1)
        norm not finite: nothing changes (skipped)
        else t <- t + 1,  g' = g * coef
             m <- beta1 m + (1 - beta1) g'
             v <- beta2 v + (1 - beta2) g'^2
             p <- p - lr / (1 - beta1^t) * m / (sqrt(v) / sqrt(1 - beta2^t) + eps)

    the bias corrections formed in fp64. Nothing is written: returns ``(params,
    exp_avg, exp_avg_sq, step int32 [1], stats [4])`` after the call, ``stats``
    = norm, coef (0 when skipped), the step count after the call, skipped."""
    b1, b2 = float(betas[0]), float(betas[1])
    if not params:
        raise ValueError("no parameters")
    dt, dev = params[0].dtype, params[0].device
    total = torch.zeros((), dtype=torch.float64, device=dev)
    for g in grads:
        total = total + g.detach().to(torch.float64).square().sum()
    norm = total.sqrt().to(dt)
    ok = torch.isfinite(norm)
    if max_grad_norm is None or math.isinf(max_grad_norm):
        coef = torch.ones((), dtype=dt, device=dev)
    else:
        coef = (float(max_grad_norm) / (norm + 1e-6)).clamp(max=1.0)
    step = torch.as_tensor(step, device=dev).to(torch.int32).reshape(1)
    t = (step + 1).to(torch.float64)
    bc1 = 1.0 - torch.full_like(t, b1) ** t
    bc2 = 1.0 - torch.full_like(t, b2) ** t
    lr = lr.detach().to(device=dev, dtype=torch.float64).reshape(1) if torch.is_tensor(lr) else float(lr)
    step_size = (lr / bc1).to(dt)
    bc2_sqrt = bc2.sqrt().to(dt)
    new_p, new_m, new_v = [], [], []
    for p, g, m, v in zip(params, grads, exp_avg, exp_avg_sq):
        p, g, m, v = p.detach(), g.detach().to(dt), m.detach(), v.detach()
        gc = g * coef
        m1 = b1 * m + (1.0 - b1) * gc
        v1 = b2 * v + (1.0 - b2) * (gc * gc)
        p1 = p - step_size * (m1 / (v1.sqrt() / bc2_sqrt + eps))
        new_p.append(torch.where(ok, p1, p))
        new_m.append(torch.where(ok, m1, m))
        new_v.append(torch.where(ok, v1, v))
    new_step = step + ok.to(torch.int32)
    stats = torch.stack([norm, torch.where(ok, coef, torch.zeros_like(coef)), new_step[0].to(dt), (~ok).to(dt)])
    return new_p, new_m, new_v, new_step, stats


def adam_work_floats(n_tensors: int, total_elements: int) -> int:
    """Floats of workspace ``gsm_adam_step`` wants (``gsm_adam_work_floats``)."""
    return _lib.work_floats("gsm_adam_work_floats", int(n_tensors), int(total_elements))


def _max_norm(max_grad_norm) -> float:
    return math.inf if max_grad_norm is None else float(max_grad_norm)


def _table_key(params):
    """What a cached ``_Table`` is valid for: the parameters' storage addresses
    (``p.data = ...`` and ``module.to(...)`` give a parameter another one)."""
    return tuple(map(torch.Tensor.data_ptr, params))


class _Table:
    """The host arrays of one gsm_adam_step call: p, g, m, v pointers and counts;
    ``key`` = ``_table_key`` of the parameters it was built from."""

    def __init__(self, params, exp_avg, exp_avg_sq):
        k = len(params)
        arr = C.c_void_p * k
        self.k = k
        self.key = _table_key(params)
        self.p = arr(*(t.data_ptr() if t.numel() else None for t in params))
        self.m = arr(*(t.data_ptr() if t.numel() else None for t in exp_avg))
        self.v = arr(*(t.data_ptr() if t.numel() else None for t in exp_avg_sq))
        self.g = arr()
        self.n = (C.c_int64 * k)(*(t.numel() for t in params))


def _adam_call(params, grads, exp_avg, exp_avg_sq, lr, step, betas, eps, max_grad_norm, status=None, work=None,
               stats=None, table=None):
    """One gsm_adam_step call on lists of contiguous fp32 tensors of one GPU:
    ``params``, ``exp_avg``, ``exp_avg_sq`` and ``step`` (int32 [1]) are
    updated in place. ``work`` and ``stats``: allocated here when None. Returns
    ``stats`` f32 [4]."""
    dev = lr.device
    lib = _lib.load()
    if work is None:
        work = torch.empty(adam_work_floats(len(params), sum(t.numel() for t in params)), dtype=torch.float32,
                           device=dev)
    if stats is None:
        stats = torch.empty(N_STATS, dtype=torch.float32, device=dev)
    tab = table if table is not None else _Table(params, exp_avg, exp_avg_sq)
    for i, g in enumerate(grads):
        tab.g[i] = g.data_ptr() if g.numel() else None
    rc = lib.gsm_adam_step(tab.p, tab.g, tab.m, tab.v, tab.n, tab.k, _ptr(lr), _ptr(step), float(betas[0]),
                           float(betas[1]), float(eps), _max_norm(max_grad_norm), _ptr(work), _ptr(stats),
                           _ptr(status), _stream(dev))
    _lib.check(lib, rc, None, "gsm_adam_step")
    return stats


class ClippedAdam:
    """``clip_grad_norm_(params, max_grad_norm)`` + ``Adam(lr, betas,
    eps).step()`` as ``clipped_adam_ref`` defines them: one set of
    hyper-parameters and one gradient norm per instance (two learning rates are
    two instances, each with its own norm). No weight decay, no amsgrad.

    With ``use_kernel``, when every parameter is a contiguous fp32 tensor of
    one GPU, ``step()`` is one ``gsm_adam_step`` (two launches for up to 32
    parameters with a gradient); otherwise it runs ``clipped_adam_ref`` and
    copies the result in. A parameter whose ``.grad`` is None is left out of
    that call, its moments untouched. Non-contiguous gradients are made
    contiguous. A non-finite gradient norm skips the update: no parameter,
    moment or step count changes. ``.grad`` is never written.

    ``lr`` (f32 [1], on the parameters' device) is read when the kernels run:
    write a schedule into it in place. ``step_count`` (int32 [1]) is the number
    of updates made. After a call ``stats`` holds f32 [4] (norm, coef, the step
    count after the call, skipped) and ``status`` (device int32 [1]; None
    without the kernel) the ``_lib.OPT_NONFINITE`` bit, OR-ed over the calls
    since it was last zeroed. None of them is read here, and moments, workspace
    and ``stats`` are allocated at construction, so a ``step()`` can be
    captured into a ``torch.cuda.graph`` (with gradients that are rewritten in
    place) and replayed, interleaved with eager calls.

    The kernel writes the parameters through raw pointers, which torch does not
    see, so the kernel path of ``step()`` ends with ``mark_updated()``: it
    raises ``_version`` of every parameter of the last active set (host only:
    no launch, no synchronisation), as ``copy_`` does on the fallback path.
    Caches keyed on the version (``TransformerConv._packed``) then repack, and a
    backward through a graph built before the step raises as it does after
    ``torch.optim.Adam.step``. A skipped step raises the versions too. A
    replayed captured step runs no Python: the route is ``graph.replay();
    opt.mark_updated()``.

    ``step()`` looks at the parameters again on every call, as ``torch.optim``
    does: after ``p.data = ...`` (or a ``module.to(...)`` that moved nothing off
    the device) the next eager step updates the new storage. A captured step
    cannot follow a replaced storage: the graph holds the addresses it was
    recorded with, so capture again after replacing one."""

    def __init__(self, params, lr: float = 7e-4, betas=(0.9, 0.999), eps: float = 1e-5, max_grad_norm=10.0,
                 use_kernel: bool = True):
        self.params = list(params)
        if not self.params:
            raise ValueError("no parameters")
        if len({id(p) for p in self.params}) != len(self.params):
            raise ValueError("a parameter appears twice")
        if not (0.0 <= betas[0] < 1.0 and 0.0 <= betas[1] < 1.0) or eps < 0 or lr < 0:
            raise ValueError("betas in [0, 1), eps >= 0, lr >= 0")
        if max_grad_norm is not None and not max_grad_norm >= 0:
            raise ValueError("max_grad_norm: None or >= 0")
        self.betas, self.eps = (float(betas[0]), float(betas[1])), float(eps)
        self.max_grad_norm = None if max_grad_norm is None else float(max_grad_norm)
        self.use_kernel = use_kernel
        dev = self.params[0].device
        self.lr = torch.full((1,), float(lr), dtype=torch.float32, device=dev)
        self.step_count = torch.zeros(1, dtype=torch.int32, device=dev)
        self.exp_avg = [torch.zeros_like(p, memory_format=torch.contiguous_format) for p in self.params]
        self.exp_avg_sq = [torch.zeros_like(p, memory_format=torch.contiguous_format) for p in self.params]
        self.kernel = bool(use_kernel) and all(p.is_cuda and p.device == dev and p.dtype == torch.float32 and
                                               p.is_contiguous() for p in self.params)
        self.stats = torch.zeros(N_STATS, dtype=torch.float32 if self.kernel else self.params[0].dtype, device=dev)
        self.status = self._work = None
        self._tables = {}
        self._last, self._marked = (), []            # the active set of the last step() and its parameters
        if self.kernel:
            self.status = torch.zeros(1, dtype=torch.int32, device=dev)
            self._work = torch.empty(adam_work_floats(len(self.params), sum(p.numel() for p in self.params)),
                                     dtype=torch.float32, device=dev)

    def _table(self, act, ps, ms, vs):
        """The cached host arrays of the active set ``act``, built again when a
        parameter's storage is no longer the one they name."""
        tab = self._tables.get(act)
        if tab is None or tab.key != _table_key(ps):
            if tab is not None and not all(p.device == self.lr.device and p.dtype == torch.float32 and
                                           p.is_contiguous() and p.shape == m.shape for p, m in zip(ps, ms)):
                raise ValueError("a parameter's new storage is not a contiguous fp32 tensor of the old shape on the "
                                 "optimizer's device")
            tab = self._tables[act] = _Table(ps, ms, vs)
        return tab

    def mark_updated(self):
        """Tell torch that the parameters of the last active set were written
        (``torch.autograd.graph.increment_version``; host only). ``step()``
        calls it on the kernel path; call it after replaying a captured step."""
        if self._marked:
            torch.autograd.graph.increment_version(self._marked)         # one call for the whole list

    @torch.no_grad()
    def step(self):
        gs = [p.grad for p in self.params]           # .grad is read once a parameter: the host's time is the call's
        act = tuple(i for i, g in enumerate(gs) if g is not None)
        if not act:                                  # nothing has a gradient: not an update
            return
        if len(act) == len(gs):
            ps, ms, vs = self.params, self.exp_avg, self.exp_avg_sq
        else:
            ps, gs = [self.params[i] for i in act], [gs[i] for i in act]
            ms, vs = [self.exp_avg[i] for i in act], [self.exp_avg_sq[i] for i in act]
        if act != self._last:
            self._last, self._marked = act, list(ps)
        if not self.kernel:
            new_p, new_m, new_v, new_step, stats = clipped_adam_ref(ps, gs, ms, vs, self.step_count, self.lr,
                                                                    self.betas, self.eps, self.max_grad_norm)
            for dst, src in zip(ps + ms + vs, new_p + new_m + new_v):
                dst.copy_(src)
            self.step_count.copy_(new_step)
            self.stats.copy_(stats)
            return
        dev = self.lr.device                         # every parameter's: by construction, and by _table after p.data = ...
        for p, g in zip(ps, gs):
            if g.dtype != torch.float32 or g.device != dev or g.shape != p.shape:
                raise ValueError("a gradient is not an fp32 tensor of its parameter's shape and device")
        gs = [g if g.is_contiguous() else g.contiguous() for g in gs]
        _adam_call(ps, gs, ms, vs, self.lr, self.step_count, self.betas, self.eps, self.max_grad_norm, self.status,
                   self._work, self.stats, self._table(act, ps, ms, vs))
        self.mark_updated()

    def zero_grad(self, set_to_none: bool = True):
        for p in self.params:
            if p.grad is None:
                continue
            if set_to_none:
                p.grad = None
            else:
                p.grad.detach_().zero_()

    def state_dict(self):
        return dict(step=self.step_count.clone(), lr=self.lr.clone(), exp_avg=[m.clone() for m in self.exp_avg],
                    exp_avg_sq=[v.clone() for v in self.exp_avg_sq], betas=self.betas, eps=self.eps,
                    max_grad_norm=self.max_grad_norm)

    @torch.no_grad()
    def load_state_dict(self, state):
        """Copies into the instance's own tensors (a captured step stays valid)."""
        if len(state["exp_avg"]) != len(self.params) or len(state["exp_avg_sq"]) != len(self.params):
            raise ValueError("the state is of another parameter list")
        for dst, src in zip(self.exp_avg + self.exp_avg_sq, list(state["exp_avg"]) + list(state["exp_avg_sq"])):
            if dst.shape != src.shape:
                raise ValueError("the state is of another parameter list")
            dst.copy_(src)
        self.step_count.copy_(state["step"])
        self.lr.copy_(state["lr"])
        self.betas, self.eps = tuple(float(b) for b in state["betas"]), float(state["eps"])
        self.max_grad_norm = state["max_grad_norm"]
