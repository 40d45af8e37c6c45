"""The actor head: policy features -> MLP -> categorical distribution.

``ActorHead.act`` turns the ``[B, N, HC]`` agent features of
``TransformerConv.forward_env(rows="agents")`` into the int32 action indices
``GpuBatchEnv.step`` takes, with their log-probabilities, in one HIP launch
(``gsm_actor_sample`` in include/gsm.h). The draw is Philox4x32-10 keyed by
``(seed, global env id, draw, agent)`` like the env layouts, so a shard samples
what its slice of the full batch samples, and the draw number can live in a
device counter that a captured graph advances. ``ActorHead.evaluate`` gives
the log-probability and entropy of stored actions for the PPO / Lagrangian
update (``gsm_actor_eval``), with ``kernel_backward`` on the HIP backward too
(``gsm_actor_eval_bwd``). For the same inputs ``evaluate`` returns the bits
``act`` returned, so the PPO ratio is exactly 1 before the first update.

The plain-torch restatements (any device and dtype, differentiable where that
applies) are the kernels' reference and the fallback of ``evaluate``:
``actor_logits_ref``, ``actor_dist_ref``, ``actor_uniform_ref``,
``actor_sample_ref`` and ``actor_eval_bwd_ref``.

``CriticHead`` is the centralised critic beside it: per-env mean pooling, an
MLP on ``[pool | x]`` and one or two values a row in one launch
(``gsm_critic_eval``, ``gsm_critic_eval_bwd``), with ``critic_values_ref`` /
``critic_bwd_ref`` as restatements and ``PopArt`` for the value normalisation
whose statistics the kernel denormalises with.
"""
from __future__ import annotations

from typing import Optional

import torch

from . import _lib

TAG_POLICY = 3          # kTagPolicy in gsm_philox.h
HIDDEN_SIZES = (0, 16, 32, 64)
MAX_IN_FEATURES, MAX_ACTIONS = 128, 8


def actor_logits_ref(x, w1, b1, w2, b2):
    """``W2 relu(W1 x + b1) + b2`` over the last dimension of ``x``; with
    ``w1 is None`` the linear head ``W2 x + b2``."""
    h = torch.relu(x @ w1.t() + b1) if w1 is not None else x
    return h @ w2.t() + b2


def actor_dist_ref(logits):
    """``(logp_all [..., A], entropy [...])`` in the kernel's operation order:
    ``m = max l; e = exp(l - m); s = e_0 + e_1 + ..; logp = (l - m) - log s;
    entropy = log s - (sum_a e_a (l_a - m)) / s``."""
    z = logits - logits.max(-1, keepdim=True)[0]
    e = torch.exp(z)
    s, t = e[..., 0], e[..., 0] * z[..., 0]
    for a in range(1, logits.shape[-1]):
        s = s + e[..., a]
        t = t + e[..., a] * z[..., a]
    logs = torch.log(s)
    return z - logs[..., None], logs - t / s


def _mulhilo32(m: int, c):
    """``(hi, lo)`` 32-bit halves of ``m * c`` for int64 tensors ``c < 2^32``."""
    lo = (c * m) & 0xFFFFFFFF                                # the wrapped product keeps its low bits
    hi = ((c >> 16) * m + (((c & 0xFFFF) * m) >> 16)) >> 16
    return hi, lo


def actor_uniform_ref(n_envs: int, n_agents: int, seed: int, env_base: int = 0, draw=0, device=None):
    """The uniforms ``gsm_actor_sample`` draws, f32 ``[n_envs, n_agents]``: one
    Philox4x32-10 call per row, counter ``(agent, draw, env_base + env, 3)``,
    key ``(seed lo32, seed hi32)``, ``u = (x0 >> 8) * 2^-24``. ``draw``: an int
    or an int64 tensor (a device counter). Plain torch integer arithmetic."""
    dev = torch.device(device) if device is not None else (draw.device if torch.is_tensor(draw) else None)
    i64 = dict(dtype=torch.int64, device=dev)
    c0 = torch.arange(n_agents, **i64)[None, :].expand(n_envs, n_agents)
    c2 = ((torch.arange(n_envs, **i64) + int(env_base)) & 0xFFFFFFFF)[:, None].expand(n_envs, n_agents)
    d = draw.to(**i64).reshape(-1)[0] if torch.is_tensor(draw) else torch.tensor(int(draw), **i64)
    c1 = (d & 0xFFFFFFFF).expand(n_envs, n_agents)
    c3 = torch.full((n_envs, n_agents), TAG_POLICY, **i64)
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    k0, k1 = seed & 0xFFFFFFFF, seed >> 32
    for r in range(10):
        if r:
            k0, k1 = (k0 + 0x9E3779B9) & 0xFFFFFFFF, (k1 + 0xBB67AE85) & 0xFFFFFFFF
        hi0, lo0 = _mulhilo32(0xD2511F53, c0)
        hi1, lo1 = _mulhilo32(0xCD9E8D57, c2)
        c0, c1, c2, c3 = hi1 ^ c1 ^ k0, lo1, hi0 ^ c3 ^ k1, lo0
    return (c0 >> 8).to(torch.float32) * 2.0 ** -24


def actor_sample_ref(logits, u):
    """The sampling rule of ``gsm_actor_sample`` with the uniforms given:
    ``t = u s; c = 0; c = c + e_a`` for ``a`` ascending; the action is the
    first ``a`` with ``t < c``, the last action if none. int32, ``u``'s shape."""
    A = logits.shape[-1]
    e = torch.exp(logits - logits.max(-1, keepdim=True)[0])
    s = e[..., 0]
    for a in range(1, A):
        s = s + e[..., a]
    t = u.to(logits.dtype) * s
    c = torch.zeros_like(s)
    act = torch.full(s.shape, A - 1, dtype=torch.int32, device=logits.device)
    found = torch.zeros(s.shape, dtype=torch.bool, device=logits.device)
    for a in range(A):
        c = c + e[..., a]
        hit = (t < c) & ~found
        act = torch.where(hit, torch.full_like(act, a), act)
        found = found | hit
    return act


def actor_eval_bwd_ref(g_logp, g_ent, x, w1, b1, w2, b2, actions):
    """The gradients of ``evaluate`` written out (the formulas of
    ``gsm_actor_eval_bwd``): ``x`` [R, in], ``actions`` [R], ``g_logp`` [R],
    ``g_ent`` [R] or None. With ``p = softmax(l)`` and ``H`` the entropy::

        dlogit_a = g_logp (1[a = action] - p_a) - g_ent p_a (log p_a + H)
        db2 = sum_r dlogit;  dW2 = sum_r dlogit (x) h
        dh = W2^T dlogit where h > 0;  db1 = sum_r dh;  dW1 = sum_r dh (x) x
        dx = W1^T dh

    Returns ``(dw1, db1, dw2, db2, dx)``; ``dw1 = db1 = None`` for the linear
    head (``w1 is None``), where ``dW2 = sum_r dlogit (x) x``, ``dx = W2^T dlogit``."""
    h = torch.relu(x @ w1.t() + b1) if w1 is not None else x
    logp_all, H = actor_dist_ref(h @ w2.t() + b2)
    p = torch.exp(logp_all)
    onehot = torch.nn.functional.one_hot(actions.to(torch.int64), w2.shape[0]).to(x.dtype)
    dl = g_logp[:, None] * (onehot - p)
    if g_ent is not None:
        dl = dl - g_ent[:, None] * p * (logp_all + H[:, None])
    db2, dw2 = dl.sum(0), dl.t() @ h
    dh = dl @ w2
    if w1 is None:
        return None, None, dw2, db2, dh
    dh = dh * (h > 0).to(x.dtype)
    return dh.t() @ x, dh.sum(0), dw2, db2, dh @ w1


_ptr, _stream = _lib.ptr, _lib.stream


def _rows(x):
    """``x`` [B, N, in] as the kernels read it: ``(tensor, row stride)``: the
    tensor itself when its rows are evenly strided, 16-byte aligned views of
    contiguous features (a slice of wider rows), a contiguous copy otherwise."""
    B, N, F = x.shape
    if x.numel() == 0:
        return x, F
    if N > 1:
        s, even = x.stride(1), B == 1 or x.stride(0) == N * x.stride(1)
    else:
        s, even = (x.stride(0) if B > 1 else F), True
    if x.stride(2) == 1 and even and s >= F and s % 4 == 0 and x.data_ptr() % 16 == 0:
        return x, int(s)
    x = x.contiguous()
    if x.data_ptr() % 16:
        x = x.clone()
    return x, F


def _actor_eval(x, w1, b1, w2, b2, actions, status):
    """One gsm_actor_eval launch. Returns ``(logp, entropy, x as read, row stride)``."""
    B, N, F = x.shape
    xk, stride = _rows(x)
    lib = _lib.load()
    hidden, nA = (int(w1.shape[0]) if w1 is not None else 0), int(w2.shape[0])
    logp = torch.empty(B, N, dtype=torch.float32, device=x.device)
    ent = torch.empty(B, N, dtype=torch.float32, device=x.device)
    rc = lib.gsm_actor_eval(_ptr(xk) if B else None, stride, _ptr(w1), _ptr(b1), _ptr(w2), _ptr(b2), int(B), int(N),
                            int(F), hidden, nA, _ptr(actions), _ptr(logp), _ptr(ent), _ptr(status), _stream(x.device))
    _lib.check(lib, rc, None, "gsm_actor_eval")
    return logp, ent, xk, stride


class _ActorEvalFn(torch.autograd.Function):
    """gsm_actor_eval / gsm_actor_eval_bwd (include/gsm.h)."""

    @staticmethod
    def forward(ctx, x, w1, b1, w2, b2, actions, status):
        logp, ent, xk, stride = _actor_eval(x, w1, b1, w2, b2, actions, status)
        ctx.save_for_backward(xk, w1, b1, w2, b2, actions, status)
        ctx.stride = stride
        return logp, ent

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g_logp, g_ent):
        xk, w1, b1, w2, b2, actions, status = ctx.saved_tensors
        B, N, F = xk.shape
        dev = xk.device
        lib = _lib.load()
        hidden, nA = (int(w1.shape[0]) if w1 is not None else 0), int(w2.shape[0])
        g_logp = g_logp.to(torch.float32).contiguous()
        g_ent = g_ent.to(torch.float32).contiguous()
        work = torch.empty(_lib.work_floats("gsm_actor_backward_work_floats", int(F), hidden, nA),
                           dtype=torch.float32, device=dev)
        dw1 = torch.empty_like(w1) if w1 is not None else None
        db1 = torch.empty_like(b1) if b1 is not None else None
        dw2, db2 = torch.empty_like(w2), torch.empty_like(b2)
        dx = torch.empty(B, N, F, dtype=torch.float32, device=dev) if ctx.needs_input_grad[0] else None
        rc = lib.gsm_actor_eval_bwd(_ptr(g_logp), _ptr(g_ent), _ptr(xk) if B else None, ctx.stride, _ptr(w1), _ptr(b1),
                                    _ptr(w2), _ptr(b2), int(B), int(N), int(F), hidden, nA, _ptr(actions), _ptr(work),
                                    _ptr(dw1), _ptr(db1), _ptr(dw2), _ptr(db2), _ptr(dx) if B else None,
                                    _ptr(status), _stream(dev))
        _lib.check(lib, rc, None, "gsm_actor_eval_bwd")
        return dx, dw1, db1, dw2, db2, None, None


class ActorHead(torch.nn.Module):
    """``lin2(relu(lin1(x)))`` -> a categorical distribution over
    ``n_actions`` discrete actions; ``hidden=0`` is the linear head (no
    ``lin1``). On the GPU, with ``use_kernel``, ``act`` and the gradient-free
    ``evaluate`` are one HIP launch each; with ``kernel_backward`` the training
    path of ``evaluate`` runs on the kernels too (forward and backward). The
    kernels' shape limits: fp32, ``in_features`` a multiple of 4 in [4, 128],
    ``hidden`` 0, 16, 32 or 64, 2 to 8 actions. After a kernel call ``status``
    holds the launch's status word (device int32 [1], ``_lib.ACTOR_*`` bits:
    a row with a non-finite logit, a stored action out of range); it is not
    read here, so every call can be captured into a graph."""

    def __init__(self, in_features: int, hidden: int = 64, n_actions: int = 5, use_kernel: bool = True,
                 kernel_backward: bool = False):
        super().__init__()
        self.in_features, self.hidden, self.n_actions = int(in_features), int(hidden), int(n_actions)
        self.lin1 = torch.nn.Linear(in_features, hidden) if hidden else None
        self.lin2 = torch.nn.Linear(hidden if hidden else in_features, n_actions)
        self.use_kernel = use_kernel
        self.kernel_backward = kernel_backward
        self.status = None

    def _weights(self):
        l1 = self.lin1
        return (l1.weight if l1 is not None else None, l1.bias if l1 is not None else None,
                self.lin2.weight, self.lin2.bias)

    def _kernel_shapes(self, x):
        if not (self.use_kernel and x.is_cuda and x.dtype == torch.float32 and x.dim() == 3):
            return False
        if any(p.dtype != torch.float32 or not p.is_contiguous() for p in self.parameters()):
            return False
        F = self.in_features
        return (x.shape[2] == F and 4 <= F <= MAX_IN_FEATURES and F % 4 == 0 and self.hidden in HIDDEN_SIZES and
                2 <= self.n_actions <= MAX_ACTIONS and x.shape[0] * x.shape[1] < 2 ** 31)

    def logits(self, x):
        """The logits in plain torch (differentiable)."""
        return actor_logits_ref(x, *self._weights())

    @torch.no_grad()
    def act(self, x, seed: int, env_base: int = 0, draw: int = 0, draw_counter: Optional[torch.Tensor] = None,
            deterministic: bool = False, entropy: bool = False, logits: bool = False):
        """Sample (or, with ``deterministic``, take the first argmax of) one
        action per row of ``x`` [B, N, in_features] on the GPU. Returns
        ``(actions int32 [B, N], logp f32 [B, N])``, then the entropy [B, N]
        and the logits [B, N, n_actions] when asked for. The draw of row
        ``(b, i)`` depends on ``(seed, env_base + b, i, draw + draw_counter)``
        alone; ``draw_counter`` is a device int64 [1] read by the kernel at
        run time (advance it inside a captured graph with ``add_``). One HIP
        launch (``gsm_actor_sample``) with ``use_kernel`` inside the kernels'
        shape limits, the torch restatements otherwise. No gradients. Off the
        GPU it raises ``GsmError``: the references take any device."""
        if not x.is_cuda:
            raise _lib.GsmError("ActorHead.act needs a ROCm GPU; use actor_logits_ref / actor_sample_ref on the CPU")
        if x.dim() != 3 or x.shape[2] != self.in_features:
            raise ValueError("x: [B, N, in_features]")
        if draw_counter is not None and (draw_counter.dtype != torch.int64 or draw_counter.device != x.device or
                                         draw_counter.numel() != 1):
            raise ValueError(f"draw_counter: an int64 tensor of one element on {x.device}")
        B, N, F = x.shape
        dev = x.device
        if not self._kernel_shapes(x):
            l = self.logits(x)
            logp_all, ent = actor_dist_ref(l)
            if deterministic:
                act = l.argmax(-1).to(torch.int32)
            else:
                d = draw_counter + int(draw) if draw_counter is not None else int(draw)
                act = actor_sample_ref(l, actor_uniform_ref(B, N, seed, env_base, d, dev))
            logp = logp_all.gather(-1, act.to(torch.int64)[..., None])[..., 0]
            return (act, logp) + ((ent,) if entropy else ()) + ((l,) if logits else ())
        xk, stride = _rows(x)
        lib = _lib.load()
        w1, b1, w2, b2 = self._weights()
        actions = torch.empty(B, N, dtype=torch.int32, device=dev)
        logp = torch.empty(B, N, dtype=torch.float32, device=dev)
        ent = torch.empty(B, N, dtype=torch.float32, device=dev) if entropy else None
        lout = torch.empty(B, N, self.n_actions, dtype=torch.float32, device=dev) if logits else None
        self.status = torch.zeros(1, dtype=torch.int32, device=dev)
        rc = lib.gsm_actor_sample(_ptr(xk) if B * N else None, stride, _ptr(w1), _ptr(b1), _ptr(w2), _ptr(b2), int(B),
                                  int(N), int(F), self.hidden, self.n_actions, int(seed) & 0xFFFFFFFFFFFFFFFF,
                                  int(env_base), int(draw), _ptr(draw_counter),
                                  _lib.ACTOR_DETERMINISTIC if deterministic else 0, _ptr(actions), _ptr(logp),
                                  _ptr(ent), _ptr(lout), _ptr(self.status), _stream(dev))
        _lib.check(lib, rc, None, "gsm_actor_sample")
        return (actions, logp) + ((ent,) if entropy else ()) + ((lout,) if logits else ())

    def evaluate(self, x, actions):
        """``(logp [B, N], entropy [B, N])`` of stored ``actions`` [B, N]
        under the current parameters. On the GPU inside the kernels' shape
        limits: one HIP launch (``gsm_actor_eval``) when no gradient is wanted;
        with ``kernel_backward`` and a parameter or ``x`` that wants one, the
        kernel forward and the HIP backward (``gsm_actor_eval_bwd``:
        gradients for the parameters and ``x``, no double backward). The
        differentiable torch formulation otherwise."""
        if x.dim() != 3 or x.shape[2] != self.in_features or actions.shape != x.shape[:2]:
            raise ValueError("x: [B, N, in_features]; actions: [B, N]")
        needs = torch.is_grad_enabled() and (x.requires_grad or any(p.requires_grad for p in self.parameters()))
        if self._kernel_shapes(x) and actions.device == x.device and (self.kernel_backward or not needs):
            acts = actions.to(torch.int32).contiguous()
            self.status = torch.zeros(1, dtype=torch.int32, device=x.device)
            w1, b1, w2, b2 = self._weights()
            if needs:
                return _ActorEvalFn.apply(x, w1, b1, w2, b2, acts, self.status)
            with torch.no_grad():
                return _actor_eval(x, w1, b1, w2, b2, acts, self.status)[:2]
        logp_all, ent = actor_dist_ref(self.logits(x))
        return logp_all.gather(-1, actions.to(torch.int64)[..., None])[..., 0], ent



# ---------------------------------------------------------------------------
# The critic head: a centralised value readout. Every agent's value depends on
# its own features and on the mean of its env's features; two heads give the
# reward critic and the Lagrangian cost critic that
# GraphRolloutBuffer.compute_returns(values, which="reward" | "cost") takes.

CRITIC_HIDDEN_SIZES = (16, 32, 64)
CRITIC_MAX_IN_FEATURES, CRITIC_MAX_OUT, CRITIC_MAX_AGENTS = 64, 2, 128


def _critic_mask(x, n_valid):
    """bool [B, N]: agent i of env b is valid (i < n_valid[b], clamped to [0, N]); None: all are."""
    if n_valid is None:
        return None
    N = x.shape[1]
    n = n_valid.to(device=x.device, dtype=torch.int64).clamp(0, N)
    return torch.arange(N, device=x.device)[None, :] < n[:, None]


def _critic_pool(x, mask):
    """``(x with padded rows zeroed, pool [B, F])``: the mean over an env's valid agents, 0 for none."""
    if mask is None:
        return x, x.sum(1) / x.shape[1]
    xm = torch.where(mask[..., None], x, torch.zeros((), dtype=x.dtype, device=x.device))
    n = mask.sum(1)
    return xm, xm.sum(1) / n.clamp(min=1).to(x.dtype)[:, None]


def critic_values_ref(x, w1, b1, w2, b2, n_valid=None, denorm=None):
    """The values of ``gsm_critic_eval`` in plain torch (any device and dtype,
    differentiable): ``x`` [B, N, F], ``w1`` [hidden, 2F] over ``[pool | x]``,
    ``w2`` [n_out, hidden]; returns ``[n_out, B, N]``::

        pool_b = mean over the valid agents of env b (0 for none)
        h = relu(W1[:, :F] pool_b + W1[:, F:] x_r + b1);  v = W2 h + b2
        out = v * std + mean with denorm [n_out, 2] = (mean, std), else v

    Rows ``i >= n_valid[b]`` are padding: not read (they may hold NaN), 0.0 in
    every head."""
    F = x.shape[2]
    mask = _critic_mask(x, n_valid)
    xm, pool = _critic_pool(x, mask)
    c = pool @ w1[:, :F].t() + b1
    h = torch.relu(c[:, None, :] + xm @ w1[:, F:].t())
    v = h @ w2.t() + b2
    if denorm is not None:
        denorm = denorm.to(v.dtype)
        v = v * denorm[:, 1] + denorm[:, 0]
    if mask is not None:
        v = torch.where(mask[..., None], v, torch.zeros((), dtype=v.dtype, device=v.device))
    return v.permute(2, 0, 1).contiguous()


def critic_bwd_ref(g, x, w1, b1, w2, b2, n_valid=None):
    """The gradients of the raw values written out (the formulas of
    ``gsm_critic_eval_bwd``): ``g`` [n_out, B, N], ``x`` [B, N, F]. With
    ``dv_r = g[:, r]`` (0 on padded rows)::

        db2 = sum_r dv;  dW2 = sum_r dv (x) h_r;  dh_r = W2^T dv_r where h_r > 0
        db1 = sum_r dh;  dW1[:, F:] = sum_r dh_r (x) x_r
        s_b = sum_{i valid} dh_{b,i};  dW1[:, :F] = sum_b s_b (x) pool_b
        dpool_b = W1[:, :F]^T s_b;  dx_r = W1[:, F:]^T dh_r + dpool_b / n_b

    Returns ``(dw1, db1, dw2, db2, dx [B, N, F])``; ``dx`` is 0 on padded rows."""
    B, N, F = x.shape
    mask = _critic_mask(x, n_valid)
    xm, pool = _critic_pool(x, mask)
    h = torch.relu((pool @ w1[:, :F].t() + b1)[:, None, :] + xm @ w1[:, F:].t())
    dv = g.permute(1, 2, 0)
    if mask is not None:
        m = mask[..., None].to(x.dtype)
        dv, h = dv * m, h * m
        n = mask.sum(1).clamp(min=1).to(x.dtype)
    else:
        n = torch.full((B,), float(N), dtype=x.dtype, device=x.device)
    db2 = dv.sum((0, 1))
    dw2 = torch.einsum("bno,bnh->oh", dv, h)
    dh = (dv @ w2) * (h > 0).to(x.dtype)
    db1 = dh.sum((0, 1))
    s = dh.sum(1)
    dw1 = torch.cat([s.t() @ pool, torch.einsum("bnh,bnf->hf", dh, xm)], 1)
    dx = dh @ w1[:, F:] + ((s @ w1[:, :F]) / n[:, None])[:, None, :]
    if mask is not None:
        dx = dx * m
    return dw1, db1, dw2, db2, dx


def _critic_eval(x, w1, b1, w2, b2, n_valid, denorm, status):
    """One gsm_critic_eval launch. Returns ``(values [n_out, B, N], x as read, row stride)``."""
    B, N, F = x.shape
    xk, stride = _rows(x)
    lib = _lib.load()
    hidden, nO = int(w1.shape[0]), int(w2.shape[0])
    values = torch.empty(nO, B, N, dtype=torch.float32, device=x.device)
    rc = lib.gsm_critic_eval(_ptr(xk) if B else None, stride, _ptr(n_valid), _ptr(w1), _ptr(b1), _ptr(w2), _ptr(b2),
                             _ptr(denorm), int(B), int(N), int(F), hidden, nO, _ptr(values), _ptr(status),
                             _stream(x.device))
    _lib.check(lib, rc, None, "gsm_critic_eval")
    return values, xk, stride


def critic_work_floats(in_features: int, hidden: int, n_out: int) -> int:
    """Floats of workspace ``gsm_critic_eval_bwd`` wants (``gsm_critic_backward_work_floats``)."""
    return _lib.work_floats("gsm_critic_backward_work_floats", int(in_features), int(hidden), int(n_out))


class _CriticEvalFn(torch.autograd.Function):
    """gsm_critic_eval (raw values) / gsm_critic_eval_bwd (include/gsm.h)."""

    @staticmethod
    def forward(ctx, x, w1, b1, w2, b2, n_valid, status):
        values, xk, stride = _critic_eval(x, w1, b1, w2, b2, n_valid, None, status)
        ctx.save_for_backward(xk, w1, b1, w2, b2, n_valid, status)
        ctx.stride = stride
        return values

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        xk, w1, b1, w2, b2, n_valid, status = ctx.saved_tensors
        B, N, F = xk.shape
        dev = xk.device
        lib = _lib.load()
        hidden, nO = int(w1.shape[0]), int(w2.shape[0])
        g = g.to(torch.float32).contiguous()
        work = torch.empty(critic_work_floats(F, hidden, nO), dtype=torch.float32, device=dev)
        dw1, db1, dw2, db2 = (torch.empty_like(t) for t in (w1, b1, w2, b2))
        dx = torch.empty(B, N, F, dtype=torch.float32, device=dev) if ctx.needs_input_grad[0] else None
        rc = lib.gsm_critic_eval_bwd(_ptr(g), _ptr(xk) if B else None, ctx.stride, _ptr(n_valid), _ptr(w1), _ptr(b1),
                                     _ptr(w2), _ptr(b2), int(B), int(N), int(F), hidden, nO, _ptr(work), _ptr(dw1),
                                     _ptr(db1), _ptr(dw2), _ptr(db2), _ptr(dx) if B else None, _ptr(status),
                                     _stream(dev))
        _lib.check(lib, rc, None, "gsm_critic_eval_bwd")
        return dx, dw1, db1, dw2, db2, None, None


class CriticHead(torch.nn.Module):
    """A centralised critic: ``lin2(relu(lin1([pool_b | x_r])))`` with
    ``pool_b`` the mean of env b's agent features, ``n_out`` values a row (two:
    the reward critic and the Lagrangian cost critic). ``forward`` takes the
    ``[B, N, in_features]`` features of ``TransformerConv.forward_env`` (B any
    number of envs: all ``(T+1) * B`` stored steps of a buffer in one call)
    and returns ``[n_out, B, N]``, so ``values[0]`` and ``values[1]`` are the
    contiguous tensors ``GraphRolloutBuffer.compute_returns`` takes.

    On the GPU, with ``use_kernel``, a gradient-free ``forward`` is one HIP
    launch (``gsm_critic_eval``); with ``kernel_backward`` the training path
    runs on the kernels too (``gsm_critic_eval_bwd``: gradients for the
    parameters and ``x``, no double backward; the denormalisation, which the
    kernels never differentiate, is then applied in torch). Otherwise, outside
    the kernels' shape limits (fp32, ``in_features`` a multiple of 4 in
    [4, 64], ``hidden`` 16, 32 or 64, 1 or 2 heads, at most 128 agents) or off
    the GPU it runs ``critic_values_ref``. After a kernel call ``status`` holds
    the launch's status word (device int32 [1], ``_lib.CRITIC_*`` bits); it is
    not read here, so every call can be captured into a graph."""

    def __init__(self, in_features: int, hidden: int = 64, n_out: int = 2, use_kernel: bool = True,
                 kernel_backward: bool = False):
        super().__init__()
        self.in_features, self.hidden, self.n_out = int(in_features), int(hidden), int(n_out)
        self.lin1 = torch.nn.Linear(2 * in_features, hidden)
        self.lin2 = torch.nn.Linear(hidden, n_out)
        self.use_kernel = use_kernel
        self.kernel_backward = kernel_backward
        self.status = None

    def _weights(self):
        return self.lin1.weight, self.lin1.bias, self.lin2.weight, self.lin2.bias

    def _kernel_shapes(self, x, n_valid, denorm):
        if not (self.use_kernel and x.is_cuda and x.dtype == torch.float32 and x.dim() == 3):
            return False
        if any(p.dtype != torch.float32 or not p.is_contiguous() or p.device != x.device for p in self.parameters()):
            return False
        if n_valid is not None and n_valid.device != x.device:
            return False
        if denorm is not None and (denorm.device != x.device or denorm.dtype != torch.float32 or
                                   not denorm.is_contiguous()):
            return False
        F = self.in_features
        return (x.shape[2] == F and 4 <= F <= CRITIC_MAX_IN_FEATURES and F % 4 == 0 and
                self.hidden in CRITIC_HIDDEN_SIZES and 1 <= self.n_out <= CRITIC_MAX_OUT and
                1 <= x.shape[1] <= CRITIC_MAX_AGENTS and x.shape[0] * x.shape[1] < 2 ** 31)

    def forward(self, x, n_valid=None, denorm=None):
        """``[n_out, B, N]`` values of ``x`` [B, N, in_features]. ``n_valid``
        [B]: the envs' own agent counts in a ragged batch (rows past them are
        padding: never read, 0.0 out, no part in the pool). ``denorm``
        [n_out, 2] = (mean, std) per head (``PopArt.stats()``): the values are
        denormalised, ``v * std + mean``; the kernel reads it when it runs."""
        if x.dim() != 3 or x.shape[2] != self.in_features:
            raise ValueError("x: [B, N, in_features]")
        if n_valid is not None and n_valid.shape != x.shape[:1]:
            raise ValueError("n_valid: [B]")
        if denorm is not None and denorm.shape != (self.n_out, 2):
            raise ValueError("denorm: [n_out, 2]")
        needs = torch.is_grad_enabled() and (x.requires_grad or any(p.requires_grad for p in self.parameters()))
        if self._kernel_shapes(x, n_valid, denorm) and (self.kernel_backward or not needs):
            nv = n_valid.to(torch.int32).contiguous() if n_valid is not None else None
            self.status = torch.zeros(1, dtype=torch.int32, device=x.device)
            if needs:
                v = _CriticEvalFn.apply(x, *self._weights(), nv, self.status)
                if denorm is not None:
                    v = v * denorm[:, 1, None, None] + denorm[:, 0, None, None]
                    if nv is not None:
                        v = torch.where(_critic_mask(x, nv)[None], v, torch.zeros((), dtype=v.dtype, device=v.device))
                return v
            with torch.no_grad():
                return _critic_eval(x, *self._weights(), nv, denorm, self.status)[0]
        return critic_values_ref(x, *self._weights(), n_valid, denorm)


class PopArt(torch.nn.Module):
    """Running value normalisation with output preservation, after the PopArt
    of the public MAPPO code base (``onpolicy/utils/popart.py``; van Hasselt
    et al. 2016). A restatement of that lineage: the reference project lists
    ``gsmarl/utils/popart.py`` but ships no such file. One set of statistics
    per head: exponentially weighted first and second moments with a debiasing
    term, ``std = sqrt(max(E[x^2] - E[x]^2, 1e-2))`` of the debiased moments.
    The statistics update is one reduction a PPO epoch and stays in torch;
    ``stats()`` is what ``CriticHead.forward(denorm=...)`` hands the kernel."""

    def __init__(self, n_out: int = 2, beta: float = 0.99999, eps: float = 1e-5):
        super().__init__()
        self.n_out, self.beta, self.eps = int(n_out), float(beta), float(eps)
        self.register_buffer("mean", torch.zeros(n_out))
        self.register_buffer("mean_sq", torch.zeros(n_out))
        self.register_buffer("debias", torch.zeros(n_out))

    def _moments(self):
        d = self.debias.clamp(min=self.eps)
        mean, mean_sq = self.mean / d, self.mean_sq / d
        return mean, (mean_sq - mean * mean).clamp(min=1e-2).sqrt()

    def stats(self):
        """f32 ``[n_out, 2]`` = (mean, std) per head."""
        mean, std = self._moments()
        return torch.stack([mean, std], 1).to(torch.float32).contiguous()

    def _per_head(self, t, like):
        return t.to(like.dtype).view((self.n_out,) + (1,) * (like.dim() - 1))

    def normalize(self, returns):
        """``(returns - mean) / std``, ``returns`` [n_out, ...]."""
        mean, std = self._moments()
        return (returns - self._per_head(mean, returns)) / self._per_head(std, returns)

    @torch.no_grad()
    def update(self, returns, head: Optional[CriticHead] = None):
        """Move the statistics towards ``returns`` [n_out, ...] and, with
        ``head``, rescale ``head.lin2`` so that its denormalised outputs are
        what they were: ``W <- W s_old / s_new``, ``b <- (s_old b + m_old -
        m_new) / s_new``."""
        old_mean, old_std = self._moments()
        flat = returns.reshape(self.n_out, -1).to(self.mean.dtype)
        w = 1.0 - self.beta
        self.mean.mul_(self.beta).add_(flat.mean(1) * w)
        self.mean_sq.mul_(self.beta).add_((flat * flat).mean(1) * w)
        self.debias.mul_(self.beta).add_(w)
        new_mean, new_std = self._moments()
        if head is not None:
            W, b = head.lin2.weight, head.lin2.bias
            W.mul_((old_std / new_std).to(W.dtype)[:, None])
            b.copy_(((old_std * b + old_mean - new_mean) / new_std).to(b.dtype))
