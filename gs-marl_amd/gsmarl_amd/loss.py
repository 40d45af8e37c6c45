"""The clipped PPO / Lagrangian loss the actor and critic heads end in.

``PPOLagrangianLoss`` takes what ``ActorHead.evaluate`` and ``CriticHead``
return (``logp``, ``entropy``, the twin values) with what the rollout stored
(``logp_old``, advantages, old values, returns) and gives the loss. On the GPU
in fp32 it is one ABI call (``gsm_ppo_loss`` in include/gsm.h: two launches)
that also writes the gradients with respect to ``logp``, ``entropy`` and the
values, so its backward is a multiplication by ``grad_output`` and the two
heads' HIP backwards follow directly. ``LagrangeMultiplier`` holds the cost
multiplier on the device, where the kernel reads it when it runs.

``ppo_loss_ref`` is the definition in plain torch (any device and dtype,
differentiable), the kernel's reference and the fallback;
``ppo_loss_grads_ref`` writes its gradients out.
"""
from __future__ import annotations


import torch

from . import _lib

_ptr, _stream = _lib.ptr, _lib.stream

N_STATS = 8     # loss, policy term, entropy, value loss of head 0 and 1, approximate KL, clip fraction, W


def _zero(t):
    return torch.zeros((), dtype=t.dtype, device=t.device)


def ppo_loss_weights(logp, weight=None, n_valid=None):
    """``w`` [B, N] in ``logp``'s dtype: ``weight`` (1 when None; a negative or
    non-finite weight counts as 0) times ``[i < n_valid[b]]`` (``n_valid``
    clamped to [0, N]). A padded row's weight is not looked at."""
    B, N = logp.shape
    w = torch.ones(B, N, dtype=logp.dtype, device=logp.device) if weight is None else weight.to(logp.dtype)
    w = torch.where((w >= 0) & torch.isfinite(w), w, _zero(w))
    if n_valid is not None:
        n = n_valid.to(device=logp.device, dtype=torch.int64).clamp(0, N)
        w = torch.where(torch.arange(N, device=logp.device)[None, :] < n[:, None], w, _zero(w))
    return w


def _lam(multiplier, like):
    if multiplier is None:
        return None
    if torch.is_tensor(multiplier):
        return multiplier.to(device=like.device, dtype=like.dtype).reshape(-1)[0]
    return torch.tensor(float(multiplier), dtype=like.dtype, device=like.device)


def _rows(logp, ent, values, logp_old, adv, v_old, ret, w, lam, clip, value_clip):
    """The per-row quantities of the definition on inputs whose rows of weight
    0 are replaced by zeros (so a NaN there reaches neither a value nor a
    gradient)."""
    on = w != 0
    z = _zero(logp)
    logp, ent, logp_old = (torch.where(on, t, z) for t in (logp, ent, logp_old))
    values, adv, v_old, ret = (torch.where(on[None], t, z) for t in (values, adv, v_old, ret))
    A = adv[0] - lam * adv[1] if values.shape[0] == 2 else adv[0]
    ratio = torch.exp(logp - logp_old)
    lo, hi = 1.0 - clip, 1.0 + clip
    s1, s2 = ratio * A, ratio.clamp(lo, hi) * A
    pol = -torch.min(s1, s2)
    d = values - v_old
    vclip = v_old + d.clamp(-value_clip, value_clip)
    q1, q2 = (values - ret) ** 2, (vclip - ret) ** 2
    val = torch.max(q1, q2)
    return dict(logp=logp, ent=ent, logp_old=logp_old, values=values, ret=ret, A=A, ratio=ratio, lo=lo, hi=hi,
                s1=s1, s2=s2, pol=pol, d=d, q1=q1, q2=q2, val=val)


def ppo_loss_ref(logp, ent, values, logp_old, adv, v_old, ret, weight=None, n_valid=None, multiplier=None,
                 clip: float = 0.2, value_clip: float = 0.2, ent_coef: float = 0.01, value_coef: float = 1.0,
                 keep=None):
    """The loss of ``gsm_ppo_loss`` in plain torch (any device and dtype,
    differentiable). ``logp``, ``ent``, ``logp_old`` [B, N]; ``values``,
    ``adv``, ``v_old``, ``ret`` [n_out, B, N], n_out 1 or 2 (reward, cost)::

        w_r   = weight[r] (or 1) * [i < n_valid[b]];  W = sum_r w_r
        A     = adv[0] - lam * adv[1]                     (n_out == 1: adv[0])
        ratio = exp(logp - logp_old)
        pol   = -min(ratio * A, clamp(ratio, 1 - clip, 1 + clip) * A)
        vclip = v_old + clamp(v - v_old, -value_clip, value_clip)
        val_o = max((v_o - ret_o)^2, (vclip_o - ret_o)^2)
        loss  = (1/W) sum_r w_r (pol_r - ent_coef ent_r + value_coef sum_o val_{o,r})

    Rows with ``w_r == 0`` are not read (they may hold NaN) and get gradient
    0; ``W == 0`` gives zeros. Returns ``(loss, stats [8])``: the weighted
    means of the loss, ``pol``, ``ent``, ``val_0``, ``val_1`` (0 for an absent
    head), ``logp_old - logp`` and ``[ratio outside the clip range]``, then
    ``W``. ``keep`` (a dict) receives ``w``, ``W``, ``ratio``, ``A`` and the
    per-row terms ``pol_rows`` [B, N] (with the entropy bonus) and ``val_rows``
    [n_out, B, N], whose sum the loss is."""
    n_out = values.shape[0]
    if n_out not in (1, 2):
        raise ValueError("values: [n_out, B, N] with n_out 1 or 2")
    if n_out == 2 and multiplier is None:
        raise ValueError("two heads need a multiplier")
    w = ppo_loss_weights(logp, weight, n_valid)
    q = _rows(logp, ent, values, logp_old, adv, v_old, ret, w, _lam(multiplier, logp), clip, value_clip)
    W = w.sum()
    inv = torch.where(W > 0, 1.0 / torch.where(W > 0, W, torch.ones_like(W)), _zero(W))
    pol_rows = w * (q["pol"] - ent_coef * q["ent"]) * inv
    val_rows = w[None] * q["val"] * (value_coef * inv)
    loss = pol_rows.sum() + val_rows.sum()
    outside = ((q["ratio"] < q["lo"]) | (q["ratio"] > q["hi"])).to(w.dtype)
    val_mean = [(w * q["val"][o]).sum() * inv for o in range(n_out)] + [_zero(W)] * (2 - n_out)
    with torch.no_grad():
        stats = torch.stack([loss.detach(), (w * q["pol"]).sum() * inv, (w * q["ent"]).sum() * inv, val_mean[0],
                             val_mean[1], (w * (q["logp_old"] - q["logp"])).sum() * inv, (w * outside).sum() * inv,
                             W])
    if keep is not None:
        total = q["pol"] - ent_coef * q["ent"] + value_coef * q["val"].sum(0)
        terms = [total, q["pol"], q["ent"], q["val"][0], q["val"][1] if n_out == 2 else torch.zeros_like(w),
                 q["logp_old"] - q["logp"], outside]
        keep.update(w=w, W=W, ratio=q["ratio"], A=q["A"], pol_rows=pol_rows, val_rows=val_rows, v=q["values"],
                    terms=torch.stack(terms).detach())
    return loss, stats


def ppo_loss_grads_ref(logp, ent, values, logp_old, adv, v_old, ret, weight=None, n_valid=None, multiplier=None,
                       clip: float = 0.2, value_clip: float = 0.2, ent_coef: float = 0.01, value_coef: float = 1.0):
    """The gradients of ``ppo_loss_ref`` written out (the formulas of
    ``gsm_ppo_loss``). With ``c = w_r / W`` (0 when ``W == 0``)::

        g_logp = c (-A ratio)  if 1 - clip <= ratio <= 1 + clip
                               or ratio A < clamp(ratio, 1 - clip, 1 + clip) A;  else 0
        g_ent  = -c ent_coef
        g_v_o  = c value_coef 2 (v - ret)  if |v - v_old| <= value_clip
                               or (v - ret)^2 > (vclip - ret)^2;  else 0

    Returns ``(g_logp [B, N], g_ent [B, N], g_values [n_out, B, N])``."""
    w = ppo_loss_weights(logp, weight, n_valid)
    q = _rows(logp, ent, values, logp_old, adv, v_old, ret, w, _lam(multiplier, logp), clip, value_clip)
    W = w.sum()
    c = w * torch.where(W > 0, 1.0 / torch.where(W > 0, W, torch.ones_like(W)), _zero(W))
    inside = (q["ratio"] >= q["lo"]) & (q["ratio"] <= q["hi"])
    g_logp = c * torch.where(inside | (q["s1"] < q["s2"]), -q["s1"], _zero(w))
    g_ent = -c * ent_coef
    live = (q["d"].abs() <= value_clip) | (q["q1"] > q["q2"])
    g_values = c[None] * torch.where(live, value_coef * 2.0 * (q["values"] - q["ret"]), _zero(w))
    return g_logp, g_ent, g_values


def ppo_loss_work_floats(n_rows: int) -> int:
    """Floats of workspace ``gsm_ppo_loss`` wants (``gsm_ppo_loss_work_floats``)."""
    return _lib.work_floats("gsm_ppo_loss_work_floats", int(n_rows))


def _ppo_loss_call(logp, ent, values, logp_old, adv, v_old, ret, weight, n_valid, lam, status, coef, grads):
    """One gsm_ppo_loss call. Returns ``(loss [1], stats [8], g_logp, g_ent,
    g_values)``; the gradients are None without ``grads``."""
    B, N = logp.shape
    n_out, dev = int(values.shape[0]), logp.device
    lib = _lib.load()
    f32 = dict(dtype=torch.float32, device=dev)
    work = torch.empty(ppo_loss_work_floats(B * N), **f32)
    loss, stats = torch.empty(1, **f32), torch.empty(N_STATS, **f32)
    g_logp = torch.empty(B, N, **f32) if grads else None
    g_ent = torch.empty(B, N, **f32) if grads else None
    g_values = torch.empty(n_out, B, N, **f32) if grads else None
    clip, value_clip, ent_coef, value_coef = coef
    rc = lib.gsm_ppo_loss(_ptr(logp), _ptr(ent), _ptr(values), _ptr(logp_old), _ptr(adv), _ptr(v_old), _ptr(ret),
                          _ptr(weight), _ptr(n_valid), int(B), int(N), n_out, _ptr(lam), clip, value_clip, ent_coef,
                          value_coef, _ptr(work), _ptr(loss), _ptr(stats), _ptr(g_logp), _ptr(g_ent),
                          _ptr(g_values), _ptr(status), _stream(dev))
    _lib.check(lib, rc, None, "gsm_ppo_loss")
    return loss, stats, g_logp, g_ent, g_values


class _PPOLossFn(torch.autograd.Function):
    """gsm_ppo_loss (include/gsm.h): the forward writes the row gradients, the
    backward multiplies them by ``grad_output``."""

    @staticmethod
    def forward(ctx, logp, ent, values, logp_old, adv, v_old, ret, weight, n_valid, lam, status, coef):
        loss, stats, g_logp, g_ent, g_values = _ppo_loss_call(logp, ent, values, logp_old, adv, v_old, ret, weight,
                                                              n_valid, lam, status, coef, True)
        ctx.save_for_backward(g_logp, g_ent, g_values)
        ctx.mark_non_differentiable(stats)
        return loss.view(()), stats

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g, _g_stats):
        g_logp, g_ent, g_values = ctx.saved_tensors
        need = ctx.needs_input_grad
        return (g * g_logp if need[0] else None, g * g_ent if need[1] else None, g * g_values if need[2] else None,
                None, None, None, None, None, None, None, None, None)


class PPOLagrangianLoss(torch.nn.Module):
    """The clipped PPO / Lagrangian loss of ``ppo_loss_ref``. ``forward``
    takes ``logp``, ``ent``, ``logp_old`` [B, N] and ``values``, ``adv``,
    ``v_old``, ``ret`` [n_out, B, N] (n_out 1 or 2, as ``CriticHead`` returns
    them), optionally ``weight`` [B, N] and ``n_valid`` [B], and the Lagrange
    ``multiplier`` of the cost advantage (a float, or a device tensor such as
    ``LagrangeMultiplier.lam``, which the kernel reads when it runs; needed
    with two heads). It returns the 0-dim loss.

    On the GPU in fp32, with ``use_kernel``, the call is one ``gsm_ppo_loss``
    (two launches) inside an ``autograd.Function`` whose backward is
    ``grad_output`` times the row gradients the forward wrote: no kernel of
    its own, no double backward. Any other device or dtype runs
    ``ppo_loss_ref``. Non-contiguous inputs are made contiguous. After a call
    ``stats`` holds the f32 [8] statistics (the weighted means of the loss,
    the policy term, the entropy, the value loss per head, the approximate KL
    and the clip fraction, then W) and ``status`` the status word (device
    int32 [1], ``_lib.LOSS_*`` bits; None after a fallback call); neither is
    read here, so every call can be captured into a graph."""

    def __init__(self, clip: float = 0.2, value_clip: float = 0.2, entropy_coef: float = 0.01,
                 value_coef: float = 1.0, use_kernel: bool = True):
        super().__init__()
        self.clip, self.value_clip = float(clip), float(value_clip)
        self.entropy_coef, self.value_coef = float(entropy_coef), float(value_coef)
        self.use_kernel = use_kernel
        self.stats = None
        self.status = None

    def _kernel_inputs(self, tensors, weight, n_valid, multiplier):
        logp = tensors[0]
        if not (self.use_kernel and logp.is_cuda and logp.shape[0] * logp.shape[1] < 2 ** 31 and logp.shape[1] >= 1):
            return False
        if any(t.dtype != torch.float32 or t.device != logp.device for t in tensors):
            return False
        if weight is not None and (weight.dtype != torch.float32 or weight.device != logp.device):
            return False
        if n_valid is not None and n_valid.device != logp.device:
            return False
        return not torch.is_tensor(multiplier) or (multiplier.device == logp.device and
                                                   multiplier.dtype == torch.float32)

    def forward(self, logp, ent, values, logp_old, adv, v_old, ret, weight=None, n_valid=None, multiplier=None):
        if logp.dim() != 2 or ent.shape != logp.shape or logp_old.shape != logp.shape:
            raise ValueError("logp, ent, logp_old: [B, N]")
        if values.dim() != 3 or values.shape[0] not in (1, 2) or values.shape[1:] != logp.shape or any(
                t.shape != values.shape for t in (adv, v_old, ret)):
            raise ValueError("values, adv, v_old, ret: [n_out, B, N] with n_out 1 or 2")
        if weight is not None and weight.shape != logp.shape:
            raise ValueError("weight: [B, N]")
        if n_valid is not None and n_valid.shape != logp.shape[:1]:
            raise ValueError("n_valid: [B]")
        if values.shape[0] == 2 and multiplier is None:
            raise ValueError("two heads need a multiplier")
        if torch.is_tensor(multiplier) and multiplier.numel() != 1:
            raise ValueError("multiplier: a float or a tensor of one element")
        tensors = (logp, ent, values, logp_old, adv, v_old, ret)
        coef = (self.clip, self.value_clip, self.entropy_coef, self.value_coef)
        if not self._kernel_inputs(tensors, weight, n_valid, multiplier):
            loss, self.stats = ppo_loss_ref(*tensors, weight, n_valid, multiplier, *coef)
            self.status = None
            return loss
        dev = logp.device
        tensors = tuple(t.contiguous() for t in tensors)
        weight = weight.contiguous() if weight is not None else None
        nv = n_valid.to(torch.int32).contiguous() if n_valid is not None else None
        lam = None
        if multiplier is not None:
            lam = (multiplier.reshape(1) if torch.is_tensor(multiplier) else
                   torch.full((1,), float(multiplier), dtype=torch.float32, device=dev))
        self.status = torch.zeros(1, dtype=torch.int32, device=dev)
        if torch.is_grad_enabled() and any(t.requires_grad for t in tensors[:3]):
            loss, self.stats = _PPOLossFn.apply(*tensors, weight, nv, lam, self.status, coef)
            return loss
        with torch.no_grad():
            loss, self.stats = _ppo_loss_call(*tensors, weight, nv, lam, self.status, coef, False)[:2]
        return loss.view(())


class LagrangeMultiplier(torch.nn.Module):
    """The Lagrange multiplier of the cost constraint as a device f32 [1]
    buffer ``lam``, which ``PPOLagrangianLoss`` hands the kernel as it is (a
    captured graph sees every update). ``update(mean_cost)`` does ``lam <-
    max(0, lam + lr * (mean_cost - cost_limit))`` in place: one small torch
    op a PPO epoch, like ``PopArt.update``."""

    def __init__(self, init: float = 0.0, *, lr: float, cost_limit: float):
        super().__init__()
        self.lr, self.cost_limit = float(lr), float(cost_limit)
        self.register_buffer("lam", torch.full((1,), float(init), dtype=torch.float32))

    @torch.no_grad()
    def update(self, mean_cost):
        """``mean_cost``: a float or a tensor of one element (the mean episode cost)."""
        if torch.is_tensor(mean_cost):
            mean_cost = mean_cost.detach().to(self.lam).reshape(1)
        self.lam.add_((mean_cost - self.cost_limit) * self.lr).clamp_(min=0.0)
        return self.lam
