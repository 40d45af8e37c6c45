"""GNN message passing over the env graph.

The reference's actor/critic encode the graph observation with a GNN
(gsmarl/algorithms, SOURCES.txt:8; torch-geometric 2.3.1, requirements.txt:119;
the InforMARL lineage uses ``TransformerConv`` with the edge distance as a
1-d edge feature). torch-geometric is not available here, so this module
restates that layer:

* projections ``q/k/v/skip = x @ W + b`` and the edge projection ``w_e`` are
  dense GEMMs (torch.matmul -> hipBLASLt / MFMA);
* the graph part — per-edge scores, segmented softmax over each target's
  neighbours, weighted aggregation — is the HIP kernel behind
  ``gsm_attn_aggregate`` (gsm_gnn.hip) on the rollout / inference path, and the
  equivalent torch formulation (``attn_aggregate_ref``) where gradients are
  needed (training) or as the numerics reference;
* ``attn_aggregate_autograd`` is the kernel with gradients (the HIP backward
  ``gsm_attn_aggregate_bwd`` over the CSR rows and the transposed graph of
  ``csr_transpose``; ``attn_aggregate_bwd_ref`` is its torch restatement), which
  ``TransformerConv(kernel_backward=True)`` trains on;
* ``csr_transpose_symmetric`` is that transposed graph without the sort, for
  symmetric graphs with ascending rows and columns such as the env's: the
  formulation ``GraphRolloutBuffer.graph_batch_csr``'s gather kernel
  (``gsm_graph_batch_gather``) is written against.

* ``env_conv`` is the whole first layer (``in_channels = 7``: the four
  projections and the attention) as one HIP launch straight from the env-form
  graph of ``GpuBatchEnv.step`` / ``GraphRolloutBuffer.slot`` (``gsm_env_conv``):
  no ``env_csr``, no [n, HC] tensors; ``TransformerConv.forward_env`` takes it on
  the inference path and ``env_conv_ref`` (plain torch, differentiable)
  elsewhere;
* ``env_conv_autograd`` is that layer with gradients for its weights
  (``gsm_env_conv_fwd`` / ``gsm_env_conv_bwd``: the backward recomputes the
  projections on chip too, so what leaves it is ``dw`` and ``dw_e``, a few KB;
  ``env_conv_bwd_ref`` is its torch restatement), which
  ``TransformerConv(kernel_backward=True).forward_env`` trains on.

Graph format: CSR over targets (``row_ptr`` [n+1] int64, ``col`` int32
sources, ``edge_w`` per CSR entry). The env graphs are symmetric (every radius
edge and agent<->goal edge is emitted both ways), so the row-major COO the
env emits *is* that CSR: ``env_csr`` only adds per-node row offsets.
"""
from __future__ import annotations

import math
from typing import Optional

import torch

from . import _lib


def env_csr(edge_index: torch.Tensor, n_nodes: int) -> torch.Tensor:
    """Per-node row offsets [n_nodes+1] (int64) of a row-major edge list whose
    sources are sorted (the env's COO output)."""
    cnt = torch.bincount(edge_index[0].to(torch.int64), minlength=n_nodes)
    ptr = torch.zeros(n_nodes + 1, dtype=torch.int64, device=edge_index.device)
    torch.cumsum(cnt, 0, out=ptr[1:])
    return ptr


def attn_aggregate_ref(q, k, v, row_ptr, col, edge_w=None, w_e=None, skip=None, heads=1, scale=None):
    """Torch (differentiable) formulation of gsm_attn_aggregate."""
    n, HC = q.shape
    Cc = HC // heads
    scale = 1.0 / math.sqrt(Cc) if scale is None else scale
    deg = row_ptr[1:] - row_ptr[:-1]
    tgt = torch.repeat_interleave(torch.arange(n, device=q.device), deg, output_size=col.numel())
    src = col.to(torch.int64)
    e = 0.0
    if edge_w is not None:
        e = edge_w[:, None] * w_e[None, :]
    kj = (k[src] + e).view(-1, heads, Cc)
    vj = (v[src] + e).view(-1, heads, Cc)
    s = (q[tgt].view(-1, heads, Cc) * kj).sum(-1) * scale                     # [nE, H]
    smax = torch.full((n, heads), -math.inf, device=q.device, dtype=q.dtype)
    smax = smax.scatter_reduce(0, tgt[:, None].expand(-1, heads), s, reduce="amax", include_self=True)
    a = torch.exp(s - smax[tgt])
    den = torch.zeros(n, heads, device=q.device, dtype=q.dtype).index_add(0, tgt, a)
    alpha = a / den[tgt]
    out = torch.zeros(n, heads, Cc, device=q.device, dtype=q.dtype).index_add(0, tgt, alpha[..., None] * vj)
    out = out.view(n, HC)
    if skip is not None:
        out = out + skip
    return out


def attn_aggregate_bwd_ref(grad_out, q, k, v, row_ptr, col, edge_w=None, w_e=None, skip=None, heads=1,
                           scale=None):
    """The gradients of ``attn_aggregate_ref`` written out (plain torch, fp32 or
    fp64, any device): the restatement the backward kernels are written
    against. With ``m_ij = v_j + e_ij`` and ``g_i = grad_out[i]``::

        dskip_i    = g_i
        D_i[h]     = sum_j a_ij <g_i[h], m_ij[h]>      (= <g_i[h], out_i[h] - skip_i[h]>)
        ds_ij[h]   = a_ij[h] * (<g_i[h], m_ij[h]> - D_i[h])
        dq_i[h]    = scale * sum_j ds_ij[h] * (k_j[h] + e_ij[h])
        dk_j[h]    = scale * sum_{i: j in row i} ds_ij[h] * q_i[h]
        dv_j[h]    =         sum_{i: j in row i} a_ij[h]  * g_i[h]
        de_ij[c]   = scale * ds_ij[h(c)] * q_i[c] + a_ij[h(c)] * g_i[c]
        dw_e[c]    = sum_ij edge_w_ij * de_ij[c]
        dedge_w_ij = sum_c de_ij[c] * w_e[c]

    Returns ``(dq, dk, dv, dedge_w, dw_e, dskip)``, None where the input is None."""
    n, HC = q.shape
    Cc = HC // heads
    scale = 1.0 / math.sqrt(Cc) if scale is None else scale
    deg = row_ptr[1:] - row_ptr[:-1]
    tgt = torch.repeat_interleave(torch.arange(n, device=q.device), deg, output_size=col.numel())
    src = col.to(torch.int64)
    e = 0.0
    if edge_w is not None:
        e = edge_w[:, None] * w_e[None, :]
    kj = (k[src] + e).view(-1, heads, Cc)
    mj = (v[src] + e).view(-1, heads, Cc)
    qi = q[tgt].view(-1, heads, Cc)
    gi = grad_out[tgt].view(-1, heads, Cc)
    s = (qi * kj).sum(-1) * scale                                              # [nE, H]
    smax = torch.full((n, heads), -math.inf, device=q.device, dtype=q.dtype)
    smax = smax.scatter_reduce(0, tgt[:, None].expand(-1, heads), s, reduce="amax", include_self=True)
    a = torch.exp(s - smax[tgt])
    den = torch.zeros(n, heads, device=q.device, dtype=q.dtype).index_add(0, tgt, a)
    a = a / den[tgt]
    gm = (gi * mj).sum(-1)
    D = torch.zeros(n, heads, device=q.device, dtype=q.dtype).index_add(0, tgt, a * gm)
    ds = a * (gm - D[tgt])
    zero = torch.zeros(n, heads, Cc, device=q.device, dtype=q.dtype)
    dq = (scale * zero.index_add(0, tgt, ds[..., None] * kj)).view(n, HC)
    dk = (scale * zero.index_add(0, src, ds[..., None] * qi)).view(n, HC)
    dv = zero.index_add(0, src, a[..., None] * gi).view(n, HC)
    dedge_w = dw_e = None
    if edge_w is not None:
        de = (scale * ds[..., None] * qi + a[..., None] * gi).view(-1, HC)
        dw_e = (edge_w[:, None] * de).sum(0)
        dedge_w = (de * w_e[None, :]).sum(-1)
    return dq, dk, dv, dedge_w, dw_e, (grad_out if skip is not None else None)


def csr_transpose(row_ptr, col):
    """The CSR entries regrouped by source, for the sums of the backward that
    run over the rows containing a source: ``(t_ptr int64 [n+1], t_edge int32
    [nE], t_tgt int32 [nE])``: offsets per source, the entry ids of each source
    in ascending order (a stable sort) and each listed entry's target row. A
    property of the graph alone: build it once per stored graph."""
    n, nE = row_ptr.numel() - 1, col.numel()
    dev = col.device
    src = col.to(torch.int64)
    perm = torch.sort(src, stable=True)[1]
    t_ptr = torch.zeros(n + 1, dtype=torch.int64, device=dev)
    torch.cumsum(torch.bincount(src, minlength=n), 0, out=t_ptr[1:])
    tgt = torch.repeat_interleave(torch.arange(n, device=dev), row_ptr[1:] - row_ptr[:-1], output_size=nE)
    return t_ptr, perm.to(torch.int32), tgt[perm].to(torch.int32)


def csr_transpose_symmetric(row_ptr, col):
    """``csr_transpose`` without the sort, for a symmetric graph whose columns
    ascend without duplicates inside every row (the env's graphs):
    there ``t_ptr == row_ptr`` and ``t_tgt == col``, and for entry ``p`` in row
    ``j`` with column ``i``, ``t_edge[p]`` is the position of ``j`` inside row
    ``i``: one ``searchsorted`` of the reverse keys ``i*n + j`` in the row-major
    keys ``j*n + i`` (which ascend). Returns ``(t_ptr, t_edge, t_tgt, ok)``,
    ``ok`` a bool tensor per entry: its reverse entry was found (where it is
    missing, ``t_edge[p] = p``, so every index stays in range). Plain
    torch on any device: the formulation ``gsm_graph_batch_gather`` is written
    against."""
    n, nE = row_ptr.numel() - 1, col.numel()
    dev = col.device
    t_tgt = col.to(torch.int32)
    if nE == 0 or n == 0:
        return (row_ptr, torch.zeros(0, dtype=torch.int32, device=dev), t_tgt,
                torch.ones(0, dtype=torch.bool, device=dev))
    src = col.to(torch.int64)
    tgt = torch.repeat_interleave(torch.arange(n, device=dev), row_ptr[1:] - row_ptr[:-1], output_size=nE)
    keys = tgt * n + src
    rev = src * n + tgt
    pos = torch.searchsorted(keys, rev).clamp_(max=nE - 1)
    ok = keys[pos] == rev
    t_edge = torch.where(ok, pos, torch.arange(nE, device=dev)).to(torch.int32)
    return row_ptr, t_edge, t_tgt, ok


def _check_kernel_inputs(q, k, v, row_ptr, col, edge_w, w_e, what):
    dev = q.device
    if dev.type != "cuda":
        raise _lib.GsmError(f"{what} needs a ROCm GPU; use attn_aggregate_ref on the CPU")
    for name, t, dt in (("q", q, torch.float32), ("k", k, torch.float32), ("v", v, torch.float32),
                        ("row_ptr", row_ptr, torch.int64), ("col", col, torch.int32)):
        if t.dtype != dt or not t.is_contiguous() or t.device != dev:
            raise ValueError(f"{name}: need a contiguous {dt} tensor on {dev}")
    if edge_w is not None and (edge_w.dtype != torch.float32 or w_e is None):
        raise ValueError("edge_w: float32, with w_e")


_ptr = _lib.ptr


class _AttnAggregateFn(torch.autograd.Function):
    """gsm_attn_aggregate_fwd / gsm_attn_aggregate_bwd (include/gsm.h)."""

    @staticmethod
    def forward(ctx, q, k, v, row_ptr, col, edge_w, w_e, skip, heads, scale, t_ptr, t_edge, t_tgt):
        n, HC = q.shape
        lib = _lib.load()
        out = torch.empty_like(q)
        lse = torch.empty(n, heads, dtype=torch.float32, device=q.device)
        # an empty tensor has no address; without edges the kernel reads neither col nor the edge terms
        col_arg = col if col.numel() else col.new_zeros(1)
        ew_arg, we_arg = (edge_w, w_e) if col.numel() else (None, None)
        stream = _lib.stream(q.device)
        rc = lib.gsm_attn_aggregate_fwd(_ptr(q), _ptr(k), _ptr(v), _ptr(ew_arg), _ptr(we_arg), _ptr(row_ptr),
                                        _ptr(col_arg), _ptr(skip), int(n), int(heads), int(HC // heads), scale,
                                        _ptr(out), _ptr(lse), stream)
        _lib.check(lib, rc, None, "gsm_attn_aggregate_fwd")
        ctx.save_for_backward(q, k, v, row_ptr, col, edge_w, w_e, skip, out, lse, t_ptr, t_edge, t_tgt)
        ctx.heads, ctx.scale = heads, scale
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_out):
        q, k, v, row_ptr, col, edge_w, w_e, skip, out, lse, t_ptr, t_edge, t_tgt = ctx.saved_tensors
        n, HC = q.shape
        nE, heads = col.numel(), ctx.heads
        lib = _lib.load()
        g = grad_out.to(torch.float32).contiguous()
        dq, dk, dv = torch.empty_like(q), torch.empty_like(q), torch.empty_like(q)
        dedge_w = torch.empty_like(edge_w) if (ctx.needs_input_grad[5] and edge_w is not None) else None
        dw_e = torch.empty_like(w_e) if (ctx.needs_input_grad[6] and w_e is not None) else None
        work = torch.empty(_lib.work_floats("gsm_attn_backward_work_floats", int(n), int(nE), int(heads),
                                            int(HC // heads)), dtype=torch.float32, device=q.device)
        stream = _lib.stream(q.device)
        ew_arg, we_arg = (edge_w, w_e) if nE else (None, None)
        rc = lib.gsm_attn_aggregate_bwd(_ptr(g), _ptr(q), _ptr(k), _ptr(v), _ptr(ew_arg), _ptr(we_arg), _ptr(row_ptr),
                                        _ptr(col), _ptr(out), _ptr(skip), _ptr(lse), _ptr(t_ptr), _ptr(t_edge),
                                        _ptr(t_tgt), int(n), int(nE), int(heads), int(HC // heads), ctx.scale,
                                        _ptr(work), _ptr(dq), _ptr(dk), _ptr(dv), _ptr(dedge_w), _ptr(dw_e),
                                        stream)
        _lib.check(lib, rc, None, "gsm_attn_aggregate_bwd")
        dskip = g if (ctx.needs_input_grad[7] and skip is not None) else None
        return dq, dk, dv, None, None, dedge_w, dw_e, dskip, None, None, None, None, None


def attn_aggregate_autograd(q, k, v, row_ptr, col, edge_w=None, w_e=None, skip=None, heads=1, scale=None,
                            transpose=None):
    """``attn_aggregate`` with gradients: forward and backward both on the HIP
    kernels (gsm_attn_aggregate_fwd / gsm_attn_aggregate_bwd in include/gsm.h).
    Gradients go to q, k, v, skip, w_e and edge_w; no double backward.
    ``transpose`` is ``csr_transpose(row_ptr, col)``; it is built here when it
    is not passed in, so pass it when the graph is reused."""
    n, HC = q.shape
    Cc = HC // heads
    scale = 1.0 / math.sqrt(Cc) if scale is None else float(scale)
    q, k, v = q.contiguous(), k.contiguous(), v.contiguous()
    _check_kernel_inputs(q, k, v, row_ptr, col, edge_w, w_e, "attn_aggregate_autograd")
    if edge_w is not None:
        edge_w, w_e = edge_w.contiguous(), w_e.contiguous()
        if edge_w.numel() != col.numel() or w_e.numel() != HC:
            raise ValueError("edge_w: one weight per CSR entry; w_e: heads*channels")
    if skip is not None:
        skip = skip.contiguous()
    if k.shape != q.shape or v.shape != q.shape or row_ptr.numel() != n + 1 or (
            skip is not None and skip.shape != q.shape):
        raise ValueError("q, k, v, skip: [n, heads*channels]; row_ptr: [n+1]")
    needs = torch.is_grad_enabled() and any(t is not None and t.requires_grad for t in (q, k, v, edge_w, w_e, skip))
    if needs and transpose is None:
        transpose = csr_transpose(row_ptr, col)
    t_ptr, t_edge, t_tgt = transpose if transpose is not None else (None, None, None)
    if transpose is not None:
        for name, t, dt, m in (("t_ptr", t_ptr, torch.int64, n + 1), ("t_edge", t_edge, torch.int32, col.numel()),
                               ("t_tgt", t_tgt, torch.int32, col.numel())):
            if t.dtype != dt or not t.is_contiguous() or t.device != q.device or t.numel() != m:
                raise ValueError(f"{name}: need a contiguous {dt} tensor of {m} on {q.device}")
    return _AttnAggregateFn.apply(q, k, v, row_ptr, col, edge_w, w_e, skip, int(heads), scale, t_ptr, t_edge, t_tgt)


def attn_aggregate(q, k, v, row_ptr, col, edge_w=None, w_e=None, skip=None, heads=1, scale=None):
    """HIP kernel (no autograd): see gsm_attn_aggregate in include/gsm.h."""
    n, HC = q.shape
    Cc = HC // heads
    scale = 1.0 / math.sqrt(Cc) if scale is None else float(scale)
    dev = q.device
    _check_kernel_inputs(q, k, v, row_ptr, col, edge_w, w_e, "attn_aggregate")
    lib = _lib.load()
    out = torch.empty_like(q)
    rc = lib.gsm_attn_aggregate(_ptr(q), _ptr(k), _ptr(v), _ptr(edge_w),
                                _ptr(w_e.contiguous() if w_e is not None else None), _ptr(row_ptr), _ptr(col),
                                _ptr(skip.contiguous() if skip is not None else None), int(n), int(heads), int(Cc),
                                scale, _ptr(out), _lib.stream(dev))
    _lib.check(lib, rc, None, "gsm_attn_aggregate")
    return out


def pack_conv_params(conv):
    """The projections of a ``TransformerConv`` (``concat=True``) in the layout
    ``gsm_env_conv`` reads: ``w`` [3 or 4, HC, in_channels+1], the blocks
    query, key, value and (with ``root_weight``) skip, a row = the weights of
    the input features then the bias (for ``in_channels = 7`` a 32-byte row);
    ``w_e`` [HC] = the edge projection, or None with ``edge_dim=None``.
    Differentiable (a ``cat`` of the parameters)."""
    if not conv.concat:
        raise ValueError("pack_conv_params: concat=True layers only")
    lins = [conv.lin_query, conv.lin_key, conv.lin_value] + ([conv.lin_skip] if conv.lin_skip is not None else [])
    w = torch.stack([torch.cat([l.weight, l.bias[:, None]], 1) for l in lins]).contiguous()
    w_e = conv.lin_edge.weight[:, 0].contiguous() if conv.lin_edge is not None else None
    return w, w_e


def _env_graph_total(edge_ptr, edge_index):
    total = int(edge_ptr[-1])
    if total > edge_index.shape[1]:
        raise ValueError(f"the graph's {total} entries run past the {edge_index.shape[1]} stored (a truncated "
                         "rollout slot); size the buffer with a larger edge capacity")
    return total


def env_conv_ref(node_feat, edge_ptr, edge_index, edge_attr, w, w_e, heads, rows_out, skip, row_ptr=False):
    """``env_conv`` in plain torch on any device and dtype (differentiable):
    ``env_csr``, the linear maps of ``w``, ``attn_aggregate_ref`` and the row
    slice. The reference of the kernel and the fallback of ``forward_env``.
    Returns ``out`` [B, rows_out, HC], or ``(out, row_ptr)``."""
    B, E, F = node_feat.shape
    n = B * E
    if w.shape[0] != (4 if skip else 3) or w.shape[2] != F + 1:
        raise ValueError("w: [4 if skip else 3, heads*channels, in_channels+1]")
    total = _env_graph_total(edge_ptr, edge_index)
    ei = edge_index[:, :total]
    ptr = env_csr(ei, n)
    x = node_feat.reshape(n, F)
    q, k, v = (x @ w[i, :, :F].t() + w[i, :, F] for i in range(3))
    sk = x @ w[3, :, :F].t() + w[3, :, F] if skip else None
    ew = edge_attr.reshape(-1)[:total] if w_e is not None else None
    out = attn_aggregate_ref(q, k, v, ptr, ei[1], ew, w_e, sk, heads)
    out = out.view(B, E, -1)[:, :rows_out]
    return (out, ptr) if row_ptr else out


def env_conv_bwd_ref(grad_out, node_feat, edge_ptr, edge_index, edge_attr, w, w_e, heads, rows_out, skip,
                     node_grads=False):
    """The weight gradients of ``env_conv_ref`` written out (plain torch, any
    dtype and device): the restatement ``gsm_env_conv_bwd`` is written against.
    ``grad_out`` [B, rows_out, HC]; the rows past ``rows_out`` have ``g_i =
    0``. With ``x_i`` the node's features and a trailing 1, and ``dq, dk, dv``
    of ``attn_aggregate_bwd_ref`` on ``env_csr`` of the graph::

        dW_q[c][f]    = sum_i dq_i[c] x_i[f]      dW_k[c][f] = sum_j dk_j[c] x_j[f]
        dW_skip[c][f] = sum_i g_i[c]  x_i[f]      dW_v[c][f] = sum_j dv_j[c] x_j[f]

    over every node of every env. Returns ``(dw, dw_e)``: ``dw`` [3 or 4, HC,
    F+1] in the layout of ``pack_conv_params`` (the last column the bias
    gradient), ``dw_e`` [HC] or None without ``w_e``; with ``node_grads`` also
    ``(dq, dk, dv, g)``, each [B*E, HC]."""
    B, E, F = node_feat.shape
    n = B * E
    if w.shape[0] != (4 if skip else 3) or w.shape[2] != F + 1:
        raise ValueError("w: [4 if skip else 3, heads*channels, in_channels+1]")
    HC = w.shape[1]
    total = _env_graph_total(edge_ptr, edge_index)
    ei = edge_index[:, :total]
    ptr = env_csr(ei, n)
    x = node_feat.reshape(n, F)
    q, k, v = (x @ w[i, :, :F].t() + w[i, :, F] for i in range(3))
    sk = x @ w[3, :, :F].t() + w[3, :, F] if skip else None
    ew = edge_attr.reshape(-1)[:total] if w_e is not None else None
    g = torch.zeros(B, E, HC, dtype=x.dtype, device=x.device)
    g[:, :rows_out] = grad_out
    g = g.view(n, HC)
    dq, dk, dv, _, dw_e, _ = attn_aggregate_bwd_ref(g, q, k, v, ptr, ei[1], ew, w_e, sk, heads)
    x1 = torch.cat([x, torch.ones(n, 1, dtype=x.dtype, device=x.device)], 1)
    dw = torch.stack([d.t() @ x1 for d in (dq, dk, dv) + ((g,) if skip else ())])
    return (dw, dw_e, (dq, dk, dv, g)) if node_grads else (dw, dw_e)


def _env_conv_args(node_feat, edge_ptr, edge_index, edge_attr, w, w_e, heads, skip, what):
    """The argument checks of ``env_conv`` / ``env_conv_autograd``. Returns
    ``(edge_attr flattened, w_e contiguous, entry bound, row stride, HC)``."""
    dev = node_feat.device
    if dev.type != "cuda":
        raise _lib.GsmError(f"{what} needs a ROCm GPU; use env_conv_ref on the CPU")
    if node_feat.dim() != 3 or node_feat.shape[2] != 7:
        raise ValueError("node_feat: [B, E, 7]")
    B, E, _ = node_feat.shape
    if edge_index.dim() != 2 or edge_index.shape[0] != 2:
        raise ValueError("edge_index: [2, cap]")
    limit = int(edge_index.shape[1])
    edge_attr = edge_attr.reshape(-1) if edge_attr.dim() != 1 else edge_attr
    for name, t, dt, contig in (("node_feat", node_feat, torch.float32, True), ("edge_ptr", edge_ptr, torch.int64, True),
                                ("edge_index", edge_index, torch.int32, False),
                                ("edge_attr", edge_attr, torch.float32, True), ("w", w, torch.float32, True)):
        if t.dtype != dt or t.device != dev or (contig and not t.is_contiguous()):
            raise ValueError(f"{name}: need a {'contiguous ' if contig else ''}{dt} tensor on {dev}")
    if limit and edge_index.stride(1) != 1:
        raise ValueError("edge_index: rows must be contiguous")
    if edge_ptr.numel() != B + 1 or edge_attr.numel() < limit:
        raise ValueError("edge_ptr: [B+1]; edge_attr: one distance per edge_index column")
    if w.dim() != 3 or w.shape[0] != (4 if skip else 3) or w.shape[2] != 8 or w.shape[1] % heads:
        raise ValueError("w: [4 if skip else 3, heads*channels, 8]")
    HC = int(w.shape[1])
    if w_e is not None:
        w_e = w_e.contiguous()
        if w_e.dtype != torch.float32 or w_e.device != dev or w_e.numel() != HC:
            raise ValueError(f"w_e: float32 [heads*channels] on {dev}")
    stride = int(edge_index.stride(0)) if limit else 0
    return edge_attr, w_e, limit, stride, HC


def _raise_env_status(st, limit, what):
    if st & _lib.BATCH_TRUNCATED:
        raise ValueError(f"{what}: an env's entries run past the {limit} stored (a truncated rollout slot); "
                         "size the buffer with a larger edge capacity")
    if st:
        msgs = [m for bit, m in ((_lib.BATCH_BAD_OFFSETS, "an env's edge offsets are not 0 <= start <= end"),
                                 (_lib.BATCH_OUT_OF_ENV, "an entry's node id lies outside its env or its rows "
                                                         "do not ascend"),
                                 (_lib.BATCH_ASYMMETRIC, "an entry's reverse entry is missing (the backward needs "
                                                         "a symmetric graph)")) if st & bit]
        raise RuntimeError(f"{what}: the graph is invalid (status {st}): " + "; ".join(msgs))


def env_conv(node_feat, edge_ptr, edge_index, edge_attr, w, w_e, heads, rows_out, skip, row_ptr=False, check=True):
    """One TransformerConv layer (in_channels 7, edge_dim 1 or None, concat) on
    an env-form graph in one HIP launch (gsm_env_conv in include/gsm.h; no
    autograd). ``node_feat`` f32 [B, E, 7]; ``edge_ptr`` int64 [B+1];
    ``edge_index`` int32 [2, cap] or its ``[:, :total]`` view (the row stride
    is taken from the tensor, the entry bound is ``shape[1]``); ``edge_attr``
    f32 with at least that many entries; ``w``, ``w_e`` from
    ``pack_conv_params``; ``rows_out``: E for every row, N for the agents'.
    Returns ``out`` [B, rows_out, HC], then ``row_ptr`` int64 [B*E+1] (the
    offsets ``env_csr`` gives) when asked for. With ``check`` one read of the
    kernel's status raises ValueError for an env whose entries run past the
    bound (a truncated rollout slot) and RuntimeError for corrupt offsets or
    ids; without it the status (device int32 [1], GSM_BATCH_* bits) is
    returned last and such envs are edgeless."""
    edge_attr, w_e, limit, stride, HC = _env_conv_args(node_feat, edge_ptr, edge_index, edge_attr, w, w_e, heads, skip,
                                                       "env_conv")
    dev = node_feat.device
    B, E, _ = node_feat.shape
    Cc = HC // heads
    lib = _lib.load()
    out = torch.empty(B, int(rows_out), HC, dtype=torch.float32, device=dev)
    ptr = torch.empty(B * E + 1, dtype=torch.int64, device=dev) if row_ptr else None
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    stream = _lib.stream(dev)
    rc = lib.gsm_env_conv(_ptr(node_feat) if B else None, _ptr(edge_ptr), _ptr(edge_index) if limit else None, stride,
                          _ptr(edge_attr) if limit else None, limit, _ptr(w), _ptr(w_e), int(B), int(E), int(heads),
                          int(Cc), 1.0 / math.sqrt(Cc), _lib.CONV_SKIP if skip else 0, int(rows_out), _ptr(out),
                          _ptr(ptr), _ptr(status), stream)
    _lib.check(lib, rc, None, "gsm_env_conv")
    res = (out,) + ((ptr,) if row_ptr else ())
    if check:
        _raise_env_status(int(status.item()), limit, "env_conv")
    else:
        res = res + (status,)
    return res[0] if len(res) == 1 else res


class _EnvConvFn(torch.autograd.Function):
    """gsm_env_conv_fwd / gsm_env_conv_bwd (include/gsm.h)."""

    @staticmethod
    def forward(ctx, w, w_e, node_feat, edge_ptr, edge_index, edge_attr, heads, rows_out, skip, want_ptr, check):
        edge_attr, w_e, limit, stride, HC = _env_conv_args(node_feat, edge_ptr, edge_index, edge_attr, w, w_e, heads,
                                                           skip, "env_conv_autograd")
        dev = node_feat.device
        B, E, _ = node_feat.shape
        Cc = HC // heads
        lib = _lib.load()
        out = torch.empty(B, rows_out, HC, dtype=torch.float32, device=dev)
        lse = torch.empty(B, rows_out, heads, dtype=torch.float32, device=dev)
        ptr = torch.empty(B * E + 1, dtype=torch.int64, device=dev) if want_ptr else None
        status = torch.zeros(1, dtype=torch.int32, device=dev)
        stream = _lib.stream(dev)
        rc = lib.gsm_env_conv_fwd(_ptr(node_feat) if B else None, _ptr(edge_ptr), _ptr(edge_index) if limit else None,
                                  stride, _ptr(edge_attr) if limit else None, limit, _ptr(w), _ptr(w_e), int(B),
                                  int(E), int(heads), int(Cc), 1.0 / math.sqrt(Cc), _lib.CONV_SKIP if skip else 0,
                                  rows_out, _ptr(out), _ptr(lse), _ptr(ptr), _ptr(status), stream)
        _lib.check(lib, rc, None, "gsm_env_conv_fwd")
        if check:
            _raise_env_status(int(status.item()), limit, "env_conv_autograd")
        ctx.save_for_backward(w, w_e, node_feat, edge_ptr, edge_index, edge_attr, out, lse, status)
        ctx.args = (heads, rows_out, skip, check, limit, stride)
        ctx.mark_non_differentiable(status, *((ptr,) if want_ptr else ()))
        return out, ptr, status

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_out, _grad_ptr, _grad_status):
        w, w_e, node_feat, edge_ptr, edge_index, edge_attr, out, lse, status = ctx.saved_tensors
        heads, rows_out, skip, check, limit, stride = ctx.args
        dev = node_feat.device
        B, E, _ = node_feat.shape
        HC = int(w.shape[1])
        Cc = HC // heads
        lib = _lib.load()
        g = grad_out.to(torch.float32).contiguous()
        flags = _lib.CONV_SKIP if skip else 0
        work = torch.empty(_lib.work_floats("gsm_env_conv_backward_work_floats", int(B), int(E), limit, int(heads),
                                            int(Cc), flags), dtype=torch.float32, device=dev)
        dw = torch.empty_like(w)
        dw_e = torch.empty_like(w_e) if (w_e is not None and ctx.needs_input_grad[1]) else None
        stream = _lib.stream(dev)
        rc = lib.gsm_env_conv_bwd(_ptr(g) if B else None, _ptr(node_feat) if B else None, _ptr(edge_ptr),
                                  _ptr(edge_index) if limit else None, stride, _ptr(edge_attr) if limit else None,
                                  limit, _ptr(w), _ptr(w_e), _ptr(out) if B else None, _ptr(lse) if B else None,
                                  int(B), int(E), int(heads), int(Cc), 1.0 / math.sqrt(Cc), flags, rows_out,
                                  _ptr(work), _ptr(dw), _ptr(dw_e), _ptr(status), stream)
        _lib.check(lib, rc, None, "gsm_env_conv_bwd")
        if check:
            _raise_env_status(int(status.item()), limit, "env_conv_autograd (backward)")
        return (dw if ctx.needs_input_grad[0] else None, dw_e) + (None,) * 9


def env_conv_autograd(node_feat, edge_ptr, edge_index, edge_attr, w, w_e, heads, rows_out, skip, row_ptr=False,
                      check=True):
    """``env_conv`` with gradients for ``w`` and ``w_e``: forward and backward
    both on the HIP kernels (gsm_env_conv_fwd / gsm_env_conv_bwd in
    include/gsm.h), so neither direction forms an [n, HC] tensor. The
    arguments and the results are ``env_conv``'s; ``node_feat`` and
    ``edge_attr`` are env data and get no gradient (a call that wants one takes
    ``env_conv_ref``); no double backward. The backward checks the graph again
    (it trusts no forward) and, relying on the env graph's symmetry, also
    reports an entry whose reverse entry is missing. With ``check`` the status
    is read once in the forward and once in the backward, each raising as
    ``env_conv`` does; without it the status tensor is returned last, and the
    backward ORs its bits into that same tensor (no read)."""
    if node_feat.requires_grad or edge_attr.requires_grad:
        raise ValueError("env_conv_autograd: no gradients for node_feat or edge_attr; use env_conv_ref")
    out, ptr, status = _EnvConvFn.apply(w, w_e, node_feat, edge_ptr, edge_index, edge_attr, int(heads), int(rows_out),
                                        bool(skip), bool(row_ptr), bool(check))
    res = (out,) + ((ptr,) if row_ptr else ()) + (() if check else (status,))
    return res[0] if len(res) == 1 else res


class TransformerConv(torch.nn.Module):
    """``TransformerConv(in_channels, out_channels, heads, concat, edge_dim=1,
    root_weight=True)`` in the torch-geometric parameterisation, with the
    aggregation on the HIP kernel when no gradient is needed. With
    ``kernel_backward=True`` (and ``use_kernel``, on the GPU) the training path
    takes the HIP forward and backward kernels (``attn_aggregate_autograd``)
    too; ``forward(..., transpose=csr_transpose(row_ptr, col))`` reuses the
    transposed graph across calls. The default keeps the torch formulation.
    ``forward_env`` is the layer on an env-form graph (what the env returns, or
    a rollout-buffer slot), fused into one launch where ``env_conv`` applies;
    with ``kernel_backward=True`` it trains on the fused kernels as well
    (``env_conv_autograd``: gradients for the parameters, none for the env
    data)."""

    def __init__(self, in_channels: int, out_channels: int, heads: int = 1, concat: bool = True,
                 edge_dim: Optional[int] = 1, root_weight: bool = True, use_kernel: bool = True,
                 kernel_backward: bool = False):
        super().__init__()
        self.heads, self.out_channels, self.concat = heads, out_channels, concat
        HC = heads * out_channels
        self.lin_query = torch.nn.Linear(in_channels, HC)
        self.lin_key = torch.nn.Linear(in_channels, HC)
        self.lin_value = torch.nn.Linear(in_channels, HC)
        self.lin_edge = torch.nn.Linear(edge_dim, HC, bias=False) if edge_dim else None
        self.lin_skip = torch.nn.Linear(in_channels, HC if concat else out_channels) if root_weight else None
        self.use_kernel = use_kernel
        self.kernel_backward = kernel_backward

    def forward(self, x: torch.Tensor, row_ptr: torch.Tensor, col: torch.Tensor,
                edge_attr: Optional[torch.Tensor] = None, transpose=None) -> torch.Tensor:
        n = x.shape[0]
        q, k, v = self.lin_query(x), self.lin_key(x), self.lin_value(x)
        w_e = self.lin_edge.weight[:, 0] if (self.lin_edge is not None and edge_attr is not None) else None
        ew = edge_attr.reshape(-1) if w_e is not None else None
        skip = self.lin_skip(x) if (self.lin_skip is not None and self.concat) else None
        grad = torch.is_grad_enabled() and any(p.requires_grad for p in self.parameters())
        needs = torch.is_grad_enabled() and (grad or x.requires_grad or (ew is not None and ew.requires_grad))
        if self.use_kernel and self.kernel_backward and x.is_cuda and needs:
            out = attn_aggregate_autograd(q, k, v, row_ptr, col.to(torch.int32), ew, w_e, skip, self.heads,
                                          transpose=transpose)
        elif self.use_kernel and x.is_cuda and not grad:
            out = attn_aggregate(q.contiguous(), k.contiguous(), v.contiguous(), row_ptr, col.to(torch.int32),
                                 ew, w_e, skip, self.heads)
        else:
            out = attn_aggregate_ref(q, k, v, row_ptr, col, ew, w_e, skip, self.heads)
        if not self.concat:
            out = out.view(n, self.heads, self.out_channels).mean(1)
            if self.lin_skip is not None:
                out = out + self.lin_skip(x)
        return out

    def _env_kernel_shapes(self, node_feat):
        if not (self.use_kernel and self.concat and node_feat.is_cuda and node_feat.dtype == torch.float32):
            return False
        if self.lin_query.in_features != 7 or (self.lin_edge is not None and self.lin_edge.in_features != 1):
            return False
        B, E, _ = node_feat.shape
        Cc, HC = self.out_channels, self.heads * self.out_channels
        return Cc & (Cc - 1) == 0 and HC <= 64 and 1 <= E <= _lib.CONV_MAX_ENTITIES and B * E < 2 ** 31

    def _env_kernel_ok(self, node_feat, edge_attr):
        if torch.is_grad_enabled() and (node_feat.requires_grad or edge_attr.requires_grad or
                                        any(p.requires_grad for p in self.parameters())):
            return False
        return self._env_kernel_shapes(node_feat)

    def _env_kernel_grad_ok(self, node_feat, edge_attr):
        """The training path of ``forward_env`` on the kernels: opted in, a
        parameter wants a gradient and the env data does not."""
        if not (self.kernel_backward and torch.is_grad_enabled()) or node_feat.requires_grad or edge_attr.requires_grad:
            return False
        params = list(self.parameters())
        if not any(p.requires_grad for p in params) or any(p.dtype != torch.float32 for p in params):
            return False
        return self._env_kernel_shapes(node_feat)

    def _packed(self):
        """``pack_conv_params`` of the current parameter values, packed again
        only after a parameter changed (inference path, no gradient): the key
        is every parameter's storage address and ``_version``. A write torch
        does not see (a kernel writing through ``data_ptr()``) has to raise
        the version, as ``ClippedAdam.mark_updated`` does."""
        key = tuple((p.data_ptr(), p._version) for p in self.parameters())
        if getattr(self, "_pack_key", None) != key:
            with torch.no_grad():
                self._pack = tuple(t.float() if t is not None else None for t in pack_conv_params(self))
            self._pack_key = key
        return self._pack

    def forward_env(self, graph: dict, rows: str = "all", n_agents: Optional[int] = None, row_ptr: bool = False):
        """The layer on an env-form graph: any dict with ``node_feat`` [B, E,
        F], ``edge_ptr`` [B+1], ``edge_index`` [2, cap or total] (global ids) and
        ``edge_attr``: what ``GpuBatchEnv.step`` / ``reset`` / ``observe`` return
        (either ``sync_edges``) or ``GraphRolloutBuffer.slot(t)``. Returns [B,
        rows, HC]: every row (``rows="all"``) or the first ``n_agents`` of each
        env (``rows="agents"``); with ``row_ptr`` also the per-node offsets of
        ``env_csr``, for a further layer on ``forward``. One HIP launch
        (``env_conv``) when the tensors are on the GPU, no gradient is wanted,
        ``use_kernel``, ``concat``, 7 input features, edge_dim 1 or None and the
        kernel's shape limits hold. Under those same conditions, with
        ``kernel_backward`` set, a parameter that wants a gradient and env data
        (``node_feat``, ``edge_attr``) that wants none, the training path runs on
        the kernels too (``env_conv_autograd``: the fused forward with its
        softmax statistics and the fused backward, the status read once in each).
        The differentiable torch formulation (``env_conv_ref``) otherwise."""
        nf, ei, ea = graph["node_feat"], graph["edge_index"], graph["edge_attr"]
        B, E, F = nf.shape
        if rows == "all":
            R = E
        elif rows == "agents":
            if n_agents is None or not 1 <= n_agents <= E:
                raise ValueError('rows="agents" needs n_agents in [1, E]')
            R = int(n_agents)
        else:
            raise ValueError('rows: "all" or "agents"')
        if self._env_kernel_ok(nf, ea):
            w, w_e = self._packed()
            return env_conv(nf.contiguous(), graph["edge_ptr"], ei, ea, w, w_e, self.heads, R,
                            self.lin_skip is not None, row_ptr=row_ptr)
        if self._env_kernel_grad_ok(nf, ea):
            w, w_e = pack_conv_params(self)                  # differentiable: autograd splits dw onto the parameters
            return env_conv_autograd(nf.contiguous(), graph["edge_ptr"], ei, ea, w, w_e, self.heads, R,
                                     self.lin_skip is not None, row_ptr=row_ptr)
        if self.concat:
            w, w_e = pack_conv_params(self)
            return env_conv_ref(nf, graph["edge_ptr"], ei, ea, w, w_e, self.heads, R, self.lin_skip is not None,
                                row_ptr=row_ptr)
        total = _env_graph_total(graph["edge_ptr"], ei)
        ptr = env_csr(ei[:, :total], B * E)
        out = self.forward(nf.reshape(B * E, F), ptr, ei[1, :total], ea.reshape(-1)[:total, None])
        out = out.view(B, E, -1)[:, :R]
        return (out, ptr) if row_ptr else out
