"""Every later read sees a parameter write (CPU): TransformerConv._packed, the
cache of the no-grad forward_env path, is pack_conv_params of the live values
after each kind of write a trainer makes, and ClippedAdam's cached pointer
tables follow a replaced storage.

_packed's key is (data_ptr, _version) per parameter. A write torch makes
(copy_, an in-place op, load_state_dict) raises _version. gsm_adam_step writes
through raw pointers; its stand-in here is a ctypes.memmove into the storage,
which leaves _version alone, followed by ClippedAdam.mark_updated(): what the
kernel path of step() does, and what a replayed captured step needs.
test_gpu_train_iterations.py runs the same on the kernels."""
import ctypes

import pytest
import torch

from gsmarl_amd import ClippedAdam
from gsmarl_amd import optim as O
from gsmarl_amd.gnn import TransformerConv, pack_conv_params


def _conv(seed=0, in_channels=7):
    torch.manual_seed(seed)
    return TransformerConv(in_channels, 16, heads=3, use_kernel=False)


def _stepped(conv, seed=1):
    """A fallback ClippedAdam over the conv's parameters after one step."""
    g = torch.Generator().manual_seed(seed)
    params = list(conv.parameters())
    for p in params:
        p.grad = torch.randn(p.shape, generator=g)
    opt = ClippedAdam(params, use_kernel=False)
    assert not opt.kernel
    opt.step()
    return params, opt


def _poke(p, values):
    """Write ``values`` into the parameter's storage behind torch's back."""
    src = values.detach().to(p.dtype).contiguous()
    assert src.shape == p.shape and p.is_contiguous()
    ctypes.memmove(p.data_ptr(), src.data_ptr(), src.numel() * src.element_size())


def _fresh(conv):
    with torch.no_grad():
        return pack_conv_params(conv)


def _snapshot(pack):
    """Copies: w_e of a pack may be a view of the live lin_edge weight."""
    return tuple(t.detach().clone() for t in pack)


def _assert_packed_is_fresh(conv, before):
    got, want = conv._packed(), _fresh(conv)
    for a, b, old in zip(got, want, before):
        assert a.dtype == b.dtype and torch.equal(a, b)
        assert not torch.equal(a, old)
    assert conv._packed()[0] is got[0]                       # nothing changed since: the same pack, not a repack


def _write_ref_step(conv):
    _stepped(conv)


def _write_load_state_dict(conv):
    conv.load_state_dict(_conv(seed=5).state_dict())


def _write_inplace(conv):
    with torch.no_grad():
        for p in conv.parameters():
            p.add_(0.25)


@pytest.mark.parametrize("write", [_write_ref_step, _write_load_state_dict, _write_inplace],
                         ids=["ref-step", "load_state_dict", "inplace"])
def test_packed_follows_a_write_torch_sees(write):
    conv = _conv()
    before = _snapshot(conv._packed())
    for a, b in zip(before, _fresh(conv)):
        assert torch.equal(a, b)
    write(conv)
    _assert_packed_is_fresh(conv, before)


def test_packed_follows_a_raw_write_after_mark_updated():
    conv = _conv()
    params, opt = _stepped(conv)
    before = _snapshot(conv._packed())
    versions = [p._version for p in params]
    g = torch.Generator().manual_seed(2)
    for p in params:
        _poke(p, p + 0.1 * torch.randn(p.shape, generator=g))
    assert [p._version for p in params] == versions          # torch did not see the writes
    opt.mark_updated()
    assert all(p._version > v for p, v in zip(params, versions))
    _assert_packed_is_fresh(conv, before)


def test_mark_updated_marks_the_last_active_set_only():
    conv = _conv()
    params = list(conv.parameters())
    for p in params[1:]:
        p.grad = torch.ones_like(p)
    opt = ClippedAdam(params, use_kernel=False)
    start = [p._version for p in params]
    opt.mark_updated()                                       # before any step: nothing to mark
    assert [p._version for p in params] == start
    opt.step()
    versions = [p._version for p in params]
    assert versions[0] == start[0] and all(v > s for v, s in zip(versions[1:], start[1:]))
    opt.mark_updated()
    assert [p._version for p in params] == [versions[0]] + [v + 1 for v in versions[1:]]


def _ring(n, seed):
    """A ring graph of n nodes in CSR (each node hears its two neighbours) with distances."""
    row_ptr = torch.arange(0, 2 * n + 1, 2, dtype=torch.int64)
    col = torch.stack([(torch.arange(n) - 1) % n, (torch.arange(n) + 1) % n], 1).reshape(-1).to(torch.int32)
    g = torch.Generator().manual_seed(seed)
    return torch.randn(n, 48, generator=g), row_ptr, col, torch.rand(2 * n, generator=g)


@torch.no_grad()
def test_uncached_forward_reads_the_live_weights():
    """A second layer (TransformerConv.forward) keeps no pack: a raw write shows at once."""
    conv2 = _conv(seed=3, in_channels=48)
    x, row_ptr, col, ew = _ring(9, seed=4)
    out0 = conv2(x, row_ptr, col, ew)
    g = torch.Generator().manual_seed(6)
    for p in conv2.parameters():
        _poke(p, p + 0.1 * torch.randn(p.shape, generator=g))
    out1 = conv2(x, row_ptr, col, ew)
    twin = _conv(seed=7, in_channels=48)
    twin.load_state_dict(conv2.state_dict())
    assert torch.equal(out1, twin(x, row_ptr, col, ew))
    assert not torch.equal(out1, out0)


def _addr(a):
    return [x or 0 for x in a]


def test_table_follows_a_replaced_storage():
    """ClippedAdam._table: the cached pointer arrays of an active set are built
    again when a parameter has another storage, and only then."""
    params = [torch.nn.Parameter(torch.randn(5)), torch.nn.Parameter(torch.randn(3, 4)),
              torch.nn.Parameter(torch.zeros(0))]
    opt = ClippedAdam(params, use_kernel=False)
    act = (0, 1, 2)
    args = (act, params, opt.exp_avg, opt.exp_avg_sq)
    tab = opt._table(*args)
    assert tab.key == O._table_key(params) == tuple(p.data_ptr() for p in params)
    assert _addr(tab.p) == [params[0].data_ptr(), params[1].data_ptr(), 0] and list(tab.n) == [5, 12, 0]
    assert opt._table(*args) is tab
    with torch.no_grad():
        params[0].add_(1.0)                                  # a write is not a new storage
    assert opt._table(*args) is tab
    old = params[0].data                                     # kept alive: its address cannot be handed out again
    params[0].data = old.clone()
    assert params[0].data_ptr() != old.data_ptr()
    new = opt._table(*args)
    assert new is not tab and opt._table(*args) is new
    assert _addr(new.p) == [params[0].data_ptr(), params[1].data_ptr(), 0]
    assert _addr(new.m) == _addr(tab.m) and _addr(new.v) == _addr(tab.v) and list(new.n) == list(tab.n)
    assert _addr(tab.p)[0] == old.data_ptr()
    # another active set has a table of its own, untouched by the rebuild
    sub = opt._table((1,), params[1:2], opt.exp_avg[1:2], opt.exp_avg_sq[1:2])
    assert sub is not new and opt._table(*args) is new
    # what the kernel cannot update is refused when it appears: another shape (the moments keep theirs), another dtype
    kept = params[1].data
    params[1].data = torch.zeros(13)
    with pytest.raises(ValueError):
        opt._table(*args)
    params[1].data = kept.double()
    with pytest.raises(ValueError):
        opt._table(*args)
    params[1].data = kept
    assert opt._table(*args) is new
