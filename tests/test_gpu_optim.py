"""gsm_adam_step (gsmarl_amd.optim.ClippedAdam) on the GPU against
clipped_adam_ref in fp64 stepped from the kernel's own fp32 state before each
step, five consecutive steps a case, in the scales of tests/optim_cases.py:

    |m - m64| <= Km 2^-24 sm        |v - v64| <= Kv 2^-24 sv
    |p - p64| <= 2^-24 |p64| + Kp 2^-24 step_size sm / denom64
    |norm - norm64| <= 2^-23 norm64   (an fp64 sum and one rounding: derived)

Km, Kv, Kp = 16, 32, 32: four times what the fp32 torch restatement shows on
the same cases (test_optim_ref.py measures 3.2, 5.2, 4.1), rounded up to a
power of two; the margin is for a legitimately different operation order. The
largest kernel ratios are printed. Everything else is bit for bit: two calls,
alignment, a non-contiguous gradient, the split over launches, coef == 1
against no clip, the skipped update, a frozen parameter, a captured step
against eager ones; and one joined case: the n3 chain of
test_gpu_train_chain.py, its kernel backward, then the step."""
import pytest
import torch

import optim_cases as oc
import train_chain as tc
from gsmarl_amd import ClippedAdam, _lib
from gsmarl_amd import optim as O

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
WORST = {"m": 0.0, "v": 0.0, "p": 0.0}


def bits(t):
    return t.detach().contiguous().view(torch.int32)


def same(a, b, what=""):
    assert a.shape == b.shape and a.dtype == b.dtype and torch.equal(bits(a), bits(b)), what


def _instance(st, max_norm="case", **kw):
    """A ClippedAdam on fresh copies of the state's tensors (those with and without a gradient)."""
    params = [torch.nn.Parameter(p.clone()) for p in st["p"]]
    opt = ClippedAdam(params, lr=oc.LR, betas=oc.BETAS, eps=oc.EPS,
                      max_grad_norm=st["max_norm"] if max_norm == "case" else max_norm, **kw)
    assert opt.kernel
    for dst, src in zip(opt.exp_avg + opt.exp_avg_sq, st["m"] + st["v"]):
        dst.copy_(src)
    opt.step_count.fill_(st["t"])
    for q, g in zip(params, st["g"]):
        q.grad = g.clone() if g is not None else None
    return params, opt


def _state(params, opt):
    """The kernel's own fp32 state, copied: what the fp64 reference steps from."""
    return dict(p=[q.detach().clone() for q in params], m=[m.clone() for m in opt.exp_avg],
                v=[v.clone() for v in opt.exp_avg_sq], g=[q.grad.clone() if q.grad is not None else None for q in params],
                t=int(opt.step_count.item()), max_norm=opt.max_grad_norm)


def _same_state(a, b, what=""):
    for key in "pmv":
        for i, (x, y) in enumerate(zip(a[key], b[key])):
            same(x, y, (what, key, i))
    assert a["t"] == b["t"], what


@pytest.mark.parametrize("case", oc.PARITY)
def test_against_fp64_from_the_same_state(case):
    st0 = oc.make(case, device=DEV)
    params, opt = _instance(st0)
    worst = [0.0, 0.0, 0.0]
    for k in range(5):
        for q, g in zip(params, st0["g"]):
            if g is not None:
                q.grad = g * (0.5 + 0.25 * k)
        st = _state(params, opt)
        opt.step()
        idx = oc.active(st)
        got = dict(p=[params[i].detach() for i in idx], m=[opt.exp_avg[i] for i in idx],
                   v=[opt.exp_avg_sq[i] for i in idx])
        rm, rv, rp, ref = oc.ratios(st, got, opt.lr)
        worst = [max(a, b) for a, b in zip(worst, (rm, rv, rp))]
        norm, coef, count, skipped = opt.stats.tolist()
        norm64, coef64 = float(ref["stats"][0]), float(ref["stats"][1])
        assert abs(norm - norm64) <= 2.0 ** -23 * norm64, (k, norm, norm64)
        assert abs(coef - coef64) <= 4 * oc.U * coef64 and (coef == 1.0) == (coef64 == 1.0)
        assert count == st["t"] + 1 == int(opt.step_count.item()) and skipped == 0.0 and int(opt.status.item()) == 0
        for i in idx:                                        # gradients are inputs
            same(params[i].grad, st["g"][i], i)
    print(f"{case}: kernel, largest ratios m {worst[0]:.2f} (bound {oc.KM:.0f}) v {worst[1]:.2f} ({oc.KV:.0f}) "
          f"p {worst[2]:.2f} ({oc.KP:.0f})")
    for key, w in zip("mvp", worst):
        WORST[key] = max(WORST[key], w)
    print(f"so far: m {WORST['m']:.2f} v {WORST['v']:.2f} p {WORST['p']:.2f}")
    assert worst[0] <= oc.KM and worst[1] <= oc.KV and worst[2] <= oc.KP, worst
    if case == "zero":
        for q, p0 in zip(params, st0["p"]):
            same(q, p0)


def _offset(t, floats):
    """A copy of ``t`` whose base lies ``floats`` floats past a 256-byte boundary."""
    buf = torch.empty(t.numel() + 64 + floats, dtype=t.dtype, device=t.device)
    lead = (-buf.data_ptr() // 4) % 64 + floats
    out = buf[lead:lead + t.numel()]
    out.copy_(t)
    assert t.numel() == 0 or out.data_ptr() % 256 == 4 * floats
    return out


def _call(st, floats=0, max_norm="case"):
    """One gsm_adam_step through optim._adam_call on copies of the state, every tensor ``floats`` floats past a
    256-byte boundary. Returns the state after it, with stats and status."""
    idx = oc.active(st)
    p, g, m, v = ([_offset(st[key][i], floats) for i in idx] for key in "pgmv")
    lr = torch.full((1,), oc.LR, dtype=torch.float32, device=DEV)
    step = torch.full((1,), st["t"], dtype=torch.int32, device=DEV)
    status = torch.zeros(1, dtype=torch.int32, device=DEV)
    stats = O._adam_call(p, g, m, v, lr, step, oc.BETAS, oc.EPS, st["max_norm"] if max_norm == "case" else max_norm,
                         status)
    for a, i in zip(g, idx):
        same(a, st["g"][i])
    return dict(p=p, m=m, v=v, t=int(step.item()), stats=stats, status=int(status.item()))


@pytest.mark.parametrize("case", ["clipped", "t999", "many", "capped"])
def test_same_bits_twice_and_at_any_alignment(case):
    st = oc.make(case, device=DEV)
    first, again, shifted = _call(st), _call(st), _call(st, floats=1)
    _same_state(first, again, "two identical calls")
    same(first["stats"], again["stats"])
    _same_state(first, shifted, "every base one float past a 256-byte boundary")
    same(first["stats"], shifted["stats"])
    assert first["t"] == st["t"] + 1 and first["status"] == 0
    assert not torch.equal(first["p"][0], st["p"][0])


def test_noncontiguous_gradient_is_its_contiguous_copy():
    st = oc.make("clipped", device=DEV)
    pa, a = _instance(st)
    pb, b = _instance(st)
    for q in pb:
        wide = torch.full((2 * q.numel(),), float("nan"), device=DEV)
        wide[::2] = q.grad
        q.grad = wide[::2]
        assert not q.grad.is_contiguous() or q.numel() == 1
    a.step()
    b.step()
    _same_state(_state(pa, a), _state(pb, b))
    same(a.stats, b.stats)


def test_split_over_launches_is_the_packed_call():
    """More tensors than one table (two launches a pass) against the same elements packed into 8 tensors (one
    launch a pass): other chunks and another order of the fp64 sum, the same norm in fp32, so the same bits."""
    st = oc.make("many", device=DEV)
    assert len(oc.active(st)) > oc.TABLE
    split = _call(st)
    groups = [list(range(k, min(k + 5, len(st["p"])))) for k in range(0, len(st["p"]), 5)]
    packed_st = dict({key: [torch.cat([st[key][i] for i in grp]) for grp in groups] for key in "pgmv"}, t=st["t"],
                     max_norm=st["max_norm"])
    assert len(groups) <= oc.TABLE
    packed = _call(packed_st)
    same(split["stats"], packed["stats"])
    for key in "pmv":
        same(torch.cat(split[key]), torch.cat(packed[key]), key)


@pytest.mark.parametrize("case", ["unclipped", "zero"])
def test_coef_one_is_no_clip(case):
    st = oc.make(case, device=DEV)
    clip, none = _call(st), _call(st, max_norm=None)
    assert float(clip["stats"][1]) == 1.0 and float(none["stats"][1]) == 1.0
    _same_state(clip, none)


@pytest.mark.parametrize("case", ["nan", "inf"])
def test_nonfinite_norm_skips_the_update(case):
    st = oc.make(case, device=DEV)
    params, opt = _instance(st)
    twin_p, twin = _instance(st)
    before = _state(params, opt)
    opt.step()
    after = _state(params, opt)
    _same_state(before, after, "skipped: not a bit changes")
    assert after["t"] == st["t"] and int(opt.status.item()) & _lib.OPT_NONFINITE
    norm, coef, count, skipped = opt.stats.tolist()
    assert skipped == 1.0 and count == st["t"] and coef == 0.0 and not torch.isfinite(opt.stats[0])
    # the next call with finite gradients goes on from t: it is the first call of a twin that never saw the bad one
    for o, ps in ((opt, params), (twin, twin_p)):
        for q, g in zip(ps, st["g"]):
            q.grad = torch.nan_to_num(g, nan=0.25, posinf=0.5)
        o.step()
    _same_state(_state(params, opt), _state(twin_p, twin))
    assert int(opt.step_count.item()) == st["t"] + 1 and float(opt.stats[3]) == 0.0 and int(twin.status.item()) == 0
    same(opt.stats, twin.stats)


def test_frozen_parameter_is_left_out():
    st = oc.make("frozen", device=DEV)
    f = oc.CASES["frozen"]["frozen"]
    params, opt = _instance(st)
    opt.step()
    same(params[f], st["p"][f])
    same(opt.exp_avg[f], st["m"][f])
    same(opt.exp_avg_sq[f], st["v"][f])
    without = {key: [x for i, x in enumerate(st[key]) if i != f] for key in "pgmv"}
    ps, other = _instance(dict(without, t=st["t"], max_norm=st["max_norm"]))
    other.step()
    got, want = _state(params, opt), _state(ps, other)
    for key in "pmv":
        del got[key][f]
    _same_state(got, want)
    same(opt.stats, other.stats)


def test_captured_step_replays_like_eager_steps():
    st = oc.make("t999", device=DEV)
    params, opt = _instance(st)
    twin_p, twin = _instance(st)
    gen = torch.Generator(device=DEV).manual_seed(3)

    def new_grads(scale):
        for q, r in zip(params, twin_p):
            q.grad.copy_(scale * torch.randn(q.shape, device=DEV, generator=gen))      # in place: the graph's pointers
            r.grad.copy_(q.grad)

    opt.step()                                               # eager first: the code objects are loaded
    twin.step()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        opt.step()                                           # recorded, not run
    _same_state(_state(params, opt), _state(twin_p, twin), "capture runs nothing")
    for k, how in enumerate(["replay", "replay", "eager", "replay"]):
        new_grads(0.1 * (k + 1))
        for o in (opt, twin):
            o.lr.fill_(oc.LR * (1.0 - 0.2 * k))              # a schedule, in place
        graph.replay() if how == "replay" else opt.step()
        twin.step()
        _same_state(_state(params, opt), _state(twin_p, twin), (k, how))
        same(opt.stats, twin.stats)
    assert int(opt.step_count.item()) == st["t"] + 5


def test_chain_backward_then_step():
    """The n3 case of test_gpu_train_chain.py on a copy of its kernel modules:
    kernel backward, then ClippedAdam.step, against the fp64 chain's gradients
    through clipped_adam_ref. The chain's own tolerance, |g - g64| <= BOUND *
    row_scale, widens the p bound: with dg that tolerance, dnorm <= sqrt(sum
    dg^2), dcoef <= coef (dnorm / norm + 4 * 2^-24) when the clip can be active,
    d = coef dg + (|g64| + dg) dcoef + 2^-24 |g'|, and a first step from zero
    moments being p - lr g' / (|g'| + eps), whose slope in g' is at most eps /
    (max(|g'| - d, 0) + eps)^2 within d of g'."""
    import test_gpu_train_chain as tg
    c, r = tg._case("n3"), tg._ref("n3")
    mods = tc.copy_of(c["mods"], torch.float32, True)
    named = tc.named_params(mods)
    tg._run("n3", mods)                                      # leaves the kernel chain's gradients in .grad
    names = list(named)
    params = [named[n] for n in names]
    assert all(q.grad is not None for q in params)
    p0 = [q.detach().clone() for q in params]
    opt = ClippedAdam(params)
    assert opt.kernel
    opt.step()
    assert int(opt.status.item()) == 0 and int(opt.step_count.item()) == 1
    g64 = [r["g64"][n].to(DEV) for n in names]
    zeros = [torch.zeros_like(g) for g in g64]
    p64, m64, v64, _, stats = O.clipped_adam_ref([p.double() for p in p0], g64, zeros, zeros, 0, opt.lr, opt.betas,
                                                 opt.eps, opt.max_grad_norm)
    norm, coef = float(stats[0]), float(stats[1])
    dg = [tg.BOUND * r["scale"][n].to(DEV) for n in names]
    dnorm = float(sum((d * d).sum() for d in dg).sqrt()) + 2.0 ** -23 * norm
    clip_possible = norm + dnorm + 1e-6 >= opt.max_grad_norm
    dcoef = coef * (dnorm / norm + 4 * oc.U) if clip_possible else 0.0
    lr, eps = float(opt.lr.double()), opt.eps
    b1 = opt.betas[0]
    step_size = lr / (1.0 - b1)
    worst = 0.0
    for n, q, p_ref, g, d_g, v in zip(names, params, p64, g64, dg, v64):
        gc = g.abs() * coef
        d = coef * d_g + (g.abs() + d_g) * dcoef + oc.U * gc
        sm = (1.0 - b1) * gc
        denom = v.sqrt() / (1.0 - opt.betas[1]) ** 0.5 + eps
        bound = oc.U * p_ref.abs() + oc.KP * oc.U * step_size * sm / denom + \
            lr * d * eps / ((gc - d).clamp(min=0.0) + eps) ** 2
        err = (q.detach().double() - p_ref).abs()
        worst = max(worst, float((err / bound).max()))
        assert bool((err <= bound).all()), (n, float((err / bound).max()))
        assert float((q.detach() - p0[names.index(n)]).abs().max()) > 0, n
    print(f"n3 chain + step: largest |p - p64| / bound {worst:.3f}; norm {norm:.4f}, coef {coef:.6f}")
