"""gsm_ppo_loss on the GPU (gsmarl_amd.loss.PPOLagrangianLoss): the loss, the
statistics and the row gradients against the fp64 restatement on the same fp32
inputs, then reproducibility, the gradient-free call, autograd, the status
word, the shape errors, capture, and the loss at the end of the kernel chain
of tests/train_chain.py.

Bound (that of test_gpu_critic.py and test_gpu_train_chain.py, 2e-5): for a
sum |x - x64| <= 2e-5 * (1 + sum_r |w_r term_r| / W); for a row gradient
|g - g64| <= 2e-5 * (w_r / W) * (1 + |d_r64|), d_r the derivative of the row's
own term. Rows within 1e-4 of a branch point of the loss in the fp64
restatement carry weight 0 in both (ppo_loss_cases.decide). The fp32 torch
restatement's error is printed beside the kernel's."""
import ctypes as C
import functools

import pytest
import torch

import ppo_loss_cases as pc
import train_chain as tc
from gsmarl_amd import LagrangeMultiplier, PPOLagrangianLoss, _lib
from gsmarl_amd import loss as L

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BOUND = 2e-5
F64 = torch.float64
COEF = (pc.COEF["clip"], pc.COEF["value_clip"], pc.COEF["ent_coef"], pc.COEF["value_coef"])
OUTPUTS = ("loss", "stats", "g_logp", "g_ent", "g_values")


def bits(t):
    return t.contiguous().view(torch.int32)


def same(a, b, what):
    assert a is not None and b is not None and a.shape == b.shape and a.dtype == b.dtype, what
    assert torch.equal(bits(a), bits(b)), what


@functools.lru_cache(maxsize=None)
def _ref(case):
    """What the fp64 restatement says of a case, computed once: the weight
    (the case's own without the undecided rows), loss, stats, the row
    gradients and the scales of the bound."""
    d = pc.inputs(case)
    weight, und, outside, clipped = pc.decide(d)
    assert und <= 0.01 and outside >= 0.10 and min(clipped) >= 1
    dd = {k: (v.to(DEV) if v is not None else None) for k, v in d.items()}
    weight = weight.to(DEV)
    t = [dd[k].double() for k in pc.TENSORS]
    lam = pc.LAM if t[2].shape[0] == 2 else None
    keep = {}
    loss, stats = L.ppo_loss_ref(*t, weight, dd["n_valid"], lam, keep=keep, **pc.COEF)
    g = L.ppo_loss_grads_ref(*t, weight, dd["n_valid"], lam, **pc.COEF)
    w, W = keep["w"], keep["W"]
    sum_scale = torch.cat([1 + (w * keep["terms"].abs()).sum((1, 2)) / W, W[None]])   # [7]: |W - W64| <= 2e-5 W
    c = w / W
    # g = c d: the bound 2e-5 c (1 + |d|) = 2e-5 (c + |g|)
    g_scale = [c + g[0].abs(), c + g[1].abs(), c[None] + g[2].abs()]
    weight = weight.float().contiguous()
    if dd["n_valid"] is not None:                    # past n_valid the weight is not looked at: NaN there too
        valid = torch.arange(w.shape[1], device=DEV)[None, :] < dd["n_valid"][:, None]
        weight = torch.where(valid, weight, torch.full((), float("nan"), device=DEV))
    return dict(dev=dd, weight=weight, lam=lam, loss=loss, stats=stats, g=g,
                sum_scale=sum_scale, g_scale=g_scale, off=w == 0)


def _lam_tensor(lam):
    return torch.full((1,), float(lam), device=DEV) if lam is not None else None


def _call(t, weight, n_valid, lam, grads=True, status=None):
    """One gsm_ppo_loss on the tensors as they are laid out; a dict of the outputs and the status."""
    status = torch.zeros(1, dtype=torch.int32, device=DEV) if status is None else status
    nv = n_valid.to(torch.int32).contiguous() if n_valid is not None else None
    out = L._ppo_loss_call(*t, weight, nv, _lam_tensor(lam), status, COEF, grads)
    return dict(zip(OUTPUTS, out), status=status)


def _inputs(case, layout="plain"):
    """The case's fp32 device tensors: as they are, as non-contiguous views
    (every second column of a wider buffer), or contiguous but one float past
    a 16-byte boundary."""
    r = _ref(case)
    t = [r["dev"][k] for k in pc.TENSORS]
    weight = r["weight"]
    if layout == "strided":
        def wide(x):
            buf = torch.full(x.shape[:-1] + (2 * x.shape[-1],), float("nan"), device=DEV)
            buf[..., ::2] = x
            v = buf[..., ::2]
            assert not v.is_contiguous()
            return v
        return [wide(x) for x in t], wide(weight)
    if layout == "offset":
        def shifted(x):
            buf = torch.empty(x.numel() + 8, device=DEV)
            assert buf.data_ptr() % 16 == 0
            v = buf[1:1 + x.numel()].view(x.shape)
            v.copy_(x)
            assert v.is_contiguous() and v.data_ptr() % 16 == 4
            return v
        return [shifted(x) for x in t], shifted(weight)
    return t, weight


def _check(case, out, what):
    """The outputs of one call against the fp64 restatement."""
    r = _ref(case)
    assert int(out["status"].item()) == 0, what
    # the fp32 torch restatement on the same inputs, for the printout
    t32 = [r["dev"][k] for k in pc.TENSORS]
    loss32, stats32 = L.ppo_loss_ref(*t32, r["weight"], r["dev"]["n_valid"], r["lam"], **pc.COEF)
    g32 = L.ppo_loss_grads_ref(*t32, r["weight"], r["dev"]["n_valid"], r["lam"], **pc.COEF)
    worst = []
    e_k = (out["stats"].double() - r["stats"]).abs() / r["sum_scale"]
    e_t = (stats32.double() - r["stats"]).abs() / r["sum_scale"]
    print(f"{what} stats err / scale: kernel {[f'{e:.2e}' for e in e_k.tolist()]}  "
          f"fp32 torch {[f'{e:.2e}' for e in e_t.tolist()]}")
    if float(e_k.max()) > BOUND:
        worst.append(("stats", e_k.tolist()))
    e_l = float((out["loss"].double()[0] - r["loss"]).abs() / r["sum_scale"][0])
    print(f"{what} loss err / scale: kernel {e_l:.2e}  fp32 torch "
          f"{float((loss32.double() - r['loss']).abs() / r['sum_scale'][0]):.2e}")
    if e_l > BOUND:
        worst.append(("loss", e_l))
    same(out["loss"].view(()), out["stats"][0], "loss is stats[0]")
    for name, g64, scale, gt in zip(OUTPUTS[2:], r["g"], r["g_scale"], g32):
        g = out[name]
        assert g.dtype == torch.float32 and g.shape == g64.shape and bool(torch.isfinite(g).all()), name
        off = r["off"].expand_as(g64)
        assert bool((g[off] == 0).all()), name                   # rows of weight 0: exactly 0.0
        on = ~off
        assert float(g64[on].abs().max()) > 0, name
        e_k = float(((g.double() - g64).abs()[on] / scale[on]).max())
        e_t = float(((gt.double() - g64).abs()[on] / scale[on]).max())
        print(f"{what} {name} err / row scale: kernel {e_k:.2e}  fp32 torch {e_t:.2e}")
        if e_k > BOUND:
            worst.append((name, e_k))
    assert not worst, (what, worst)


@pytest.mark.parametrize("case", list(pc.CASES))
def test_against_the_fp64_restatement(case):
    r = _ref(case)
    t, weight = _inputs(case)
    R = t[0].numel()
    assert all(x.is_contiguous() and x.data_ptr() % 16 == 0 for x in t + [weight])
    if case == "capped":                                         # the grid as built: every partial is written
        assert L.ppo_loss_work_floats(R) == pc.MAX_BLOCKS * L.N_STATS
        assert R // pc.ROWS_PER_THREAD > (2 * pc.MAX_BLOCKS - 1) * pc.THREADS
    if pc.CASES[case].get("ragged"):
        assert all(bool(torch.isnan(x[..., r["off"]]).all()) for x in t)
    out = _call(t, weight, r["dev"]["n_valid"], r["lam"])
    _check(case, out, case)


@pytest.mark.parametrize("layout", ["strided", "offset"])
@pytest.mark.parametrize("case", ["r768", "ragged24", "capped"])
def test_layouts(case, layout):
    """Non-contiguous views go through the module (made contiguous);
    pointers one float off a 16-byte boundary take the scalar loads. The sums
    are formed in the same order either way: the plain call's bits."""
    r = _ref(case)
    plain = _call(*_inputs(case), r["dev"]["n_valid"], r["lam"])
    t, weight = _inputs(case, layout)
    if layout == "offset":
        out = _call(t, weight, r["dev"]["n_valid"], r["lam"])
        assert all(g.data_ptr() % 16 == 0 for g in (out["g_logp"], out["g_ent"], out["g_values"]))
    else:
        mod = PPOLagrangianLoss(*COEF)
        with torch.no_grad():
            loss_ng = mod(*t, weight, r["dev"]["n_valid"], r["lam"])
        same(loss_ng, plain["loss"].view(()), "the module on non-contiguous views")
        # the wide buffers as leaves: the gradients come back through the views
        leaves = [x._base.detach().clone().requires_grad_() for x in t[:3]]
        loss = mod(*[x[..., ::2] for x in leaves], *t[3:], weight, r["dev"]["n_valid"], r["lam"])
        loss.backward()
        assert all(int(torch.count_nonzero(x.grad[..., 1::2])) == 0 for x in leaves)
        g = [x.grad[..., ::2].contiguous() for x in leaves]
        out = dict(loss=loss.detach().view(1), stats=mod.stats, g_logp=g[0], g_ent=g[1], g_values=g[2],
                   status=mod.status)
    _check(case, out, f"{case}/{layout}")
    for k in OUTPUTS:
        same(out[k], plain[k], f"{case}/{layout}: {k} has the plain call's bits")


@pytest.mark.parametrize("case", ["r771", "capped", "ragged24"])
def test_two_calls_give_the_same_bits_and_no_grad_call(case):
    r = _ref(case)
    t, weight = _inputs(case)
    a = _call(t, weight, r["dev"]["n_valid"], r["lam"])
    b = _call(t, weight, r["dev"]["n_valid"], r["lam"])
    for k in OUTPUTS:
        same(a[k], b[k], k)
    ng = _call(t, weight, r["dev"]["n_valid"], r["lam"], grads=False)
    assert ng["g_logp"] is None and ng["g_ent"] is None and ng["g_values"] is None
    same(ng["loss"], a["loss"], "loss without the gradients")
    same(ng["stats"], a["stats"], "stats without the gradients")
    assert int(ng["status"].item()) == 0
    mod = PPOLagrangianLoss(*COEF)
    with torch.no_grad():
        loss = mod(*t, weight, r["dev"]["n_valid"], r["lam"])
    assert loss.dim() == 0 and loss.grad_fn is None
    same(loss, a["loss"].view(()), "the module under no_grad")
    same(mod.stats, a["stats"], "the module's stats under no_grad")


def test_autograd_delivers_the_row_gradients():
    case = "ragged24"
    r = _ref(case)
    t, weight = _inputs(case)
    raw = _call(t, weight, r["dev"]["n_valid"], r["lam"])
    mod = PPOLagrangianLoss(*COEF)
    lam = LagrangeMultiplier(pc.LAM, lr=0.05, cost_limit=1.0).to(DEV)

    def run(factor):
        leaves = [x.detach().clone().requires_grad_() for x in t[:3]]
        loss = mod(*leaves, *t[3:], weight, r["dev"]["n_valid"], lam.lam)
        names = tc.graph_names(loss)
        assert any("PPOLoss" in n for n in names), sorted(names)
        assert loss.dim() == 0 and not mod.stats.requires_grad
        same(loss.detach(), raw["loss"].view(()), "loss")
        same(mod.stats, raw["stats"], "stats")
        (factor * loss).backward()
        assert int(mod.status.item()) == 0
        return [x.grad for x in leaves]

    for name, g, want in zip(OUTPUTS[2:], run(1.0), (raw["g_logp"], raw["g_ent"], raw["g_values"])):
        same(g, want, name)
    for name, g, want in zip(OUTPUTS[2:], run(3.0), (raw["g_logp"], raw["g_ent"], raw["g_values"])):
        same(g, 3.0 * want, "3 x " + name)
    # only the values want a gradient: the others get none
    v = t[2].detach().clone().requires_grad_()
    mod(t[0], t[1], v, *t[3:], weight, r["dev"]["n_valid"], pc.LAM).backward()
    same(v.grad, raw["g_values"], "g_values alone, the multiplier a float")
    # the fallback: fp64 inputs run the restatement
    loss64 = mod(*[x.double() for x in t], weight.double(), r["dev"]["n_valid"], pc.LAM)
    assert loss64.dtype == F64 and mod.status is None and abs(float(loss64) - float(r["loss"])) <= 1e-12


def test_status_word():
    case = "r771"
    r = _ref(case)
    t, weight = _inputs(case)
    base = _call(t, weight, None, r["lam"])
    assert int(base["status"].item()) == 0
    idx = (weight > 0).nonzero()
    on, other = idx[5], idx[-1]                                  # two weighted rows, in envs other than env 3
    assert int(on[0]) != 3 and int(other[0]) != 3
    # a NaN in a weighted row
    bad = [x.clone() for x in t]
    bad[0][on[0], on[1]] = float("nan")
    out = _call(bad, weight, None, r["lam"])
    assert int(out["status"].item()) == _lib.LOSS_NONFINITE
    assert bool(torch.isnan(out["loss"]).all())                  # it reaches the loss, as autograd's would
    # the same NaN in a row of weight 0 is not seen
    w0 = weight.clone()
    w0[on[0], on[1]] = 0.0
    out = _call(bad, w0, None, r["lam"])
    assert int(out["status"].item()) == 0 and bool(torch.isfinite(out["loss"]).all())
    want = _call(t, w0, None, r["lam"])
    for k in OUTPUTS:
        same(out[k], want[k], k)
    # n_valid = N + 1 (and -1): flagged and clamped
    B, N = weight.shape
    nv = torch.full((B,), N, dtype=torch.int32, device=DEV)
    full = _call(t, weight, nv, r["lam"])
    assert int(full["status"].item()) == 0
    for k in OUTPUTS:
        same(full[k], base[k], k)
    nv_bad = nv.clone()
    nv_bad[3] = N + 1
    out = _call(t, weight, nv_bad, r["lam"])
    assert int(out["status"].item()) == _lib.LOSS_BAD_COUNT
    for k in OUTPUTS:
        same(out[k], base[k], k)
    nv_bad[3], nv[3] = -1, 0
    out, want = _call(t, weight, nv_bad, r["lam"]), _call(t, weight, nv, r["lam"])
    assert int(out["status"].item()) == _lib.LOSS_BAD_COUNT and int(want["status"].item()) == 0
    for k in OUTPUTS:
        same(out[k], want[k], k)
    # a negative (an infinite, a NaN) weight: flagged and taken as 0
    for v in (-0.5, float("inf"), float("nan")):
        wb = weight.clone()
        wb[on[0], on[1]] = v
        out = _call(t, wb, None, r["lam"])
        assert int(out["status"].item()) == _lib.LOSS_BAD_WEIGHT, v
        want = _call(t, w0, None, r["lam"])
        for k in OUTPUTS:
            same(out[k], want[k], k)
    # the bits are OR-ed into what the caller left there
    st = torch.full((1,), 64, dtype=torch.int32, device=DEV)
    bad2 = [x.clone() for x in t]
    bad2[2][1, other[0], other[1]] = float("inf")
    _call(bad2, wb, nv_bad, r["lam"], status=st)
    assert int(st.item()) == 64 | _lib.LOSS_NONFINITE | _lib.LOSS_BAD_COUNT | _lib.LOSS_BAD_WEIGHT


def test_no_weighted_row_and_no_rows_give_zeros():
    r = _ref("r12")
    t, weight = _inputs("r12")
    for kw in (dict(weight=torch.zeros_like(weight), n_valid=None),
               dict(weight=weight, n_valid=torch.zeros(4, dtype=torch.int32, device=DEV))):
        nan_in = [torch.full_like(x, float("nan")) for x in t]   # nothing is weighted: nothing is read
        out = _call(nan_in, kw["weight"], kw["n_valid"], r["lam"])
        assert int(out["status"].item()) == 0
        for k in OUTPUTS:
            assert int(torch.count_nonzero(bits(out[k]))) == 0, k        # +0.0 everywhere
    empty = [x[..., :0, :].contiguous() for x in t]
    out = _call(empty, None, None, r["lam"])
    assert int(torch.count_nonzero(bits(out["loss"]))) == 0 and int(torch.count_nonzero(bits(out["stats"]))) == 0
    assert out["g_values"].shape == (2, 0, 3) and int(out["status"].item()) == 0


def test_shape_errors_return_einval_without_launching():
    lib = _lib.load()
    buf = torch.zeros(64, device=DEV)
    canary = buf.clone()
    p = C.c_void_p(buf.data_ptr())
    stream = C.c_void_p(torch.cuda.current_stream(DEV).cuda_stream)

    def call(n_envs=4, n_agents=3, n_out=2, mult=p):
        # every pointer is the one buffer: a launch would overwrite it
        return lib.gsm_ppo_loss(p, p, p, p, p, p, p, None, None, n_envs, n_agents, n_out, mult, 0.2, 0.2, 0.01, 1.0,
                                p, p, p, p, p, p, None, stream)

    for kw, word in ((dict(n_out=0), "n_out"), (dict(n_out=3), "n_out"), (dict(n_agents=0), "n_agents"),
                     (dict(n_envs=2 ** 31 // 3 + 1), "2^31"), (dict(n_envs=2 ** 40, n_agents=2 ** 20), "2^31"),
                     (dict(n_envs=-1), "n_envs"), (dict(mult=None), "multiplier")):
        assert call(**kw) == _lib.GSM_EINVAL, kw
        assert word in _lib.last_error(lib), (kw, _lib.last_error(lib))
    nf = C.c_int64()
    assert lib.gsm_ppo_loss_work_floats(-1, C.byref(nf)) == _lib.GSM_EINVAL
    assert lib.gsm_ppo_loss_work_floats(2 ** 31, C.byref(nf)) == _lib.GSM_EINVAL
    assert lib.gsm_ppo_loss_work_floats(12, None) == _lib.GSM_EINVAL
    torch.cuda.synchronize()
    assert torch.equal(buf, canary)
    with pytest.raises(ValueError):
        a, b = buf[:12].view(4, 3), buf[:24].view(2, 4, 3)
        PPOLagrangianLoss()(a, a, b, a, b, b, b)                 # two heads and no multiplier


def test_captured_call_reads_the_multiplier_when_it_runs():
    case = "r1026"
    r = _ref(case)
    t, weight = _inputs(case)
    lam = LagrangeMultiplier(pc.LAM, lr=0.5, cost_limit=1.0).to(DEV)
    status = torch.zeros(1, dtype=torch.int32, device=DEV)

    def call():
        return L._ppo_loss_call(*t, weight, None, lam.lam, status, COEF, True)

    eager_first = [x.clone() for x in call()]                    # warms the kernels too
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = call()
    graph.replay()
    first = [x.clone() for x in out]
    lam.update(2.5)                                              # in place: 0.5 -> 1.25
    graph.replay()
    second = [x.clone() for x in out]
    torch.cuda.synchronize()
    del graph
    assert abs(float(lam.lam) - 1.25) <= 1e-6
    eager_second = call()
    for k, a, b, c, d in zip(OUTPUTS, first, eager_first, second, eager_second):
        same(a, b, f"first replay: {k}")
        same(c, d, f"second replay: {k}")
    assert not torch.equal(bits(first[2]), bits(second[2]))      # g_logp depends on the multiplier
    same(first[3], second[3], "g_ent does not")
    assert int(status.item()) == 0


@pytest.mark.parametrize("case", ["n3", "mixed"])
def test_at_the_end_of_the_kernel_chain(case):
    """Kernel features -> ActorHead.evaluate and CriticHead (HIP forward and
    backward) -> PPOLagrangianLoss -> backward: every parameter gradient
    against the fp64 chain of test_gpu_train_chain.py, the loss against
    train_chain.ppo_loss on the same features."""
    import test_gpu_train_chain as chain
    c, r = chain._case(case), chain._ref(case)
    mods, data, graph = c["mods"], c["data"], c["graph"]
    weight = r["weight"]
    n_valid = data["n_valid"]
    assert (n_valid is not None) == (case == "mixed")
    tc.zero_grads(mods)
    feats = tc.loss_rows(mods, graph, c["form"])
    logp, ent = mods["actor"].evaluate(feats, data["actions"])
    v = mods["critic"](feats, n_valid, data["denorm"])
    mod = PPOLagrangianLoss(tc.CLIP, tc.VCLIP, tc.ENT_COEF, 1.0)
    loss = mod(logp, ent, v, data["logp_old"], data["adv"], data["v_old"], data["ret"],
               weight.to(DEV, torch.float32), n_valid, tc.COST_MULT)
    names = tc.graph_names(loss)
    for w in ("EnvConv", "ActorEval", "CriticEval", "PPOLoss"):
        assert any(w in n for n in names), (w, sorted(names))
    loss.backward()
    assert int(mod.status.item()) == 0
    assert int(mods["actor"].status.item()) == 0 and int(mods["critic"].status.item()) == 0
    gk = tc.grads_of(mods)
    assert set(gk) == set(r["g64"])
    worst = []
    for name, g64 in r["g64"].items():
        assert gk[name] is not None and bool(torch.isfinite(gk[name]).all()), name
        e = tc.nerr(gk[name], g64, r["scale"][name])
        print(f"{case} {name}: err / row_scale with the fused loss {e:.3e}")
        if e > BOUND:
            worst.append((name, e))
    assert not worst, worst
    # the loss value: the fp64 heads and the helper's loss on the same features
    ref = tc.copy_of(mods, F64, False)
    keep = {}
    with torch.no_grad():
        loss64 = tc.ppo_loss(ref, feats.detach().double(), tc.cast_data(data, F64), weight.to(DEV), keep)
    scale = 1 + float(keep["pol_rows"].abs().sum() + keep["val_rows"].abs().sum())
    err = abs(float(loss.detach()) - float(loss64)) / scale
    print(f"{case}: loss {float(loss.detach()):.7f}, fp64 {float(loss64):.7f}, err / scale {err:.2e}")
    assert err <= BOUND
    assert abs(float(mod.stats[7]) - float(weight.sum())) <= BOUND * float(weight.sum())
