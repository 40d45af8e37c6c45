"""The optimizer step on the CPU: clipped_adam_ref (gsmarl_amd/optim.py), the
torch restatement of gsm_adam_step, held to torch's own clip_grad_norm_ + Adam
in fp64; its fp32 form measured against its fp64 form in the scales of
tests/optim_cases.py (these ratios set Km, Kv, Kp of test_gpu_optim.py); the
committed cases held to what each has to show; ClippedAdam's fallback and its
state_dict; and include/gsm_optim.h held to _lib.OPTIM_SIGNATURES, libgsm.so
and the guard file, as test_abi.py and test_guard_ref.py hold include/gsm.h."""
import ctypes as C
import re
import subprocess
from pathlib import Path

import pytest
import torch

import optim_cases as oc
from gsmarl_amd import ClippedAdam, _lib
from gsmarl_amd.optim import clipped_adam_ref

ROOT = Path(__file__).resolve().parents[1]
HEADER = ROOT / "include" / "gsm_optim.h"


@pytest.mark.parametrize("case", ["clipped", "unclipped", "noclip"])
def test_fp64_restatement_is_torch_clip_and_adam(case):
    """10 steps on the 13 tensors, gradients redrawn every step: to 1e-12 relative."""
    st = oc.make(case, torch.float64)
    st["t"] = 0                                              # torch's Adam starts its own count at 0
    params = [torch.nn.Parameter(p.clone()) for p in st["p"]]
    opt = torch.optim.Adam(params, lr=oc.LR, betas=oc.BETAS, eps=oc.EPS)
    p, m, v = st["p"], [torch.zeros_like(x) for x in st["p"]], [torch.zeros_like(x) for x in st["p"]]
    gen = torch.Generator().manual_seed(5)
    coefs = []
    for k in range(10):
        grads = [g * (0.5 + torch.rand(g.shape, generator=gen, dtype=torch.float64)) for g in st["g"]]
        for q, g in zip(params, grads):
            q.grad = g.clone()
        if st["max_norm"] is not None:
            torch.nn.utils.clip_grad_norm_(params, st["max_norm"])
        opt.step()
        p, m, v, step, stats = clipped_adam_ref(p, grads, m, v, k, oc.LR, oc.BETAS, oc.EPS, st["max_norm"])
        coefs.append(float(stats[1]))
        assert int(step) == k + 1
        for i, q in enumerate(params):
            s = opt.state[q]
            for got, want in ((p[i], q.detach()), (m[i], s["exp_avg"]), (v[i], s["exp_avg_sq"])):
                assert float((got - want).abs().max()) <= 1e-12 * float(want.abs().max()), (k, i)
    assert all(c < 1 for c in coefs) if case == "clipped" else all(c == 1.0 for c in coefs)


def test_fp32_restatement_against_fp64_sets_the_bounds():
    """The fp32 restatement against the fp64 one from the same fp32 state, five
    steps a case: the largest ratios, printed, times 4 and rounded up to a
    power of two, are Km, Kv, Kp."""
    worst = [0.0, 0.0, 0.0]
    for case in oc.PARITY:
        st = oc.make(case)
        for k in range(5):
            r32 = oc.ref_step(st, torch.float32)
            rm, rv, rp, r64 = oc.ratios(st, r32)
            worst = [max(a, b) for a, b in zip(worst, (rm, rv, rp))]
            assert abs(float(r32["stats"][0]) - float(r64["stats"][0])) <= 2.0 ** -23 * float(r64["stats"][0])
            for j, i in enumerate(oc.active(st)):             # go on from the fp32 form's own state
                st["p"][i], st["m"][i], st["v"][i] = r32["p"][j], r32["m"][j], r32["v"][j]
            st["t"] += 1
        print(f"{case}: fp32 restatement, largest ratios so far m {worst[0]:.2f} v {worst[1]:.2f} p {worst[2]:.2f}")
    assert all(w > 0 for w in worst)
    assert [oc.pow2_above(4 * w) for w in worst] == [oc.KM, oc.KV, oc.KP], worst


@pytest.mark.parametrize("case", list(oc.CASES))
def test_every_case_shows_what_it_is_for(case):
    c, st = oc.CASES[case], oc.make(case)
    r32, r64 = oc.ref_step(st, torch.float32), oc.ref_step(st, torch.float64)
    idx = oc.active(st)
    for r in (r32, r64):
        norm, coef, step, skipped = (float(x) for x in r["stats"])
        if c["want"] == "skip":
            assert skipped == 1.0 and coef == 0.0 and step == st["t"] and int(r["step"]) == st["t"]
            assert not torch.isfinite(r["stats"][0])
            for k, i in enumerate(idx):                      # nothing changes by a bit
                assert all(torch.equal(r[key][k], st[key][i].to(r[key][k].dtype)) for key in "pmv")
            continue
        assert skipped == 0.0 and step == st["t"] + 1 and torch.isfinite(r["stats"]).all()
        assert all(bool(torch.isfinite(x).all()) for key in "pmv" for x in r[key])
        if c["want"] == "clip":
            assert coef < 1.0 and norm > st["max_norm"]
        if c["want"] == "one":
            assert coef == 1.0
            assert all(torch.equal(st["g"][i].to(r["stats"].dtype) * r["stats"][1], st["g"][i].to(r["stats"].dtype))
                       for i in idx)
        if c["want"] == "zero":
            assert norm == 0.0 and coef == 1.0
            assert all(torch.equal(r["p"][k], st["p"][i].to(r["p"][k].dtype)) for k, i in enumerate(idx))
    if case == "huge":                                       # the squares overflow fp32, their fp64 sum does not
        assert all(bool(torch.isinf(st["g"][i] * st["g"][i]).all()) for i in idx)
    if case == "frozen":
        assert len(idx) == len(st["p"]) - 1
    if case == "many":
        assert len(idx) > oc.TABLE and 0 in [x.numel() for x in st["p"]]
    if case == "capped":
        assert sum(-(-x.numel() // oc.CHUNK) for x in st["p"]) > oc.CAP


def _instance(st, dtype, **kw):
    params = [torch.nn.Parameter(p.to(dtype).clone()) for p in st["p"]]
    opt = ClippedAdam(params, lr=oc.LR, betas=oc.BETAS, eps=oc.EPS, max_grad_norm=st["max_norm"], **kw)
    for dst, src in zip(opt.exp_avg + opt.exp_avg_sq, st["m"] + st["v"]):
        dst.copy_(src.to(dtype))
    opt.step_count.fill_(st["t"])
    for q, g in zip(params, st["g"]):
        q.grad = g.to(dtype).clone() if g is not None else None
    return params, opt


@pytest.mark.parametrize("case", ["clipped", "noclip", "frozen", "nan", "many"])
def test_module_on_cpu_fp64_is_the_restatement(case):
    st = oc.make(case)
    params, opt = _instance(st, torch.float64)
    assert not opt.kernel and opt.lr.dtype == torch.float32 and opt.step_count.dtype == torch.int32
    before = [g.clone() if g is not None else None for g in (q.grad for q in params)]
    opt.step()
    ref = oc.ref_step(st, torch.float64, opt.lr)
    idx = oc.active(st)
    for k, i in enumerate(idx):
        assert torch.equal(params[i].detach(), ref["p"][k]) and torch.equal(opt.exp_avg[i], ref["m"][k])
        assert torch.equal(opt.exp_avg_sq[i], ref["v"][k])
        assert torch.equal(params[i].grad.view(torch.int64), before[i].view(torch.int64))    # never written
    for i in set(range(len(params))) - set(idx):             # the frozen one, bit for bit
        assert torch.equal(params[i].detach(), st["p"][i].double()) and torch.equal(opt.exp_avg[i], st["m"][i].double())
        assert torch.equal(opt.exp_avg_sq[i], st["v"][i].double())
    assert int(opt.step_count) == int(ref["step"])
    assert torch.equal(opt.stats.view(torch.int64), ref["stats"].view(torch.int64))     # by bits: the norm may be NaN
    opt.zero_grad()
    assert all(q.grad is None for q in params)
    opt.step()                                               # no gradient anywhere: not an update
    assert int(opt.step_count) == int(ref["step"])


def test_constructor_checks():
    p = torch.nn.Parameter(torch.zeros(3))
    with pytest.raises(ValueError, match="twice"):
        ClippedAdam([p, p])
    with pytest.raises(ValueError):
        ClippedAdam([])
    opt = ClippedAdam([p])
    assert float(opt.lr) == pytest.approx(7e-4) and opt.betas == (0.9, 0.999) and opt.eps == 1e-5
    assert opt.max_grad_norm == 10.0
    p.grad = torch.ones(3)
    opt.zero_grad(set_to_none=False)
    assert p.grad is not None and not p.grad.any()


def test_state_dict_round_trip_is_bit_identical():
    st = oc.make("t999")
    params, opt = _instance(st, torch.float32)
    opt.step()
    opt.lr.mul_(0.5)                                         # a schedule wrote the rate in place
    state = opt.state_dict()
    twins = [torch.nn.Parameter(q.detach().clone()) for q in params]
    new = ClippedAdam(twins, lr=1.0, betas=(0.5, 0.5), eps=1.0, max_grad_norm=None)
    new.load_state_dict(state)
    for o, qs in ((opt, params), (new, twins)):
        for q, g in zip(qs, st["g"]):
            q.grad = (g * 0.75).clone()
        o.step()
    assert torch.equal(new.step_count, opt.step_count) and int(new.step_count) == 1001
    assert torch.equal(new.stats, opt.stats) and torch.equal(new.lr, opt.lr)
    for a, b in zip(twins + new.exp_avg + new.exp_avg_sq, params + opt.exp_avg + opt.exp_avg_sq):
        assert torch.equal(a.detach(), b.detach())
    state["exp_avg"][0].add_(1.0)                            # the dict holds copies
    assert not torch.equal(state["exp_avg"][0], opt.exp_avg[0])


# ---- include/gsm_optim.h: what test_abi.py and test_guard_ref.py keep for include/gsm.h ------------
def declared_functions():
    return sorted(set(re.findall(r"^\s*(?:int|const char \*)\s+(gsm_\w+)\s*\(", HEADER.read_text(), re.M)))


@pytest.fixture(scope="module")
def lib():
    if not _lib.LIB_PATH.exists():
        import __graft_entry__ as g
        g.build()
    return _lib.load()


def test_header_binding_library_and_guard_file_agree(lib):
    names = declared_functions()
    assert set(names) == set(_lib.OPTIM_SIGNATURES) == {"gsm_adam_step", "gsm_adam_work_floats"}
    assert not set(names) & set(_lib.SIGNATURES)
    assert _lib.ABI_VERSION == 8 and "gsm_adam" not in (ROOT / "include" / "gsm.h").read_text()
    out = subprocess.run(["nm", "-D", "--defined-only", str(_lib.LIB_PATH)], capture_output=True, text=True,
                         check=True).stdout
    exported = set(re.findall(r" T (gsm_\w+)", out))
    for name in names:
        assert name in exported and getattr(lib, name).argtypes == _lib.OPTIM_SIGNATURES[name][1], name
    assert int(re.search(r"#define GSM_OPT_NONFINITE (\d+)", HEADER.read_text()).group(1)) == _lib.OPT_NONFINITE
    # the entry point that launches has a guarded case that names it; the other launches nothing
    text = (ROOT / "tests" / "test_gpu_guard_optim.py").read_text()
    assert re.search(r"^def test_adam_step\(", text, re.M) and "gsm_adam_step" in text


def test_header_compiles_as_c(tmp_path):
    probe = tmp_path / "probe.c"
    probe.write_text('#include "gsm_optim.h"\nint main(void){ return GSM_OPT_NONFINITE == 1 ? 0 : 1; }\n')
    subprocess.run(["gcc", "-fsyntax-only", "-I", str(ROOT / "include"), str(probe)], check=True)


def test_work_floats_and_argument_checks_launch_nothing(lib):
    """gsm_adam_work_floats is a host query; gsm_adam_step rejects bad arguments before any launch (no GPU here)."""
    nf = C.c_int64()
    assert lib.gsm_adam_work_floats(0, 0, C.byref(nf)) == _lib.GSM_OK and nf.value >= 4 and nf.value % 2 == 0
    sizes = [x for x in oc.MANY]
    assert lib.gsm_adam_work_floats(len(sizes), sum(sizes), C.byref(nf)) == _lib.GSM_OK
    chunks = sum(-(-n // oc.CHUNK) for n in sizes)
    assert nf.value >= 2 * chunks + 4                        # a header and one double per chunk
    assert lib.gsm_adam_work_floats(-1, 0, C.byref(nf)) == _lib.GSM_EINVAL
    assert lib.gsm_adam_work_floats(1, 1, None) == _lib.GSM_EINVAL
    a = C.c_void_p(4096)
    ptrs, n = (C.c_void_p * 1)(4096), (C.c_int64 * 1)(8)
    ok = dict(p=ptrs, g=ptrs, m=ptrs, v=ptrs, n=n, k=1, lr=a, step=a, b1=0.9, b2=0.999, eps=1e-5, mx=10.0, work=a,
              stats=a)
    bad = [dict(k=-1), dict(n=(C.c_int64 * 1)(1 << 31)), dict(n=(C.c_int64 * 1)(-1)), dict(g=(C.c_void_p * 1)(None)),
           dict(b1=1.0), dict(b2=-0.1), dict(eps=-1.0), dict(mx=-1.0), dict(mx=float("nan")), dict(lr=None),
           dict(step=None), dict(work=None), dict(stats=None), dict(work=C.c_void_p(4100)), dict(p=None)]
    for change in bad:
        x = dict(ok, **change)
        rc = lib.gsm_adam_step(x["p"], x["g"], x["m"], x["v"], x["n"], x["k"], x["lr"], x["step"], x["b1"], x["b2"],
                               x["eps"], x["mx"], x["work"], x["stats"], None, None)
        assert rc == _lib.GSM_EINVAL, change
        assert _lib.last_error(lib)
