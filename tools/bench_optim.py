"""Measure the optimizer step (gsmarl_amd.optim.ClippedAdam: gsm_adam_step,
two launches) against torch's clip_grad_norm_ + Adam, in one process on one
GPU.

Parameter sets: `chain` = the modules of the two-layer training chain as
tests/train_chain.py builds them (conv 7 -> 3 x 16, conv2 48 -> 3 x 16, actor
(48, 64, 5), critic (48, 64, 2): 26 tensors), and `wide` = the same with every
hidden width 256 (4 x 64 channels, heads of 256). Forms:
  fused          ClippedAdam.step()
  foreach        clip_grad_norm_(foreach=True) + Adam(foreach=True).step()
  torch_fused    clip_grad_norm_(foreach=True) + Adam(fused=True).step()
  capturable     clip_grad_norm_(foreach=True) + Adam(foreach=True, capturable=True).step()
Gradients are drawn once with a norm below max_norm, so torch's in-place
rescaling multiplies by 1 and a thousand calls see the same gradients. Before
timing, one step of every form from the same state is compared with the fused
one. Timing: torch.cuda events around REPS calls after 3 warm-up calls, three
alternating repeats (fused, foreach, ..., fused, ...). One JSON line per set,
written to profiles/optim.json (or $OPTIM_OUT).

Launch counts come from runs of their own under the profiler:
  rocprofv3 --kernel-trace --stats -d DIR/<form>_<N> -o run --output-format csv -- \\
      python tools/bench_optim.py --trace <form> --calls <N>
for two values of N; `--launches DIR` takes the difference of the kernel
calls, per call, and writes `launches_per_call` into the JSON lines."""
import argparse
import csv
import inspect
import json
import os
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "gs-marl_amd"))
import torch  # noqa: E402

from gsmarl_amd import ActorHead, ClippedAdam, CriticHead  # noqa: E402
from gsmarl_amd.gnn import TransformerConv  # noqa: E402

DEV = "cuda:0"
REPS = int(os.environ.get("OPTIM_REPS", 1000))
LR, BETAS, EPS, MAX_NORM = 7e-4, (0.9, 0.999), 1e-5, 10.0
SETS = {"chain": dict(heads=3, channels=16, hidden=64), "wide": dict(heads=4, channels=64, hidden=256)}
FORMS = ["fused", "foreach", "torch_fused", "capturable"]
OUT = Path(os.environ.get("OPTIM_OUT") or ROOT / "profiles" / "optim.json")


def parameters(which, seed=0):
    s = SETS[which]
    hc = s["heads"] * s["channels"]
    torch.manual_seed(seed)
    mods = [TransformerConv(7, s["channels"], heads=s["heads"], use_kernel=False),
            TransformerConv(hc, s["channels"], heads=s["heads"], use_kernel=False),
            ActorHead(hc, s["hidden"], 5, use_kernel=False), CriticHead(hc, s["hidden"], 2, use_kernel=False)]
    params = [p for m in mods for p in m.to(DEV).parameters()]
    gen = torch.Generator(device=DEV).manual_seed(seed + 1)
    n = sum(p.numel() for p in params)
    for p in params:                                          # a norm of about 1: below MAX_NORM, coef == 1
        p.grad = torch.randn(p.shape, device=DEV, generator=gen) / n ** 0.5
    return params


def make_form(form, which):
    """(params, step function) of one form on fresh copies of the set's parameters and gradients."""
    params = parameters(which)
    if form == "fused":
        opt = ClippedAdam(params, lr=LR, betas=BETAS, eps=EPS, max_grad_norm=MAX_NORM)
        assert opt.kernel
        return params, opt.step
    kw = dict(foreach=dict(foreach=True), torch_fused=dict(fused=True),
              capturable=dict(foreach=True, capturable=True))[form]
    if not all(k in inspect.signature(torch.optim.Adam).parameters for k in kw):
        return params, None
    opt = torch.optim.Adam(params, lr=LR, betas=BETAS, eps=EPS, **kw)

    def step():
        torch.nn.utils.clip_grad_norm_(params, MAX_NORM, foreach=True)
        opt.step()
    return params, step


def timed(fn, reps):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps * 1e3          # microseconds a call


def case(which):
    forms = {f: make_form(f, which) for f in FORMS}
    forms = {f: v for f, v in forms.items() if v[1] is not None}
    # the same result first: one step of every form from the same state (fp32 against fp32)
    for params, step in forms.values():
        step()
    torch.cuda.synchronize()
    ref = forms["fused"][0]
    diff = {}
    for f, (params, _) in forms.items():
        if f != "fused":
            diff[f] = max(float(((a - b).abs() / (LR + a.abs() * 2.0 ** -20)).max()) for a, b in zip(ref, params))
    assert max(diff.values()) <= 1e-3, diff                  # of one step's size lr (an Adam step moves p by <= ~lr)
    times = {f: [] for f in forms}
    for _ in range(3):
        for f, (_, step) in forms.items():
            times[f].append(round(timed(step, REPS), 1))
    med = {f: sorted(v)[1] for f, v in times.items()}
    best = min((f for f in med if f != "fused"), key=med.get)
    n = [p.numel() for p in ref]
    return {"op": "ClippedAdam.step (gsm_adam_step) against clip_grad_norm_ + torch.optim.Adam", "set": which,
            "tensors": len(n), "elements": sum(n), "us": times, "median_us": med, "best_torch_form": best,
            "torch_best_over_fused": round(med[best] / med["fused"], 2),
            "fused_faster_beyond_spread": max(times["fused"]) < min(times[best]),
            "max_diff_after_one_step_in_units_of_lr": diff, "torch": torch.__version__,
            "launches_per_call": "not measured",
            "timing": f"torch.cuda events around {REPS} calls after 3 warm-up calls, three alternating repeats, one "
                      "stream, one process; the host's part of a call included"}


def trace(form, calls):
    _, step = make_form(form, "chain")
    if step is None:
        raise SystemExit(f"{form}: not in this torch build")
    for _ in range(calls):
        step()
    torch.cuda.synchronize()


def launches(src):
    """{form: kernel launches a call} from DIR/<form>_<N>/**/*kernel_stats.csv at two N."""
    out = {}
    for form in FORMS:
        runs = {}
        for d in Path(src).glob(f"{form}_*"):
            files = sorted(d.rglob("*kernel_stats.csv"))
            if files:
                with open(files[0]) as f:
                    runs[int(d.name.rsplit("_", 1)[1])] = sum(int(r["Calls"]) for r in csv.DictReader(f))
        if len(runs) >= 2:
            lo, hi = min(runs), max(runs)
            out[form] = round((runs[hi] - runs[lo]) / (hi - lo), 2)
    return out


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--trace", choices=FORMS)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--launches")
    a = ap.parse_args()
    if a.trace:
        trace(a.trace, a.calls)
    elif a.launches:
        counts = launches(a.launches)
        lines = [json.loads(l) for l in OUT.read_text().splitlines() if l]
        for line in lines:
            if line["set"] == "chain" and counts:
                line["launches_per_call"] = counts
        OUT.write_text("\n".join(json.dumps(l) for l in lines) + "\n")
        print(counts)
    else:
        lines = []
        for which in SETS:
            lines.append(json.dumps(case(which)))
            print(lines[-1], flush=True)
        OUT.parent.mkdir(parents=True, exist_ok=True)
        OUT.write_text("\n".join(lines) + "\n")
