"""Guard bands around the optimizer step: gsm_adam_step (include/gsm_optim.h)
through optim._adam_call: the five assertions of tests/guard.py.

Inputs under guard: every gradient (floats: NaN, then 1e30 around it), the
learning rate (floats) and the step word (0 / 100 around it), and the values
the parameters and moments start from. p, m and v are in-out: inside the call
they are copied into tensors allocated under guard (the patched
torch.empty_like) and those are stepped, so the bands around them, around a
tensor of one element among them, have to stay as they are (a), and their
bits must not depend on the fills (d), the prefill (e) or the guard (c). The
step word, the status word and stats are outputs of the same kind. The
workspace is allocated under guard by _adam_call at the queried size and is
exempt from (b) as a whole ("a header, then one fp64 partial per chunk": the
query bounds the chunks from above); what it held must not reach a result (e).

Layouts: `aligned`, and `offset`: every gradient 4 bytes past a 256-byte
boundary and every in-out tensor the elements [1:] of a guarded allocation of
one more (element 0 stays unwritten; the views are what is returned and held to
(b)). Cases of tests/optim_cases.py: clipped (the chunk and vector edges), nan
(the skipped update still writes stats), many (more tensors than one launch's
table, one of no elements) and capped (every workgroup loops)."""
import pytest
import torch

import guard as G
import optim_cases as oc
from gsmarl_amd import optim as O

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _under_guard(src, offset):
    """A copy of ``src`` in memory from torch.empty (guarded while run_case runs)."""
    if src.numel() == 0:
        return src.clone()
    buf = torch.empty(src.numel() + offset, dtype=src.dtype, device=src.device)
    out = buf[offset:]
    out.copy_(src)
    return out


@pytest.mark.parametrize("case,layout", [("clipped", "aligned"), ("clipped", "offset"), ("nan", "aligned"),
                                         ("many", "aligned"), ("many", "offset"), ("capped", "aligned")])
def test_adam_step(case, layout):
    st = oc.make(case, device=DEV)
    idx = oc.active(st)
    off = 1 if layout == "offset" else 0
    total = sum(st["p"][i].numel() for i in idx)
    seen = set()

    def call(lr, step, **t):
        p, m, v = ([_under_guard(t[f"{key}{i}"], off) for i in idx] for key in "pmv")
        g = [t[f"g{i}"] for i in idx]
        step_out, status = _under_guard(step, 0), torch.empty(1, dtype=torch.int32, device=DEV)
        status.zero_()
        stats = O._adam_call(p, g, m, v, lr, step_out, oc.BETAS, oc.EPS, st["max_norm"], status)
        seen.add(tuple(sorted({x.data_ptr() % 16 for x in p + g + m + v if x.numel()})))
        out = dict(stats=stats, step=step_out, status=status)
        for key, ts in (("p", p), ("m", m), ("v", v)):
            out.update({f"{key}{i}": x for i, x in zip(idx, ts)})
        return out

    ins = dict(lr=G.In(torch.full((1,), oc.LR, device=DEV), G.floats),
               step=G.In(torch.full((1,), st["t"], dtype=torch.int32, device=DEV), lambda f: G.counts(f, 100)))
    for key in "pgmv":
        for i in idx:
            x = st[key][i]
            ins[f"{key}{i}"] = G.In(x, G.floats, misalign=4 * off if key == "g" else 0) if x.numel() else x
    plain = G.run_case(call, ins, work=[(O.adam_work_floats(len(idx), total),)])
    assert seen == ({(0, 4), (4,)} if off else {(0,)})       # the plain call's gradients are the aligned ones
    skipped = oc.CASES[case]["want"] == "skip"
    assert int(plain["status"].item()) == (1 if skipped else 0) and float(plain["stats"][3]) == float(skipped)
    assert int(plain["step"].item()) == st["t"] + (0 if skipped else 1)
    changed = [not torch.equal(plain[f"p{i}"], st["p"][i]) for i in idx if st["p"][i].numel()]
    assert not any(changed) if skipped else all(changed)
