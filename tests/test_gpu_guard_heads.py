"""Guard bands around the MLP heads (gsm_actor_sample, gsm_actor_eval,
gsm_actor_eval_bwd, gsm_critic_eval, gsm_critic_eval_bwd) through
policy.ActorHead and policy.CriticHead: the five assertions of tests/guard.py
on the HEADS lists of test_gpu_actor.py and test_gpu_critic.py (the head of 52
features reads a strided x: rows of 64 floats, the 12 between them band).

Shapes (B, N): (7, 3), one tile of 21 rows; (171, 24), 4104 rows = 32 tiles of
128 and one of 8; for the critic also (5, 96) (one env a tile) and (300, 1)
(the cap of 64 envs a tile, a last partial tile).

Inputs under guard: x, the four weight tensors, grad outputs, denorm (floats),
the stored actions (0 / A-1), n_valid (0 / N), the draw counter. Outputs under
guard through the wrappers' own torch.empty: actions, logp, entropy, logits,
values, dw1, db1, dw2, db2, dx and the workspaces.

Exceptions of (b): none for the outputs. include/gsm.h: rows i >= n_valid[b]
"get 0.0 in every head" and "(padded rows: dx = 0)": padded rows are written.
The workspaces (gsm_actor_backward_work_floats, gsm_critic_backward_work_floats:
"one partial per workgroup of a capped grid") are exempt from (b) as a whole: a
launch of fewer workgroups than the cap writes fewer partials. They have to be
allocated under guard, so (a) holds for them, and what they held before must
not reach an output (e)."""
import pytest
import torch

import guard as G
import test_gpu_actor as ta
import test_gpu_critic as tcr
from gsmarl_amd import ActorHead, CriticHead, _lib

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
A_SHAPES = [(7, 3), (171, 24)]
C_SHAPES = [(7, 3), (171, 24), (5, 96), (300, 1)]
W = ("w1", "b1", "w2", "b2")


def _x_in(x):
    """x under guard in the layout it has: contiguous, or a view of rows of 64 floats."""
    if x.is_contiguous():
        return G.In(x, G.floats)
    B, N, F = x.shape
    assert x.stride() == (N * 64, 64, 1)
    return G.In(x, G.floats, base_shape=(B, N, 64), view=lambda t: t[:, :, :F])


def _weights_in(head):
    return {n: (G.In(t.detach(), G.floats) if t is not None else None) for n, t in zip(W, head._weights())}


def _with(head, w1, b1, w2, b2):
    """``head`` reading its parameters from the given tensors (no copies)."""
    if head.lin1 is not None:
        head.lin1.weight, head.lin1.bias = torch.nn.Parameter(w1), torch.nn.Parameter(b1)
    head.lin2.weight, head.lin2.bias = torch.nn.Parameter(w2), torch.nn.Parameter(b2)
    assert [p.data_ptr() for p in head._weights() if p is not None] == \
        [t.data_ptr() for t in (w1, b1, w2, b2) if t is not None]
    return head


def _rand(shape, seed):
    return torch.randn(shape, device=DEV, generator=torch.Generator(device=DEV).manual_seed(seed))


@pytest.mark.parametrize("B,N", A_SHAPES)
@pytest.mark.parametrize("F,hidden,A", ta.HEADS, ids=ta.ids_h)
def test_actor_sample(F, hidden, A, B, N):
    """gsm_actor_sample with the entropy and the logits, the draw number in a device counter."""
    head, x = ta.make_head(F, hidden, A), ta.make_x(B, N, F)
    counter = torch.tensor([3], dtype=torch.int64, device=DEV)

    def call(x, w1, b1, w2, b2, counter):
        h = _with(ActorHead(F, hidden, A), w1, b1, w2, b2)
        out = h.act(x, ta.SEED, env_base=5, draw=96, draw_counter=counter, entropy=True, logits=True)
        assert int(h.status.item()) == 0
        return dict(zip(("actions", "logp", "entropy", "logits"), out))

    ins = dict(x=_x_in(x), **_weights_in(head), counter=G.In(counter, lambda f: G.counts(f, 5)))
    plain = G.run_case(call, ins)
    assert int(plain["actions"].min()) >= 0 and int(plain["actions"].max()) < A

    def bare(x, w1, b1, w2, b2, counter):                    # entropy and logits_out NULL, deterministic
        h = _with(ActorHead(F, hidden, A), w1, b1, w2, b2)
        return dict(zip(("actions", "logp"), h.act(x, ta.SEED, draw_counter=counter, deterministic=True)))

    first = (plain["logits"] == plain["logits"].max(-1, keepdim=True)[0]).int().argmax(-1)
    assert torch.equal(G.run_case(bare, ins)["actions"].long(), first)


@pytest.mark.parametrize("want_dx", [True, False], ids=["dx", "no-dx"])
@pytest.mark.parametrize("B,N", A_SHAPES)
@pytest.mark.parametrize("F,hidden,A", ta.HEADS, ids=ta.ids_h)
def test_actor_eval_and_backward(F, hidden, A, B, N, want_dx):
    """gsm_actor_eval and gsm_actor_eval_bwd (the training path of evaluate)."""
    head, x = ta.make_head(F, hidden, A), ta.make_x(B, N, F)
    acts = torch.randint(0, A, (B, N), device=DEV, dtype=torch.int32,
                         generator=torch.Generator(device=DEV).manual_seed(5))
    g_logp, g_ent = _rand((B, N), 6), _rand((B, N), 7)

    def call(x, w1, b1, w2, b2, acts, g_logp, g_ent):
        h = _with(ActorHead(F, hidden, A, kernel_backward=True), w1, b1, w2, b2)
        xl = x.detach().requires_grad_(want_dx)
        logp, ent = h.evaluate(xl, acts)
        names = [n for n, t in zip(W, (w1, b1, w2, b2)) if t is not None]
        leaves = [p for p in h._weights() if p is not None]
        grads = torch.autograd.grad([logp, ent], leaves + ([xl] if want_dx else []), [g_logp, g_ent])
        assert int(h.status.item()) == 0
        out = dict(logp=logp.detach(), entropy=ent.detach(), **{"d" + n: t for n, t in zip(names, grads)})
        if want_dx:
            out["dx"] = grads[-1]
        return out

    ins = dict(x=_x_in(x), **_weights_in(head), acts=G.In(acts, lambda f: G.actions(f, A)),
               g_logp=G.In(g_logp, G.floats), g_ent=G.In(g_ent, G.floats))
    work = (_lib.work_floats("gsm_actor_backward_work_floats", F, hidden, A),)
    plain = G.run_case(call, ins, work=[work])
    assert ("dx" in plain) == want_dx and ("dw1" in plain) == (hidden != 0)


def _ragged(x, B, N):
    n_valid = tcr.make_counts(B, N)
    xr = x.clone() if x.is_contiguous() else x.contiguous()
    xr[torch.arange(N, device=DEV)[None, :] >= n_valid[:, None]] = float("nan")     # padded rows are not read
    if not x.is_contiguous():
        wide = torch.full((B, N, 64), float("nan"), device=DEV)
        wide[:, :, :x.shape[2]] = xr
        xr = wide[:, :, :x.shape[2]]
    return xr, n_valid


@pytest.mark.parametrize("B,N", C_SHAPES)
@pytest.mark.parametrize("F,hidden,O", tcr.HEADS, ids=tcr.ids_h)
def test_critic_eval(F, hidden, O, B, N):
    """gsm_critic_eval: dense and raw, then ragged with NaN in the padded rows and denormalised."""
    head, x = tcr.make_head(F, hidden, O), tcr.make_x(B, N, F)
    xr, n_valid = _ragged(x, B, N)
    st = torch.tensor([[0.5, 3.0], [-2.0, 0.25]], device=DEV)[:O].contiguous()

    def call(x, w1, b1, w2, b2, n_valid, denorm):
        h = _with(CriticHead(F, hidden, O), w1, b1, w2, b2)
        v = tcr.fwd(h, x, n_valid, denorm)
        assert int(h.status.item()) == 0
        return dict(values=v)

    G.run_case(call, dict(x=_x_in(x), **_weights_in(head), n_valid=None, denorm=None))
    plain = G.run_case(call, dict(x=_x_in(xr), **_weights_in(head), n_valid=G.In(n_valid, lambda f: G.counts(f, N)),
                                  denorm=G.In(st, G.floats)))
    pad = torch.arange(N, device=DEV)[None, :] >= n_valid[:, None]
    assert bool((plain["values"].view(torch.int32)[:, pad] == 0).all())


@pytest.mark.parametrize("F,hidden,A", [(48, 64, 5), (4, 0, 2)], ids=["in48-h64-a5", "in4-h0-a2"])
def test_actor_backward_without_entropy_gradient(F, hidden, A):
    """gsm_actor_eval_bwd with g_ent = NULL ("or NULL (zeros)"). ActorHead always passes an entropy
    gradient, so this one is called through _lib, as test_gpu_actor._bwd calls it, its outputs and its
    workspace from torch.empty under guard."""
    B, N = 171, 24
    head, x = ta.make_head(F, hidden, A), ta.make_x(B, N, F)
    acts = torch.randint(0, A, (B, N), device=DEV, dtype=torch.int32,
                         generator=torch.Generator(device=DEV).manual_seed(5))
    g_logp = _rand((B, N), 6)
    lib, P = _lib.load(), _lib.ptr
    n_work = _lib.work_floats("gsm_actor_backward_work_floats", F, hidden, A)

    def run(g_ent):
        def call(x, w1, b1, w2, b2, acts, g_logp):
            work = torch.empty(n_work, dtype=torch.float32, device=DEV)
            dw = [torch.empty_like(t) if t is not None else None for t in (w1, b1, w2, b2)]
            dx = torch.empty(B, N, F, dtype=torch.float32, device=DEV)
            rc = lib.gsm_actor_eval_bwd(P(g_logp), P(g_ent), P(x), F, P(w1), P(b1), P(w2), P(b2), B, N, F, hidden, A,
                                        P(acts), P(work), *(P(t) for t in dw), P(dx), None, _lib.stream(x.device))
            _lib.check(lib, rc, None, "gsm_actor_eval_bwd")
            return dict(zip(("dw1", "db1", "dw2", "db2"), dw), dx=dx)
        return call

    ins = dict(x=_x_in(x), **_weights_in(head), acts=G.In(acts, lambda f: G.actions(f, A)),
               g_logp=G.In(g_logp, G.floats))
    plain = G.run_case(run(None), ins, work=[(n_work,)])
    zeros = G.run_case(run(torch.zeros(B, N, device=DEV)), ins, work=[(n_work,)])
    assert all(zeros[k] is None or torch.allclose(plain[k], zeros[k], atol=1e-6) for k in plain)


@pytest.mark.parametrize("want_dx", [True, False], ids=["dx", "no-dx"])
@pytest.mark.parametrize("ragged", [False, True], ids=["dense", "ragged"])
@pytest.mark.parametrize("B,N", C_SHAPES)
@pytest.mark.parametrize("F,hidden,O", tcr.HEADS, ids=tcr.ids_h)
def test_critic_backward(F, hidden, O, B, N, ragged, want_dx):
    """gsm_critic_eval_bwd behind the training path of forward, with and without dx, dense and with ragged
    n_valid."""
    head, x = tcr.make_head(F, hidden, O), tcr.make_x(B, N, F)
    n_valid = None
    if ragged:
        x, n_valid = _ragged(x, B, N)
    g_v = _rand((O, B, N), 7)

    def call(x, w1, b1, w2, b2, n_valid, g_v):
        h = _with(CriticHead(F, hidden, O, kernel_backward=True), w1, b1, w2, b2)
        xl = x.detach().requires_grad_(want_dx)
        v = h(xl, n_valid)
        grads = torch.autograd.grad(v, list(h._weights()) + ([xl] if want_dx else []), g_v)
        assert int(h.status.item()) == 0
        return dict(values=v.detach(), **{"d" + n: t for n, t in zip(W + ("x",), grads)})

    ins = dict(x=_x_in(x), **_weights_in(head), g_v=G.In(g_v, G.floats),
               n_valid=G.In(n_valid, lambda f: G.counts(f, N)) if ragged else None)
    work = (_lib.work_floats("gsm_critic_backward_work_floats", F, hidden, O),)
    plain = G.run_case(call, ins, work=[work])
    assert ("dx" in plain) == want_dx
    if ragged and want_dx:
        pad = torch.arange(N, device=DEV)[None, :] >= n_valid[:, None]
        assert bool((plain["dx"].view(torch.int32)[pad] == 0).all())
