"""Guard bands around the loss end of the chain: gsm_ppo_loss (through
loss._ppo_loss_call, and through PPOLagrangianLoss for non-contiguous views)
and gsm_gae (through GraphRolloutBuffer.compute_returns): the five assertions
of tests/guard.py.

PPO loss: ppo_loss_cases r768 (16-byte loads), r771 (scalar), ragged24
(n_valid, weights, NaN in the masked rows) and capped (every workgroup loops),
contiguous, `offset` (every input 4 bytes past a 256-byte boundary: the scalar
loads) and `strided` (every second column of a wider buffer, the columns
between them band; the module makes such views contiguous), with and without
gradients. Inputs under guard: the seven tensors and the weight (floats),
n_valid (0 / N), the multiplier. Outputs under guard through the wrapper's own
torch.empty: loss, stats, g_logp, g_ent, g_values and the workspace.

GAE: (N, B, T) = (3, 7, 1), (3, 101, 7), (3, 9, 11): the remainders of the
unroll by four and a partial workgroup, on a real buffer whose reward, cost
and done fields are arenas; slot 0 of reward, which the launch does not read,
is filled like the band before it; done holds 0 / 1 around it.

Exceptions of (b): none for the outputs. include/gsm.h: "A row with w_r == 0
... gets the gradient 0.0": masked rows are written. The loss workspace ("one
[8] partial per workgroup of a capped grid") is exempt from (b) as a whole: a
launch of fewer workgroups than the cap writes fewer partials. It has to be
allocated under guard, so (a) holds for it, and what it held before must not
reach an output (e)."""
import pytest
import torch

import guard as G
import ppo_loss_cases as pc
from gsmarl_amd import EnvConfig, GpuBatchEnv, GraphRolloutBuffer, PPOLagrangianLoss
from gsmarl_amd import loss as L
from test_gpu_ppo_loss import COEF, OUTPUTS, _ref

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NAMES = pc.TENSORS + ("weight",)


def _tensors(case):
    r = _ref(case)
    t = {k: r["dev"][k] for k in pc.TENSORS}
    t["weight"] = r["weight"]
    n_valid = r["dev"]["n_valid"]
    lam = torch.full((1,), float(r["lam"]), device=DEV) if r["lam"] is not None else None
    return t, n_valid, lam


def _common(n_valid, lam, N):
    return dict(n_valid=G.In(n_valid.to(torch.int32).contiguous(), lambda f: G.counts(f, N))
                if n_valid is not None else None,
                lam=G.In(lam, G.floats) if lam is not None else None)


@pytest.mark.parametrize("grads", [True, False], ids=["grads", "no-grads"])
@pytest.mark.parametrize("layout", ["contiguous", "offset"])
@pytest.mark.parametrize("case", ["r768", "r771", "ragged24", "capped"])
def test_ppo_loss(case, layout, grads):
    """gsm_ppo_loss on contiguous inputs, aligned and one float past the alignment."""
    t, n_valid, lam = _tensors(case)
    B, N = t["logp"].shape

    seen = set()

    def call(n_valid, lam, **t):
        status = torch.zeros(1, dtype=torch.int32, device=DEV)
        out = L._ppo_loss_call(*(t[k] for k in NAMES), n_valid, lam, status, COEF, grads)
        assert int(status.item()) == 0
        seen.add(tuple(t[k].data_ptr() % 16 for k in NAMES))
        return dict(zip(OUTPUTS, out))

    ins = {k: G.In(v, G.floats, misalign=4 if layout == "offset" else 0) for k, v in t.items()}
    plain = G.run_case(call, dict(ins, **_common(n_valid, lam, N)), work=[(L.ppo_loss_work_floats(B * N),)])
    assert (plain["g_logp"] is not None) == grads
    assert seen == ({(0,) * 8, (4,) * 8} if layout == "offset" else {(0,) * 8})     # the plain call is the aligned one


@pytest.mark.parametrize("grads", [True, False], ids=["grads", "no-grads"])
@pytest.mark.parametrize("case", ["r768", "r771", "ragged24", "capped"])
def test_ppo_loss_strided_views(case, grads):
    """The module on non-contiguous views: what lies between the columns is
    band (NaN, then 1e30), and the saved row gradients, which the module does
    not return, are held to (a), (b) and the same bits in both runs."""
    t, n_valid, lam = _tensors(case)
    B, N = t["logp"].shape

    def call(n_valid, lam, **t):
        mod = PPOLagrangianLoss(*COEF)
        assert not any(t[k].is_contiguous() for k in NAMES) or N == 1
        with torch.enable_grad() if grads else torch.no_grad():
            lead = [t[k].detach().requires_grad_(grads) for k in NAMES[:3]]
            loss = mod(*lead, *(t[k] for k in NAMES[3:7]), t["weight"], n_valid, lam)
        assert int(mod.status.item()) == 0 and (loss.grad_fn is not None) == grads
        return dict(loss=loss.detach().view(1), stats=mod.stats)

    def wide(x):
        if not x.is_contiguous():                    # the plain call: the same layout, NaN between the columns
            return x
        buf = torch.full(x.shape[:-1] + (2 * x.shape[-1],), float("nan"), device=DEV)
        buf[..., ::2] = x
        return buf[..., ::2]

    ins = {k: G.In(wide(v), G.floats, base_shape=v.shape[:-1] + (2 * v.shape[-1],), view=lambda b: b[..., ::2])
           for k, v in t.items()}
    G.run_case(call, dict(ins, **_common(n_valid, lam, N)), work=[(L.ppo_loss_work_floats(B * N),)])


@pytest.mark.parametrize("N,B,T", [(3, 7, 1), (3, 101, 7), (3, 9, 11)])
def test_gae(N, B, T):
    """gsm_gae on a GraphRolloutBuffer of a small env whose reward, cost and done fields are replaced by
    arenas. compute_returns reads slots 1..T of reward: slot 0 lies inside the field and is filled like the
    band in front of it, so a read before the first reward used shows as one before the tensor does."""
    env = GpuBatchEnv(EnvConfig(n_agents=N, n_envs=B, seed=8), DEV)
    buf = GraphRolloutBuffer(env, episode_length=T)
    gen = torch.Generator(device=DEV).manual_seed(T)
    stored = torch.zeros(T + 1, B, N, device=DEV)
    stored[1:] = torch.randn(T, B, N, device=DEV, generator=gen)
    values = torch.randn(T + 1, B, N, device=DEV, generator=gen)
    done = (torch.rand(T + 1, B, device=DEV, generator=gen) < 0.3).to(torch.uint8)
    done[T, 0], done[T, B - 1] = 1, 0

    def call(used, values, done, kernel=True):
        field = used.as_strided((T + 1, B, N), (B * N, N, 1), used.storage_offset() - B * N)
        assert field.shape == buf.reward.shape and done.shape == buf.done.shape
        buf.reward, buf.cost, buf.done = field, field, done
        return {which: buf.compute_returns(values, 0.99, 0.95, which=which, kernel=kernel)
                for which in ("reward", "cost")}

    ins = dict(used=G.In(stored[1:], G.floats, base_shape=(T + 1, B, N), view=lambda t: t[1:]),
               values=G.In(values, G.floats), done=G.In(done, G.flags))
    plain = G.run_case(call, ins)
    ref = call(stored[1:], values, done, kernel=False)
    assert all(G.same_bits(plain[k], ref[k]) for k in ref)       # the torch loop, as test_gpu_gae.py holds it
    env.close()
