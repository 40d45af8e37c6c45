"""CPU checks of the PPO / Lagrangian loss's definition (gsmarl_amd.loss): the
torch restatement against the loss of tests/train_chain.py, the written-out
gradients against autograd, masked rows, the share conditions of the synthetic
inputs test_gpu_ppo_loss.py runs the kernel on, and LagrangeMultiplier."""
import functools

import pytest
import torch

import ppo_loss_cases as pc
import train_chain as tc
from gsmarl_amd import LagrangeMultiplier, PPOLagrangianLoss
from gsmarl_amd import loss as L

T = 4
F64 = torch.float64


@functools.lru_cache(maxsize=None)
def _chain():
    """Case n3 of the training-step tests on oracle graphs: the fp64 chain's
    loss with what it keeps, and the same loss's inputs."""
    kind, N, B, form = "n3", 3, 20, "env1"
    seed = tc.SEEDS[kind]
    slots, rew, cost, done = tc.oracle_graph(B, N, T, seed)
    graph = tc.env_graph(slots, N, slots[0]["node_feat"].shape[1], T)
    mods = tc.build(kind, 1, torch.float32, False)
    gae = {"reward": tc.gae_ref(rew, done), "cost": tc.gae_ref(cost, done)}
    data = tc.rollout_data(mods, tc.cast_graph(graph, torch.float32), form, gae, seed)
    ref = tc.copy_of(mods, F64, False)
    weight = tc.decide(ref, graph, form, data)[0]
    d64 = tc.cast_data(data, F64)
    keep = {}
    with torch.no_grad():
        feats = tc.loss_rows(ref, tc.cast_graph(graph, F64), form)
        loss = tc.ppo_loss(ref, feats, d64, weight, keep)
    return dict(loss=loss, keep=keep, data=d64, weight=weight)


def _case64(case):
    d = pc.inputs(case)
    t = [d[k].double() for k in pc.TENSORS]
    lam = pc.LAM if t[2].shape[0] == 2 else None
    return d, t, lam


def test_restatement_is_the_helpers_loss():
    c = _chain()
    k, d = c["keep"], c["data"]
    assert float(c["weight"].sum()) > 0 and bool((c["weight"] == 0).any())
    keep = {}
    loss, stats = L.ppo_loss_ref(k["logp"], k["ent"], k["v"], d["logp_old"], d["adv"], d["v_old"], d["ret"],
                                 c["weight"], None, tc.COST_MULT, tc.CLIP, tc.VCLIP, tc.ENT_COEF, 1.0, keep=keep)
    assert abs(float(loss) - float(c["loss"])) <= 1e-12
    assert float((keep["pol_rows"] - k["pol_rows"]).abs().max()) <= 1e-12
    assert float((keep["val_rows"] - k["val_rows"]).abs().max()) <= 1e-12
    assert abs(float(stats[0]) - float(loss)) <= 1e-12 and float(stats[7]) == float(c["weight"].sum())
    # the module off the GPU is the restatement
    mod = PPOLagrangianLoss(tc.CLIP, tc.VCLIP, tc.ENT_COEF, 1.0)
    got = mod(k["logp"], k["ent"], k["v"], d["logp_old"], d["adv"], d["v_old"], d["ret"], c["weight"], None,
              tc.COST_MULT)
    assert got.dim() == 0 and float(got) == float(loss) and mod.status is None
    assert torch.equal(mod.stats, stats)


def test_stats_are_the_weighted_means():
    d, t, lam = _case64("ragged24")
    keep = {}
    loss, stats = L.ppo_loss_ref(*t, d["weight"], d["n_valid"], lam, keep=keep, **pc.COEF)
    w, W = keep["w"], keep["W"]
    assert stats.shape == (8,) and bool(torch.isfinite(stats).all()) and float(W) > 0
    for i in range(7):
        assert abs(float((w * keep["terms"][i]).sum() / W) - float(stats[i])) <= 1e-12, i
    assert float(stats[7]) == float(W) and 0.0 < float(stats[6]) < 1.0
    c = pc.COEF
    assert abs(float(stats[1] - c["ent_coef"] * stats[2] + c["value_coef"] * (stats[3] + stats[4])) -
               float(loss)) <= 1e-12


@pytest.mark.parametrize("case", ["r771", "ragged24", "nout1"])
def test_written_out_gradients_against_autograd(case):
    d, t, lam = _case64(case)
    weight = pc.decide(d)[0]
    leaves = [x.clone().requires_grad_() for x in t[:3]]
    loss, _ = L.ppo_loss_ref(*leaves, *t[3:], weight, d["n_valid"], lam, **pc.COEF)
    auto = torch.autograd.grad(loss, leaves)
    ours = L.ppo_loss_grads_ref(*t, weight, d["n_valid"], lam, **pc.COEF)
    for name, a, o in zip(("g_logp", "g_ent", "g_values"), auto, ours):
        assert a.shape == o.shape and bool(torch.isfinite(a).all()), name
        assert float(a.abs().max()) > 0 and float((a - o).abs().max()) <= 1e-12, name
        assert bool((a[..., weight == 0] == 0).all()) and bool((o[..., weight == 0] == 0).all()), name


def test_masked_rows_take_no_part():
    d, t, lam = _case64("ragged24")
    w = pc.decide(d)[0]
    off = w == 0
    assert bool(off.any()) and all(bool(torch.isnan(x[..., off]).all()) for x in t)
    assert bool(torch.isnan(d["weight"]).any())             # past n_valid the weight itself is NaN
    loss, stats = L.ppo_loss_ref(*t, w, d["n_valid"], lam, **pc.COEF)
    clean = [torch.where(off, torch.full((), 7.0, dtype=F64), x) for x in t]
    loss_c, stats_c = L.ppo_loss_ref(*clean, w, d["n_valid"], lam, **pc.COEF)
    assert bool(torch.isfinite(loss)) and float(loss) == float(loss_c) and torch.equal(stats, stats_c)
    for g, g_c in zip(L.ppo_loss_grads_ref(*t, w, d["n_valid"], lam, **pc.COEF),
                      L.ppo_loss_grads_ref(*clean, w, d["n_valid"], lam, **pc.COEF)):
        assert torch.equal(g, g_c) and bool((g[..., off] == 0).all())
    # weight and n_valid multiply: the same loss from the product given as the weight alone
    N = w.shape[1]
    valid = torch.arange(N)[None, :] < d["n_valid"][:, None]
    w_raw = torch.where(valid, d["weight"].double(), torch.zeros((), dtype=F64))
    both, _ = L.ppo_loss_ref(*t, w_raw, d["n_valid"], lam, **pc.COEF)
    alone, _ = L.ppo_loss_ref(*t, w_raw * valid, None, lam, **pc.COEF)
    assert float(both) == float(alone)
    dense, _ = L.ppo_loss_ref(*clean, torch.ones_like(w), d["n_valid"], lam, **pc.COEF)
    assert float(dense) != float(both)                      # the weight does count
    # n_valid is clamped to [0, N]
    wide = torch.where(d["n_valid"] == N, d["n_valid"] + 5, d["n_valid"])
    wide = torch.where(wide == 0, wide - 3, wide)
    assert float(L.ppo_loss_ref(*t, w, wide, lam, **pc.COEF)[0]) == float(loss)


def test_no_weighted_row_gives_zeros():
    d, t, lam = _case64("r12")
    leaves = [x.clone().requires_grad_() for x in t[:3]]
    for kw in (dict(weight=torch.zeros(4, 3, dtype=F64)), dict(n_valid=torch.zeros(4, dtype=torch.int32))):
        loss, stats = L.ppo_loss_ref(*leaves, *t[3:], multiplier=lam, **kw, **pc.COEF)
        assert float(loss.detach()) == 0.0 and bool((stats == 0).all())
        assert all(bool((g == 0).all()) for g in torch.autograd.grad(loss, leaves))
        assert all(bool((g == 0).all()) for g in L.ppo_loss_grads_ref(*t, multiplier=lam, **kw, **pc.COEF))
    # a negative or non-finite weight counts as 0
    bad = torch.ones(4, 3, dtype=F64)
    bad[0, 0], bad[1, 1], bad[2, 2] = -1.0, float("inf"), float("nan")
    zero = torch.where((bad == 1), bad, torch.zeros((), dtype=F64))
    assert float(L.ppo_loss_ref(*t, bad, None, lam, **pc.COEF)[0]) == float(L.ppo_loss_ref(*t, zero, None, lam,
                                                                                          **pc.COEF)[0])


def test_one_head():
    d, t, lam = _case64("nout1")
    assert t[2].shape[0] == 1 and lam is None
    keep = {}
    loss, stats = L.ppo_loss_ref(*t, keep=keep, **pc.COEF)
    assert torch.equal(keep["A"], t[4][0]) and float(stats[4]) == 0.0 and float(stats[3]) > 0
    two = [x if x.dim() == 2 else torch.cat([x, torch.zeros_like(x)]) for x in t]
    loss2, _ = L.ppo_loss_ref(*two, multiplier=0.0, **pc.COEF)   # a cost head of zeros adds nothing
    assert abs(float(loss) - float(loss2)) <= 1e-12
    with pytest.raises(ValueError):
        L.ppo_loss_ref(*two, **pc.COEF)                          # two heads need a multiplier
    assert float(PPOLagrangianLoss(**{"entropy_coef" if k == "ent_coef" else k: v for k, v in pc.COEF.items()})(
        *t)) == float(loss)


@pytest.mark.parametrize("case", list(pc.CASES))
def test_share_conditions_of_the_synthetic_inputs(case):
    d = pc.inputs(case)
    weight, und, outside, clipped = pc.decide(d)
    print(f"{case}: undecided {und:.4%}, outside the clip range {outside:.2%}, clipped value rows {clipped}")
    assert float(weight.sum()) > 0
    assert und <= 0.01
    assert outside >= 0.10
    assert len(clipped) == d["values"].shape[0] and min(clipped) >= 1
    if pc.CASES[case].get("ragged"):
        assert set(weight.unique().tolist()) == {0.0, 0.5, 1.0}
        assert int(d["n_valid"].min()) == 0 and int(d["n_valid"].max()) == pc.CASES[case]["N"]


def test_capped_case_is_past_one_pass_of_the_grid():
    R = pc.CASES["capped"]["B"] * 3
    items = R // pc.ROWS_PER_THREAD
    assert R % 4 == 0 and R == pc.B_CAPPED * 3
    assert items > (2 * pc.MAX_BLOCKS - 1) * pc.THREADS          # the last workgroup takes a second item
    assert items <= 2 * pc.MAX_BLOCKS * pc.THREADS


def test_lagrange_multiplier_update():
    m = LagrangeMultiplier(0.5, lr=0.1, cost_limit=1.0)
    assert m.lam.dtype == torch.float32 and m.lam.shape == (1,) and "lam" in dict(m.named_buffers())
    ptr = m.lam.data_ptr()
    m.update(3.0)                                   # over the limit: up
    assert abs(float(m.lam) - 0.7) <= 1e-6
    m.update(torch.tensor(0.0))                     # under it: down
    assert abs(float(m.lam) - 0.6) <= 1e-6
    m.update(-100.0)                                # floored at 0
    assert float(m.lam) == 0.0
    m.update(1.0)                                   # at the limit: unchanged
    assert float(m.lam) == 0.0 and m.lam.data_ptr() == ptr       # in place
    with pytest.raises(TypeError):
        LagrangeMultiplier(0.0)                     # lr and cost_limit are required
