"""One whole PPO update's backward on the kernel path, stage joined to stage:
rollout buffer slots (or a graph_batch_csr minibatch) -> gsm_env_conv_fwd/_bwd
and gsm_attn_aggregate_fwd/_bwd -> gsm_actor_eval/_bwd and gsm_critic_eval/_bwd
-> the clipped PPO / Lagrangian loss of tests/train_chain.py, every parameter
gradient against fp64 autograd of the same chain in the torch formulations.

Forms of the chain (train_chain.features):
  env1  forward_env(slot, rows="agents") per stored slot, joined by torch.cat;
        the loss reads the slice [:T*B] (the last slot only feeds the returns)
  env2  forward_env(rows="all", row_ptr=True) -> relu -> conv2.forward on the
        env's own edges -> .view(B, E, -1)[:, :N], per slot, joined by torch.cat
  csr2  both layers through TransformerConv.forward on one graph_batch_csr
        minibatch with its transpose -> .view(K, E, -1)[:, :N]

Bound (that of test_gpu_actor.py, test_gpu_critic.py and
test_gpu_env_conv_backward.py at row granularity): for every parameter tensor
max |g - g64| / row_scale <= 2e-5, row_scale = 1 + sum over the loss rows of
|the fp64 gradient of that row's weighted term alone| (train_chain.row_scales).
Rows within 1e-4 of a branch point of the loss in the fp64 chain carry weight 0
in every chain (train_chain.undecided). The fp32 torch chain's error is printed
beside the kernel chain's; with GSM_TRAIN_CHAIN_JSON set both are written there
(profiles/train_chain_grad.json is such a run). The wiring between the stages
and the exact properties of the step are compared bit for bit."""
import functools
import json
import os

import pytest
import torch

import train_chain as tc
from gsmarl_amd import EnvConfig, GpuBatchEnv, GraphRolloutBuffer, gnn, policy
from test_gpu_actor import _bwd as actor_bwd
from test_gpu_critic import _bwd as critic_bwd

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BOUND = 2e-5
T = 4
CASES = {
    "n3": dict(N=3, B=20, form="env1", cfg=dict(episode_length=2)),         # E = 9; done flags inside the window
    "n6-env2": dict(N=6, B=12, form="env2"),
    "n6-csr2": dict(N=6, B=12, form="csr2"),
    "n24": dict(N=24, B=3, form="env1"),                                    # E = 72: rows longer than a wave
    "mixed": dict(N=12, B=24, form="env1", cfg=dict(scenario="mixed")),     # ragged: n_valid, padded agents
}
# the minibatch of n6-csr2: K = 17, slots 0 and T, (2, 7) drawn twice; the first 8 and the last 9 are disjoint
CSR_T = [0, 0, 1, 1, 2, 3, 3, 4, 4, 0, 1, 2, 3, 4, 2, 2, 2]
CSR_B = [0, 5, 1, 6, 2, 3, 8, 4, 9, 10, 11, 0, 1, 2, 7, 3, 7]
KERNEL_NODES = ("EnvConv", "AttnAggregate", "ActorEval", "CriticEval")
RESULTS = {}


def bits(t):
    return t.contiguous().view(torch.int32)


def same(a, b, what):
    assert a is not None and b is not None and a.shape == b.shape and a.dtype == b.dtype, what
    assert torch.equal(bits(a), bits(b)), what


def _csr_graph(c, t_idx, b_idx):
    batch = c["buf"].graph_batch_csr(torch.tensor(t_idx), torch.tensor(b_idx))
    assert int(batch["status"].item()) == 0
    return dict(N=c["N"], E=c["E"], slots=c["slots"], rows=len(t_idx), batch=batch, n_valid=None,
                samples=(c["slots"], list(t_idx), list(b_idx)))


@functools.lru_cache(maxsize=None)
def _case(case):
    """The buffer, the graph, the kernel modules and the data of a case: built
    once and left unchanged."""
    spec, seed = CASES[case], tc.SEEDS[case]
    N, B, form = spec["N"], spec["B"], spec["form"]
    env = GpuBatchEnv(EnvConfig(n_envs=B, n_agents=N, seed=seed, **spec.get("cfg", {})), DEV)
    buf = GraphRolloutBuffer(env, episode_length=T)
    buf.reset(seed=seed)
    gen = torch.Generator(device=DEV).manual_seed(seed)
    for _ in range(T):
        buf.insert(torch.randint(0, 5, (B, N), dtype=torch.int32, device=DEV, generator=gen))
    torch.cuda.synchronize()
    assert not bool(buf.overflowed())
    slots = [{k: buf.slot(t)[k] for k in ("node_feat", "edge_ptr", "edge_index", "edge_attr")} for t in range(T + 1)]
    c = dict(case=case, N=N, B=B, E=env.E, form=form, env=env, buf=buf, slots=slots, seed=seed)
    if form == "csr2":
        graph = _csr_graph(c, CSR_T, CSR_B)
    else:
        graph = tc.env_graph(slots, N, env.E, T)
    if env.cfg.ragged:
        nv = env.outputs(sync_edges=False)["n_agents_env"].to(torch.int32).clone()
        assert int(nv.min()) < N and int(nv.max()) <= N                     # there are padded agents
        graph.update(n_valid_env=nv, n_valid=nv.repeat(T))
    if "episode_length" in spec.get("cfg", {}):
        assert bool(buf.done[1:T].any())                                    # an episode ends inside the window
    mods = tc.build(case, 1 if form == "env1" else 2, torch.float32, True, DEV)
    gae = {w: (lambda v, w=w: buf.compute_returns(v, which=w, kernel=True)) for w in ("reward", "cost")}
    data = tc.rollout_data(mods, graph, form, gae, seed)
    c.update(graph=graph, mods=mods, gae=gae, data=data)
    return c


@functools.lru_cache(maxsize=None)
def _ref(case):
    """What the fp64 chain says of a case: the weight (valid and decided
    rows), its gradients and the row scales; computed once."""
    c = _case(case)
    ref = tc.copy_of(c["mods"], torch.float64, False)
    weight, und, outside, clipped = tc.decide(ref, c["graph"], c["form"], c["data"])
    print(f"{case}: undecided {und:.4%}, outside the clip range {outside:.2%}, clipped value rows {clipped}")
    assert und <= 0.01 and outside >= 0.10 and clipped >= 1
    g64, _ = tc.run(ref, tc.cast_graph(c["graph"], torch.float64), c["form"], tc.cast_data(c["data"], torch.float64),
                    weight)
    scale = tc.row_scales(ref, c["graph"], c["data"], weight)
    return dict(weight=weight, g64=g64, scale=scale)


def _run(case, mods=None, **kw):
    c = _case(case)
    weight = kw.pop("weight", None)
    weight = _ref(case)["weight"] if weight is None else weight
    return tc.run(mods if mods is not None else c["mods"], kw.pop("graph", c["graph"]), c["form"],
                  kw.pop("data", c["data"]), weight, **kw)


def _on_kernel_path(case, keep, mods):
    names = tc.graph_names(keep["loss"])
    want = {"env1": ("EnvConv",), "env2": ("EnvConv", "AttnAggregate"), "csr2": ("AttnAggregate",)}[CASES[case]["form"]]
    for w in want + ("ActorEval", "CriticEval"):
        assert any(w in n for n in names), (w, sorted(names))
    assert int(mods["actor"].status.item()) == 0 and int(mods["critic"].status.item()) == 0


@pytest.mark.parametrize("case", list(CASES))
def test_gradients_against_fp64_autograd(case):
    c, r = _case(case), _ref(case)
    gk, keep = _run(case)
    _on_kernel_path(case, keep, c["mods"])              # the status words after the backward kernels too
    t32 = tc.copy_of(c["mods"], torch.float32, False)
    gt, keep_t = _run(case, t32)
    assert not any(w in n for n in tc.graph_names(keep_t["loss"]) for w in KERNEL_NODES)
    assert set(gk) == set(r["g64"]) == set(r["scale"])
    res, worst = {}, []
    for name, g64 in r["g64"].items():
        assert gk[name] is not None and gk[name].dtype == torch.float32 and bool(torch.isfinite(gk[name]).all()), name
        assert float(g64.abs().max()) > 0, name
        e_k, e_t = tc.nerr(gk[name], g64, r["scale"][name]), tc.nerr(gt[name], g64, r["scale"][name])
        print(f"{case} {name}: err / row_scale  kernel chain {e_k:.3e}  fp32 torch chain {e_t:.3e}")
        res[name] = dict(kernel=e_k, torch_fp32=e_t)
        if e_k > BOUND:
            worst.append((name, e_k))
    RESULTS[case] = res
    out = os.environ.get("GSM_TRAIN_CHAIN_JSON")
    if out:
        with open(out, "w") as f:
            json.dump(RESULTS, f, indent=1, sort_keys=True)
    assert not worst, worst


def _forward_with_hooks(case):
    """The kernel chain's forward with hooks on feats, logp, ent, v, the
    per-slot features and the first layer's outputs; ``cap`` fills in backward."""
    c = _case(case)
    mods = c["mods"]
    tc.zero_grads(mods)
    keep, cap = {}, {}
    feats = tc.loss_rows(mods, c["graph"], c["form"], keep)
    loss = tc.ppo_loss(mods, feats, c["data"], _ref(case)["weight"], keep)

    def hook(name, t):
        t.register_hook(lambda g: cap.__setitem__(name, g.detach().clone()))
    hook("feats", feats)
    for k in ("logp", "ent", "v"):
        hook(k, keep[k])
    for k in ("slot_feats", "h"):
        for t, x in enumerate(keep.get(k, [])):
            hook((k, t), x)
    keep["feats"] = feats
    return mods, keep, cap, loss


@pytest.mark.parametrize("case", ["n6-env2", "mixed"])
def test_wiring_between_the_stages_bit_for_bit(case):
    c = _case(case)
    mods, keep, cap, loss = _forward_with_hooks(case)
    loss.backward()
    got = tc.grads_of(mods)
    data, feats = c["data"], keep["feats"].detach()
    n_valid = data["n_valid"]
    # the heads' own backward kernels on the upstream gradients the loss produced
    dw1, db1, dw2, db2, dx_a, st = actor_bwd(mods["actor"], feats, data["actions"], cap["logp"].contiguous(),
                                             cap["ent"].contiguous())
    assert int(st.item()) == 0
    g_v = cap["v"]
    if n_valid is not None:                              # the torch tail of CriticHead.forward, backwards
        g_v = torch.where(policy._critic_mask(feats, n_valid)[None], g_v, torch.zeros((), device=DEV))
    g_raw = (g_v * data["denorm"][:, 1, None, None]).contiguous()
    cr = critic_bwd(mods["critic"], feats, g_raw, n_valid)
    assert int(cr["status"].item()) == 0
    same(cap["feats"], dx_a + cr["dx"], "the gradient the heads send down = dx_actor + dx_critic")
    for name, want in (("actor.lin1.weight", dw1), ("actor.lin1.bias", db1), ("actor.lin2.weight", dw2),
                       ("actor.lin2.bias", db2), ("critic.lin1.weight", cr["dw1"]), ("critic.lin1.bias", cr["db1"]),
                       ("critic.lin2.weight", cr["dw2"]), ("critic.lin2.bias", cr["db2"])):
        same(got[name], want, name)
    # the first layer: env_conv_autograd on each slot with the gradient that reached it, split by
    # autograd through pack_conv_params; autograd runs the later slots first
    conv, N, E = mods["conv"], c["N"], c["E"]
    key, R = ("slot_feats", N) if c["form"] == "env1" else ("h", E)
    for p in conv.parameters():
        p.grad = None
    for t in reversed(range(T + 1)):
        s = c["graph"]["slots"][t]
        w, w_e = gnn.pack_conv_params(conv)
        out = gnn.env_conv_autograd(s["node_feat"].contiguous(), s["edge_ptr"], s["edge_index"], s["edge_attr"], w, w_e,
                                    conv.heads, R, True)
        same(out.detach(), keep[key][t].detach(), f"slot {t}: the forward")
        g = cap[(key, t)]
        assert g.shape == out.shape
        if t == T:
            assert int(torch.count_nonzero(g)) == 0      # the last slot is outside the loss rows
        else:
            assert float(g.abs().sum()) > 0
        out.backward(g)
    for n, p in conv.named_parameters():
        same(p.grad, got["conv." + n], "conv." + n)


@pytest.mark.parametrize("case", list(CASES))
def test_backward_is_reproducible(case):
    first, _ = _run(case)
    again, _ = _run(case)
    for name, g in first.items():
        same(again[name], g, name)


def test_gradients_accumulate_over_two_minibatches():
    c = _case("n6-csr2")
    mods = c["mods"]
    parts = []
    for lo, hi in ((0, 8), (8, 17)):
        graph = _csr_graph(c, CSR_T[lo:hi], CSR_B[lo:hi])
        data = tc.rollout_data(mods, graph, "csr2", c["gae"], c["seed"] + lo)
        weight = tc.base_weight(data["logp_old"][..., None])
        g, _ = tc.run(mods, graph, "csr2", data, weight)
        parts.append((graph, data, weight, g))
    assert not set(zip(CSR_T[:8], CSR_B[:8])) & set(zip(CSR_T[8:], CSR_B[8:]))
    tc.zero_grads(mods)
    for graph, data, weight, _ in parts:                 # no zero_grad in between
        tc.ppo_loss(mods, tc.loss_rows(mods, graph, "csr2"), data, weight).backward()
    for name, p in tc.named_params(mods).items():
        same(p.grad, parts[0][3][name] + parts[1][3][name], name)
        assert not torch.equal(parts[0][3][name], parts[1][3][name]), name


def _frozen(case, freeze):
    """A copy of the case's kernel modules with the named parameters frozen."""
    m = tc.copy_of(_case(case)["mods"], torch.float32, True)
    hit = 0
    for name, p in tc.named_params(m).items():
        if any(name.startswith(f) for f in freeze):
            p.requires_grad_(False)
            hit += 1
    assert hit >= len(freeze)
    return m


def test_frozen_subsets():
    case = "n6-env2"
    full, keep = _run(case, _frozen(case, ()))
    ref, _ = _run(case)
    for name, g in ref.items():
        same(full[name], g, name)                        # a copy of the modules is the modules
    heads = [n for n in full if n.startswith(("actor.", "critic."))]
    convs = [n for n in full if n.startswith("conv")]

    # both layers frozen: no conv node in the graph, the heads' gradients unchanged
    g, keep = _run(case, _frozen(case, ("conv.", "conv2.")))
    assert not keep["feats"].requires_grad
    assert not any(w in n for n in tc.graph_names(keep["loss"]) for w in ("EnvConv", "AttnAggregate"))
    assert all(g[n] is None for n in convs)
    for n in heads:
        same(g[n], full[n], n)

    # lin_edge frozen in both layers
    g, _ = _run(case, _frozen(case, ("conv.lin_edge", "conv2.lin_edge")))
    for n in full:
        if "lin_edge" in n:
            assert g[n] is None, n
        else:
            same(g[n], full[n], n)

    # the actor frozen: its dx still reaches the layers, so everything else is the full run's; a loss
    # without the policy and entropy terms has no actor node, the critic's own gradients (the value
    # terms alone decide them) and other layer gradients
    g, keep = _run(case, _frozen(case, ("actor.",)))
    assert any("ActorEval" in n for n in tc.graph_names(keep["loss"]))
    for n in full:
        if n.startswith("actor."):
            assert g[n] is None, n
        else:
            same(g[n], full[n], n)
    g, keep = _run(case, _frozen(case, ("actor.",)), policy_term=False)
    assert not any("ActorEval" in n for n in tc.graph_names(keep["loss"]))
    g_v, _ = _run(case, _frozen(case, ()), policy_term=False)
    for n in full:
        if n.startswith("actor."):
            assert g[n] is None and g_v[n] is None, n
        else:
            same(g[n], g_v[n], n)
        if n.startswith("critic."):
            same(g[n], full[n], n)
    assert any(not torch.equal(g[n], full[n]) for n in convs)

    # the critic's lin1 frozen
    g, _ = _run(case, _frozen(case, ("critic.lin1",)))
    for n in full:
        if n.startswith("critic.lin1"):
            assert g[n] is None, n
        else:
            same(g[n], full[n], n)


def test_padded_agents_never_reach_a_gradient():
    case = "mixed"
    c = _case(case)
    base, _ = _run(case)
    g, keep = _run(case, nan_pad=True)
    pad = ~policy._critic_mask(keep["feats"], c["data"]["n_valid"])
    assert bool(pad.any()) and bool(torch.isnan(keep["xc"][pad]).all()) and bool((keep["xa"][pad] == 0).all())
    _on_kernel_path(case, keep, c["mods"])
    for name, b in base.items():
        assert bool(torch.isfinite(g[name]).all()), name
        same(g[name], b, name)


@pytest.mark.parametrize("case", ["n3", "n6-env2"])
def test_same_bits_as_the_rollout(case):
    """logp_old from the current actor's act: the ratio is exactly 1 on every
    row and the clipped term's gradient is that of -logp * A."""
    c = _case(case)
    data = tc.rollout_data(c["mods"], c["graph"], c["form"], c["gae"], c["seed"], perturb=0.0)
    weight = tc.base_weight(data["logp_old"][..., None])
    g_clip, keep = _run(case, data=data, weight=weight)
    same(keep["logp"].detach(), data["logp_old"], "evaluate in the training graph returns act's bits")
    assert bool((keep["ratio"] == 1.0).all())
    g_logp, _ = _run(case, data=data, weight=weight, surrogate="logp")
    assert float(g_clip["actor.lin2.weight"].abs().sum()) > 0
    for name, g in g_clip.items():
        same(g_logp[name], g, name)
