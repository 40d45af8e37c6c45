"""One PPO update's chain, stage by stage, for test_train_chain_ref.py (CPU) and
test_gpu_train_chain.py (GPU): graph -> TransformerConv layer(s) -> ActorHead and
CriticHead -> the clipped PPO / Lagrangian loss. Helpers only; they run on any
device and dtype, so the same code is the kernel chain (``kernel=True`` modules,
fp32, on the GPU), the fp32 torch chain and the fp64 reference.

A *graph* is a dict: ``N``, ``E``; ``slots`` (env-form graphs of B envs each:
the features of every slot are computed, the loss takes the envs of the first
``rows``); for ``csr2`` a ``batch`` of ``GraphRolloutBuffer.graph_batch_csr``;
``samples`` = (slot graphs, slot of each loss env, env of each loss env), from
which ``row_scales`` cuts one-env graphs. *data* is what a rollout stores
(``make_data``); it is computed once, by one chain, and every chain reads it.
"""
import copy

import numpy as np
import torch

from gsmarl_amd import ActorHead, CriticHead, PopArt, policy
from gsmarl_amd.gnn import TransformerConv

HEADS, CC, HC = 3, 16, 48
CLIP, VCLIP, ENT_COEF, COST_MULT = 0.2, 0.2, 0.01, 0.5
EDGE, TIE = 1e-4, 1e-5                   # undecided(): distance to a branch point; of the two squared errors
PERTURB = 0.05                           # the old actor: every parameter + PERTURB * randn
MODULES = ("conv", "conv2", "actor", "critic")
# one seed per case: the modules, the old actor's perturbation and the draws. test_train_chain_ref.py holds
# every seed to the share conditions (undecided rows, rows outside the clip range, a clipped value row)
SEEDS = {"env1": 11, "env2": 12, "n3": 21, "n6-env2": 22, "n6-csr2": 23, "n24": 24, "mixed": 25}
# the second window of the two-iteration tests (test_gpu_train_iterations.py): the seed of its old actor's
# perturbation and draws, after one optimizer step; held to the same share conditions
SEEDS_W2 = {"n3": 31}


def _make(layers, dtype, kernel, device):
    kw = dict(kernel_backward=True) if kernel else dict(use_kernel=False)
    mods = dict(conv=TransformerConv(7, CC, heads=HEADS, **kw), actor=ActorHead(HC, 64, 5, **kw),
                critic=CriticHead(HC, 64, 2, **kw), popart=PopArt(2))
    if layers == 2:
        mods["conv2"] = TransformerConv(HC, CC, heads=HEADS, **kw)
    return {k: m.to(device=device, dtype=dtype) for k, m in mods.items()}


def build(kind, layers, dtype, kernel, device="cpu"):
    """The modules of one chain, seeded by ``SEEDS[kind]``: ``conv`` (7 -> 3 x
    16), with two layers ``conv2`` (48 -> 3 x 16), ``actor`` (48, 64, 5),
    ``critic`` (48, 64, 2) and a ``popart`` that has seen one update."""
    torch.manual_seed(SEEDS[kind])
    mods = _make(layers, dtype, kernel, "cpu")
    g = torch.Generator().manual_seed(SEEDS[kind])
    seen = torch.stack([torch.randn(64, generator=g) * 2.0 - 1.0, torch.rand(64, generator=g) * 0.5])
    mods["popart"].update(seen.to(dtype))
    return {k: m.to(device) for k, m in mods.items()}


def copy_of(mods, dtype, kernel, device=None):
    """The same chain in another dtype / formulation: fresh modules that get
    their parameters (and PopArt's statistics) through ``load_state_dict``."""
    device = device if device is not None else next(mods["actor"].parameters()).device
    new = _make(2 if "conv2" in mods else 1, dtype, kernel, device)
    for k, m in new.items():
        m.load_state_dict(mods[k].state_dict())
    return new


def named_params(mods):
    """{"conv.lin_query.weight": parameter, ...} over conv, conv2, actor, critic."""
    return {f"{k}.{n}": p for k in MODULES if k in mods for n, p in mods[k].named_parameters()}


def grads_of(mods):
    return {n: (p.grad.detach().clone() if p.grad is not None else None) for n, p in named_params(mods).items()}


def zero_grads(mods):
    for p in named_params(mods).values():
        p.grad = None


def _cast_env(g, dtype, device):
    out = {k: (v.to(device) if torch.is_tensor(v) else v) for k, v in g.items()}
    out["node_feat"], out["edge_attr"] = out["node_feat"].to(dtype), out["edge_attr"].to(dtype)
    return out


def cast_graph(graph, dtype, device=None):
    """The graph with its float tensors in ``dtype`` (ids and offsets unchanged)."""
    dev = device if device is not None else graph["slots"][0]["node_feat"].device
    out = dict(graph, slots=[_cast_env(s, dtype, dev) for s in graph["slots"]])
    if graph.get("batch") is not None:
        out["batch"] = _cast_env(graph["batch"], dtype, dev)
    for k in ("n_valid", "n_valid_env"):
        if graph.get(k) is not None:
            out[k] = graph[k].to(dev)
    out["samples"] = ([_cast_env(s, dtype, dev) for s in graph["samples"][0]],) + tuple(graph["samples"][1:])
    return out


def cast_data(data, dtype, device=None):
    return {k: (v if v is None else v.to(device=device if device is not None else v.device,
                                         dtype=dtype if v.is_floating_point() else v.dtype))
            for k, v in data.items()}


def features(mods, graph, form, keep=None):
    """Agent features [rows of the form, N, 48] in one of three forms (module
    docstring of test_gpu_train_chain.py); ``keep["h"]`` collects the first
    layer's outputs of the two-layer forms, ``keep["slot_feats"]`` the per-slot
    tensors the ``cat`` joins."""
    conv, N, E = mods["conv"], graph["N"], graph["E"]
    keep = keep if keep is not None else {}
    if form == "env1":
        outs = [conv.forward_env(s, rows="agents", n_agents=N) for s in graph["slots"]]
        keep["slot_feats"] = outs
        return torch.cat(outs)
    conv2 = mods["conv2"]
    if form == "env2":
        outs = []
        for s in graph["slots"]:
            h, ptr = conv.forward_env(s, rows="all", row_ptr=True)
            keep.setdefault("h", []).append(h)
            B = h.shape[0]
            total = int(s["edge_ptr"][-1])
            o = conv2(torch.relu(h).reshape(B * E, -1), ptr, s["edge_index"][1][:total],
                      s["edge_attr"].reshape(-1)[:total])
            outs.append(o.view(B, E, -1)[:, :N])
        keep["slot_feats"] = outs
        return torch.cat(outs)
    if form == "csr2":
        b = graph["batch"]
        args = (b["row_ptr"], b["col"], b["edge_attr"])
        h = conv(b["node_feat"], *args, transpose=b["transpose"])
        keep.setdefault("h", []).append(h)
        o = conv2(torch.relu(h), *args, transpose=b["transpose"])
        return o.view(-1, E, o.shape[-1])[:, :N]
    raise ValueError(form)


def loss_rows(mods, graph, form, keep=None):
    """The features the loss reads: the first ``graph["rows"]`` envs of ``features``."""
    return features(mods, graph, form, keep)[:graph["rows"]]


def ppo_loss(mods, feats, data, weight, keep=None, policy_term=True, surrogate="clip", nan_pad=False, wsum=None):
    """The clipped PPO / Lagrangian loss of ``feats`` [R, N, 48]; every term a
    weighted mean over its rows (``weight`` [R, N]; ``wsum``: the mean's
    denominator when ``feats`` is a part of the rows). ``keep`` receives
    ``logp, ent, v, ratio`` and the per-row terms ``pol_rows`` [R, N] and
    ``val_rows`` [2, R, N], whose sum the loss is. ``policy_term=False`` leaves
    out the policy and entropy terms; ``surrogate="logp"`` replaces the clipped
    term by ``-logp * A`` (its gradient where ``ratio == 1``). ``nan_pad``
    overwrites the padded agents' rows with NaN inside the chain: the critic
    and the loss mask them, the actor gets zeros there."""
    dt = feats.dtype
    n_valid = data.get("n_valid")
    xa = xc = feats
    if nan_pad:
        pad = ~policy._critic_mask(feats, n_valid)[..., None]
        xc = torch.where(pad, torch.full((), float("nan"), dtype=dt, device=feats.device), feats)
        xa = torch.where(pad, torch.zeros((), dtype=dt, device=feats.device), xc)
    w = weight.to(dt)
    wsum = w.sum() if wsum is None else wsum
    v = mods["critic"](xc, n_valid, data["denorm"])
    ret, v_old = data["ret"], data["v_old"]
    v_clip = v_old + (v - v_old).clamp(-VCLIP, VCLIP)
    val_rows = w[None] * torch.max((v - ret) ** 2, (v_clip - ret) ** 2) / wsum
    out = dict(v=v, val_rows=val_rows, xa=xa, xc=xc)
    loss = val_rows.sum()
    if policy_term:
        logp, ent = mods["actor"].evaluate(xa, data["actions"])
        A = data["adv"][0] - COST_MULT * data["adv"][1]
        ratio = torch.exp(logp - data["logp_old"])
        if surrogate == "clip":
            pol = -torch.min(ratio * A, ratio.clamp(1.0 - CLIP, 1.0 + CLIP) * A)
        else:
            pol = -ratio.detach() * 0 + (-logp * A)
        pol_rows = w * (pol - ENT_COEF * ent) / wsum
        out.update(logp=logp, ent=ent, ratio=ratio, pol_rows=pol_rows)
        loss = loss + pol_rows.sum()
    if keep is not None:
        keep.update(out)
    return loss


def gae_ref(reward, done, gamma=0.99, gae_lambda=0.95):
    """``GraphRolloutBuffer.compute_returns`` without a buffer: ``reward`` [T,
    B, N] and ``done`` [T, B] of the steps; returns a function (values [T+1, B,
    N]) -> returns [T, B, N]."""
    def run(values):
        T = reward.shape[0]
        masks = (1.0 - done.to(values.dtype))[..., None]
        ret, gae = torch.empty_like(reward, dtype=values.dtype), torch.zeros_like(values[0])
        for t in reversed(range(T)):
            delta = reward[t].to(values.dtype) + gamma * values[t + 1] * masks[t] - values[t]
            gae = delta + gamma * gae_lambda * masks[t] * gae
            ret[t] = gae + values[t]
        return ret
    return run


@torch.no_grad()
def returns(mods, feats_all, n_slots, gae, n_valid=None):
    """Returns [2, S, B, N] of both heads: the critic's denormalised values of
    every stored slot, GAE (``gae["reward"]`` / ``gae["cost"]``: values [S, B,
    N] -> [S-1, B, N]) and, for the last slot, its value."""
    denorm = mods["popart"].stats()
    v = mods["critic"](feats_all, n_valid, denorm)
    v = v.view(2, n_slots, -1, v.shape[-1])
    out = []
    for h, which in enumerate(("reward", "cost")):
        vh = v[h].contiguous()
        out.append(torch.cat([gae[which](vh).to(vh.dtype), vh[-1:]]))
    return torch.stack(out)


def _act(actor, feats, seed):
    if feats.is_cuda:
        return actor.act(feats, seed)[:2]
    logits = actor.logits(feats)
    u = policy.actor_uniform_ref(feats.shape[0], feats.shape[1], seed, device=feats.device)
    act = policy.actor_sample_ref(logits, u)
    logp = policy.actor_dist_ref(logits)[0].gather(-1, act.to(torch.int64)[..., None])[..., 0]
    return act, logp


@torch.no_grad()
def make_data(mods, feats, ret, seed, n_valid=None, perturb=PERTURB):
    """What the rollout stored for the loss rows ``feats`` [R, N, 48] with
    returns ``ret`` [2, R, N]: actions and ``logp_old`` of an old actor (the
    current one, every parameter + ``perturb * randn``; ``perturb=0``: the
    current actor itself), ``v_old`` = the values + 0.1 randn, the advantages
    ``ret - v`` normalised per head over the valid rows, PopArt's statistics."""
    feats = feats.contiguous()
    g = torch.Generator().manual_seed(seed)
    old = mods["actor"]
    if perturb:
        old = copy.deepcopy(mods["actor"])
        for p in old.parameters():
            p.add_((perturb * torch.randn(p.shape, generator=g)).to(p))
    actions, logp_old = _act(old, feats, seed)
    denorm = mods["popart"].stats()
    v = mods["critic"](feats, n_valid, denorm)
    v_old = v + (0.1 * torch.randn(v.shape, generator=g)).to(v)
    mask = policy._critic_mask(feats, n_valid)
    m = (mask if mask is not None else torch.ones_like(actions, dtype=torch.bool)).to(v.dtype)[None]
    adv = ret - v
    mean = (adv * m).sum((1, 2), keepdim=True) / m.sum()
    std = (((adv - mean) ** 2 * m).sum((1, 2), keepdim=True) / m.sum()).sqrt()
    adv = (adv - mean) / (std + 1e-5) * m
    return dict(actions=actions, logp_old=logp_old.clone(), v_old=v_old, ret=ret.clone(), adv=adv, denorm=denorm,
                n_valid=n_valid)


def base_weight(feats, n_valid=None):
    """[R, N]: 1 for an agent of its env, 0 for a padded one."""
    mask = policy._critic_mask(feats, n_valid)
    return (mask if mask is not None else torch.ones(feats.shape[:2], dtype=torch.bool, device=feats.device)).to(
        torch.float64)


def undecided(out, data):
    """bool [R, N] from the fp64 chain's outputs (``keep`` of ``ppo_loss``):
    the row lies within ``EDGE`` of a branch point of the loss: the ratio at a
    clip bound, ``|v - v_old|`` at the value clip, or, on a clipped value row,
    the two squared errors within ``TIE`` of each other."""
    r, v, v_old, ret = out["ratio"], out["v"], data["v_old"], data["ret"]
    u = ((r - (1.0 - CLIP)).abs() < EDGE) | ((r - (1.0 + CLIP)).abs() < EDGE)
    d = (v - v_old).abs()
    v_clip = v_old + (v - v_old).clamp(-VCLIP, VCLIP)
    tie = (d > VCLIP) & (((v - ret) ** 2 - (v_clip - ret) ** 2).abs() < TIE)
    return u | (((d - VCLIP).abs() < EDGE) | tie).any(0)


def shares(out, data, weight):
    """(share of weighted rows with the ratio outside the clip range, number
    of weighted value rows that are clipped)."""
    on = weight > 0
    r = out["ratio"]
    outside = ((r < 1.0 - CLIP) | (r > 1.0 + CLIP)) & on
    clipped = ((out["v"] - data["v_old"]).abs() > VCLIP) & on[None]
    return float(outside.sum()) / max(int(on.sum()), 1), int(clipped.sum())


@torch.no_grad()
def rollout_data(mods, graph, form, gae, seed, perturb=PERTURB):
    """``make_data`` for the loss rows of ``graph``, by the chain ``mods``: the
    values of every slot (the env form of the chain's depth), the returns of
    both heads, then the loss rows' own features in ``form``. The loss envs'
    returns are gathered by ``graph["samples"]``."""
    S = len(graph["slots"])
    nv = graph.get("n_valid")
    B = graph["slots"][0]["node_feat"].shape[0]
    env_form = "env2" if "conv2" in mods else "env1"
    feats_all = features(mods, graph, env_form)
    nv_all = graph.get("n_valid_env")
    ret_all = returns(mods, feats_all, S, gae, nv_all.repeat(S) if nv_all is not None else None)
    _, t_idx, b_idx = graph["samples"]
    dev = feats_all.device
    ret = ret_all[:, torch.tensor(t_idx, device=dev), torch.tensor(b_idx, device=dev)].contiguous()
    feats = feats_all[:graph["rows"]] if form == env_form else loss_rows(mods, graph, form)
    assert feats.shape[0] == len(t_idx) and B * S == feats_all.shape[0]
    return make_data(mods, feats, ret, seed, nv, perturb)


def run(mods, graph, form, data, weight, backward=True, **kw):
    """One forward (and backward from fresh ``.grad``) of the chain. Returns
    ``(gradients by name, keep)``; ``keep`` holds ``loss``, ``feats`` and what
    ``features`` and ``ppo_loss`` keep."""
    zero_grads(mods)
    keep = {}
    with torch.set_grad_enabled(backward):
        feats = loss_rows(mods, graph, form, keep)
        loss = ppo_loss(mods, feats, data, weight, keep, **kw)
    keep.update(feats=feats, loss=loss)
    if backward:
        loss.backward()
    return grads_of(mods), keep


def decide(ref_mods, graph, form, data):
    """``(weight [R, N] fp64, share of undecided rows, share of rows outside
    the clip range, clipped value rows)`` from the fp64 chain alone: the valid
    rows without the undecided ones."""
    g64, d64 = cast_graph(graph, torch.float64), cast_data(data, torch.float64)
    n_valid = data.get("n_valid")
    _, out = run(ref_mods, g64, form, d64, base_weight(data["logp_old"][..., None], n_valid), backward=False)
    w0 = base_weight(out["feats"], n_valid)
    und = undecided(out, d64) & (w0 > 0)
    weight = w0 * (~und).to(w0.dtype)
    outside, clipped = shares(out, d64, weight)
    return weight, float(und.sum()) / max(int((w0 > 0).sum()), 1), outside, clipped


def nerr(got, ref, scale):
    """max |got - ref| / scale over a tensor."""
    return float(((got.double().cpu() - ref.double().cpu()).abs() / scale.cpu()).max())


def graph_names(t):
    """The autograd node type names below a tensor."""
    seen, todo, names = set(), [t.grad_fn], set()
    while todo:
        f = todo.pop()
        if f is None or f in seen:
            continue
        seen.add(f)
        names.add(type(f).__name__)
        todo.extend(n for n, _ in f.next_functions)
    return names


def sample_graph(slot, b, E):
    """Env ``b`` of an env-form graph as a graph of one env (local ids)."""
    p0, p1 = int(slot["edge_ptr"][b]), int(slot["edge_ptr"][b + 1])
    return dict(node_feat=slot["node_feat"][b:b + 1], edge_ptr=torch.tensor([0, p1 - p0], dtype=torch.int64),
                edge_index=slot["edge_index"][:, p0:p1] - b * E, edge_attr=slot["edge_attr"].reshape(-1)[p0:p1])


def row_scales(ref_mods, graph, data, weight, with_sum=False):
    """For every parameter tensor ``1 + sum_r |g_r|``, ``g_r`` the fp64
    gradient of row r's weighted loss term alone; a row is one (sample, agent)
    of the policy term (with its entropy bonus) or one (head, sample, agent) of
    the value term. Row r reads the graph of its own env only, so the rows are
    taken env by env on one-env graphs, on the CPU; rows of weight 0 have no
    gradient. ``with_sum``: also ``sum_r g_r`` (the full gradient)."""
    mods = copy_of(ref_mods, torch.float64, False, "cpu")
    params = named_params(mods)
    names, plist = list(params), list(params.values())
    form = "env2" if "conv2" in mods else "env1"
    slots, t_idx, b_idx = cast_graph(graph, torch.float64, "cpu")["samples"]
    data = cast_data(data, torch.float64, "cpu")
    weight = weight.to("cpu", torch.float64)
    wsum = weight.sum()
    tot = [torch.zeros_like(p) for p in plist]
    mag = [torch.zeros_like(p) for p in plist]
    for e, (t, b) in enumerate(zip(t_idx, b_idx)):
        if not bool((weight[e] > 0).any()):
            continue
        one = dict(N=graph["N"], E=graph["E"], slots=[sample_graph(slots[t], b, graph["E"])])
        d = {k: (v if v is None or k == "denorm" else (v[:, e:e + 1] if v.dim() == 3 else v[e:e + 1]))
             for k, v in data.items()}
        keep = {}
        ppo_loss(mods, features(mods, one, form), d, weight[e:e + 1], keep, wsum=wsum)
        on = (weight[e] > 0).nonzero()[:, 0].tolist()
        rows = [keep["pol_rows"][0, i] for i in on] + [keep["val_rows"][h, 0, i] for h in range(2) for i in on]
        for r in rows:
            gs = torch.autograd.grad(r, plist, retain_graph=True, allow_unused=True)
            for k, g in enumerate(gs):
                if g is not None:
                    tot[k] += g
                    mag[k] += g.abs()
    scale = {n: 1 + m for n, m in zip(names, mag)}
    return (scale, dict(zip(names, tot))) if with_sum else scale


def oracle_graph(n_envs, n_agents, n_steps, seed, episode_length=None):
    """CPU graphs from ``oracle.batch_ref``: a reset and ``n_steps`` steps with
    random actions, fp32 node features and distances; an episode lasts
    ``episode_length`` steps (half of ``n_steps`` when None). Returns (slots,
    reward [T, B, N], cost [T, B, N], done [T, B])."""
    from oracle import batch_ref as br
    cfg = br.make_cfg(n_envs=n_envs, n_agents=n_agents, seed=seed,
                      episode_length=episode_length or max(n_steps // 2, 1))
    st = br.new_state(cfg, seed=seed, dtype=np.float32)
    rng = np.random.default_rng(seed)

    def slot(ob):
        return dict(node_feat=torch.from_numpy(np.asarray(ob["node_feat"], np.float32)),
                    edge_ptr=torch.from_numpy(np.asarray(ob["edge_ptr"], np.int64)),
                    edge_index=torch.from_numpy(np.asarray(ob["edge_index"], np.int32)),
                    edge_attr=torch.from_numpy(np.asarray(ob["edge_attr"], np.float32)).reshape(-1))
    slots, rew, cost, done = [slot(br.observe(cfg, st, np.float32))], [], [], []
    for _ in range(n_steps):
        st, ob = br.step(cfg, st, rng.integers(0, 5, (n_envs, n_agents)).astype(np.int32), 1, np.float32, seed)
        slots.append(slot(ob))
        rew.append(torch.from_numpy(np.asarray(ob["reward"], np.float32)))
        cost.append(torch.from_numpy(np.asarray(ob["cost"], np.float32)))
        done.append(torch.from_numpy(np.asarray(ob["done"], np.uint8)))
    return slots, torch.stack(rew), torch.stack(cost), torch.stack(done)


def env_graph(slots, N, E, rows_slots):
    """The graph dict of the env forms: every slot's features are computed, the
    loss takes the envs of the first ``rows_slots`` slots."""
    B = slots[0]["node_feat"].shape[0]
    t_idx = [t for t in range(rows_slots) for _ in range(B)]
    b_idx = [b for _ in range(rows_slots) for b in range(B)]
    return dict(N=N, E=E, slots=slots, rows=rows_slots * B, batch=None, n_valid=None, samples=(slots, t_idx, b_idx))
