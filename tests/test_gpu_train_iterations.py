"""Two iterations of what a trainer runs (collect, update, collect, update) on
the kernel path: the weights ClippedAdam.step wrote reach every later read.

gsm_adam_step writes the parameters through raw pointers. What is carried
across that write, and which test holds it:
  TransformerConv._packed, the cached pack of the no-grad forward_env path
  (every collection step, every value pass of rollout_data), keyed on the
  parameters' versions: test_no_grad_forward_env_sees_every_kind_of_write,
  test_second_iteration_ratio_is_one, test_second_collection_is_the_fresh_twins
  autograd graphs built before the step: test_backward_across_a_step_raises
  ClippedAdam's cached pointer tables: test_step_follows_a_replaced_storage
  the rollout buffer's slot 0 and the done flag carried into it:
  test_buffer_seam_between_the_windows, test_after_update_carries_assign
  the numbers of the second update: test_second_iteration_gradients_against_fp64

A "fresh twin" is tc.copy_of(mods, torch.float32, True) made after the write:
new modules, which hold no cache. Everything is compared bit for bit except
the last test, whose criterion is test_gpu_train_chain.py's: for every
parameter tensor max |g - g64| / row_scale <= 2e-5 on the rows the fp64 chain
decides. The cached cases of test_gpu_train_chain.py are read, never written:
every write goes to copies of their modules and to buffers built here."""
import functools

import pytest
import torch

import optim_cases as oc
import test_gpu_train_chain as tg
import train_chain as tc
from gsmarl_amd import ClippedAdam, EnvConfig, GpuBatchEnv, GraphRolloutBuffer, gnn
from test_gpu_optim import _instance, _same_state, _state

pytestmark = pytest.mark.gpu
DEV = tg.DEV
T = tg.T
BOUND = 2e-5
TWO = ["n3", "n6-env2"]
GRAPH_KEYS = ("node_feat", "edge_ptr", "edge_index", "edge_attr")


def same(a, b, what):
    """The same shape, dtype and bytes (any dtype)."""
    assert a is not None and b is not None and a.shape == b.shape and a.dtype == b.dtype, what
    assert torch.equal(a.detach().contiguous().view(torch.uint8), b.detach().contiguous().view(torch.uint8)), what


def same_graph(a, b, B, what):
    """Two env-form graphs: the features, the offsets and the stored entries."""
    total = int(a["edge_ptr"].reshape(-1)[B])
    assert total > 0
    same(a["node_feat"], b["node_feat"], (what, "node_feat"))
    same(a["edge_ptr"], b["edge_ptr"], (what, "edge_ptr"))
    same(a["edge_index"][:, :total], b["edge_index"][:, :total], (what, "edge_index"))
    same(a["edge_attr"].reshape(-1)[:total], b["edge_attr"].reshape(-1)[:total], (what, "edge_attr"))


def _params(mods):
    return list(tc.named_params(mods).values())


def _slot(buf, t):
    return {k: buf.slot(t)[k] for k in GRAPH_KEYS}


@torch.no_grad()
def _env_forward(mods, slot, N):
    """What a collection step reads: the no-grad forward_env of one slot, for a
    two-layer chain the ``(h, row_ptr)`` form and conv2 on top of it. Returns
    the tensors in the order computed; the last one is the agents' features."""
    conv = mods["conv"]
    if "conv2" not in mods:
        return (conv.forward_env(slot, rows="agents", n_agents=N),)
    h, ptr = conv.forward_env(slot, rows="all", row_ptr=True)
    B, E = h.shape[:2]
    total = int(slot["edge_ptr"][-1])
    o = mods["conv2"](torch.relu(h).reshape(B * E, -1), ptr, slot["edge_index"][1][:total],
                      slot["edge_attr"].reshape(-1)[:total])
    return h, ptr, o.view(B, E, -1)[:, :N]


@torch.no_grad()
def _env_conv_direct(conv, slot, N, two_layers):
    """The first layer by a direct gnn.env_conv call on a pack made now."""
    w, w_e = gnn.pack_conv_params(conv)
    E = slot["node_feat"].shape[1]
    return gnn.env_conv(slot["node_feat"].contiguous(), slot["edge_ptr"], slot["edge_index"], slot["edge_attr"], w, w_e,
                        conv.heads, E if two_layers else N, conv.lin_skip is not None, row_ptr=two_layers, check=True)


def _kernel_step(case, mods, **kw):
    """The chain's kernel backward on the cached case, then one ClippedAdam step."""
    tg._run(case, mods)
    opt = ClippedAdam(_params(mods), **kw)
    assert opt.kernel == kw.get("use_kernel", True)
    opt.step()
    return opt


def _write(kind, case, mods, warm):
    """Write the parameters of ``mods`` in the way ``kind`` names. ``warm()`` is
    the no-grad forward; the kinds that write twice call it between the writes,
    so the last write meets a pack of the values before it. Returns that
    forward's result (None: the caller's own is the one before the write)."""
    gen = torch.Generator(device=DEV).manual_seed(7)
    if kind == "kernel-step":
        opt = _kernel_step(case, mods)
        assert int(opt.status.item()) == 0 and int(opt.step_count.item()) == 1
        return None
    if kind == "ref-step":
        _kernel_step(case, mods, use_kernel=False)
        return None
    if kind == "inplace":
        with torch.no_grad():
            for p in _params(mods):
                p.add_(0.01 * torch.randn(p.shape, device=DEV, generator=gen))
        return None
    if kind == "load_state_dict":
        for k in tc.MODULES:
            if k in mods:
                sd = {n: v + 0.01 * torch.randn(v.shape, device=DEV, generator=gen)
                      for n, v in mods[k].state_dict().items()}
                mods[k].load_state_dict(sd)
        return None
    assert kind == "replayed-step"
    opt = _kernel_step(case, mods)                           # eager first: the code objects are loaded
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        opt.step()                                           # recorded, not run
    before = warm()                                          # the pack of the values the replay will overwrite
    for p in _params(mods):
        p.grad.copy_(0.5 * torch.randn(p.shape, device=DEV, generator=gen))    # in place: the graph's pointers
    graph.replay()
    opt.mark_updated()                                       # a replay runs no Python: the documented route
    assert int(opt.status.item()) == 0 and int(opt.step_count.item()) == 2
    return before


@pytest.mark.parametrize("case", TWO)
@pytest.mark.parametrize("kind", ["kernel-step", "ref-step", "inplace", "load_state_dict", "replayed-step"])
def test_no_grad_forward_env_sees_every_kind_of_write(kind, case):
    c = tg._case(case)
    N, two = c["N"], c["form"] == "env2"
    slot = c["slots"][1]
    mods = tc.copy_of(c["mods"], torch.float32, True)
    conv = mods["conv"]

    def warm():
        return _env_forward(mods, slot, N), {n: p.detach().clone() for n, p in conv.named_parameters()}
    before = warm()                                          # the pack is cached now
    before = _write(kind, case, mods, warm) or before
    out0, p0 = before
    out1 = _env_forward(mods, slot, N)
    changed = [n for n, p in conv.named_parameters() if not torch.equal(p.detach(), p0[n])]
    assert "lin_value.weight" in changed and "lin_query.weight" in changed and "lin_edge.weight" in changed, changed
    twin = tc.copy_of(mods, torch.float32, True)
    out_t = _env_forward(twin, slot, N)
    direct = _env_conv_direct(conv, slot, N, two)
    direct = direct if two else (direct,)
    assert len(out1) == len(out_t) == len(out0) == (3 if two else 1)
    for i, (a, b) in enumerate(zip(out1, out_t)):
        same(a, b, f"{kind}: output {i} is the fresh twin's")
    for i, (a, b) in enumerate(zip(out1, direct)):          # h (or the agents' rows) and row_ptr
        same(a, b, f"{kind}: output {i} is the direct env_conv call's")
    assert not torch.equal(out1[0], out0[0]), "the first layer's output did not move with its weights"
    assert not torch.equal(out1[-1], out0[-1])
    if two:
        same(out1[1], out0[1], "row_ptr is the graph's")


def _new_buffer(case):
    spec, seed = tg.CASES[case], tc.SEEDS[case]
    env = GpuBatchEnv(EnvConfig(n_envs=spec["B"], n_agents=spec["N"], seed=seed, **spec.get("cfg", {})), DEV)
    buf = GraphRolloutBuffer(env, episode_length=T)
    buf.reset(seed=seed)
    return env, buf


def _fields(buf, t):
    return {k: v.clone() for k, v in buf.slot(t).items()}


def _collect(mods, buf, N, seed, draw0):
    """T steps of the collecting policy: ``actor.act`` on the no-grad
    forward_env features of the current slot, draw ``draw0 + t`` at step t.
    Returns the actions and their log-probabilities, [T, B, N] each."""
    acts, logps = [], []
    for t in range(T):
        feats = _env_forward(mods, _slot(buf, buf.step), N)[-1]
        a, lp = mods["actor"].act(feats, seed, draw=draw0 + t)[:2]
        buf.insert(a)
        acts.append(a.clone())
        logps.append(lp.clone())
    assert int(mods["actor"].status.item()) == 0
    return torch.stack(acts), torch.stack(logps)


def _window(buf, N, E):
    """The buffer's current window as a graph of the env forms, its GAE and the
    done flags asserted where the case has them."""
    graph = tc.env_graph([_slot(buf, t) for t in range(T + 1)], N, E, T)
    gae = {w: (lambda v, w=w: buf.compute_returns(v, which=w, kernel=True)) for w in ("reward", "cost")}
    return graph, gae


@functools.lru_cache(maxsize=None)
def _two(case):
    """The two-iteration run of a case, made once; the tests read what it
    recorded. Window 1 is the cached case's (the same env config, seed and
    random actions) in a buffer of its own; the update is the kernel backward
    with ``logp_old`` of the current actor and one kernel ClippedAdam step;
    window 2 is collected by the stepped modules themselves."""
    c = tg._case(case)
    N, B, E, form, seed = c["N"], c["B"], c["E"], c["form"], c["seed"]
    episodic = "episode_length" in tg.CASES[case].get("cfg", {})
    r = dict(N=N, B=B, E=E, form=form, episodic=episodic)
    env, buf = _new_buffer(case)
    gen = torch.Generator(device=DEV).manual_seed(seed)
    for _ in range(T):
        buf.insert(torch.randint(0, 5, (B, N), dtype=torch.int32, device=DEV, generator=gen))
    assert not bool(buf.overflowed())
    for t in range(T + 1):                                   # the cached case's window, rebuilt
        same_graph(buf.slot(t), c["slots"][t], B, t)
    acts1 = buf.actions.clone()
    r["done1"] = buf.done.clone()

    # iteration 1: what test_same_bits_as_the_rollout does, then the step
    mods = tc.copy_of(c["mods"], torch.float32, True)
    graph1, gae = _window(buf, N, E)
    data1 = tc.rollout_data(mods, graph1, form, gae, seed, perturb=0.0)
    weight = tc.base_weight(data1["logp_old"][..., None])
    _, keep1 = tc.run(mods, graph1, form, data1, weight)
    r["ratio1"] = keep1["ratio"].detach().clone()
    opt = ClippedAdam(_params(mods))
    assert opt.kernel
    p0 = [p.detach().clone() for p in opt.params]
    opt.step()
    assert all(not torch.equal(p.detach(), q) for p, q in zip(opt.params, p0) if p.dim() == 2)     # every weight

    # the seam
    r["last1"] = _fields(buf, T)
    buf.after_update()
    r["first2"] = _fields(buf, 0)
    r["step_after_update"] = buf.step

    # collection 2, by the stepped modules; and by a fresh twin on a second env fed window 1's actions
    draw0 = T
    r["acts2"], r["logp2"] = _collect(mods, buf, N, seed, draw0)
    env_b, buf_b = _new_buffer(case)
    for t in range(T):
        buf_b.insert(acts1[t])
    buf_b.after_update()
    twin = tc.copy_of(mods, torch.float32, True)
    r["acts2_twin"], r["logp2_twin"] = _collect(twin, buf_b, N, seed, draw0)
    assert not bool(buf.overflowed()) and not bool(buf_b.overflowed())
    r.update(buf=buf, buf_b=buf_b, env=env, env_b=env_b)

    # iteration 2
    graph2, gae = _window(buf, N, E)
    r["graph2"] = graph2
    if case in tc.SEEDS_W2:                                  # the numbers of the second update, before its step
        data2p = tc.rollout_data(mods, graph2, form, gae, tc.SEEDS_W2[case])
        ref64 = tc.copy_of(mods, torch.float64, False)
        w2p, und, outside, clipped = tc.decide(ref64, graph2, form, data2p)
        gk, keep = tc.run(mods, graph2, form, data2p, w2p)
        tg._on_kernel_path(case, keep, mods)
        r.update(data2p=data2p, ref64=ref64, t32=tc.copy_of(mods, torch.float32, False), weight2p=w2p,
                 shares2p=(und, outside, clipped), gk2p=gk)
    data2 = tc.rollout_data(mods, graph2, form, gae, seed + 1, perturb=0.0)
    weight = tc.base_weight(data2["logp_old"][..., None])
    g_logp, _ = tc.run(mods, graph2, form, data2, weight, surrogate="logp")
    g_clip, keep2 = tc.run(mods, graph2, form, data2, weight)
    tg._on_kernel_path(case, keep2, mods)
    r.update(data2=data2, g_logp=g_logp, g_clip=g_clip, logp_train2=keep2["logp"].detach().clone(),
             ratio2=keep2["ratio"].detach().clone())
    opt.step()
    r["step_count"], r["opt_status"] = int(opt.step_count.item()), int(opt.status.item())

    # GAE over window 2, whose slot 0 carries window 1's last done flags
    vals = torch.randn(T + 1, B, N, device=DEV, generator=gen)
    r["values"] = vals
    r["masks0"] = buf.masks[0].clone()
    r["ret"] = {w: buf.compute_returns(vals, which=w, kernel=True) for w in ("reward", "cost")}
    kept = buf.done[0].clone()
    buf.done[0] = 1 - kept
    r["ret_flipped"] = {w: buf.compute_returns(vals, which=w, kernel=True) for w in ("reward", "cost")}
    buf.done[0] = kept
    torch.cuda.synchronize()
    return r


@pytest.mark.parametrize("case", TWO)
def test_second_iteration_ratio_is_one(case):
    """After the kernel step the value pass and ``act`` of rollout_data (the
    no-grad path) and ``evaluate`` in the training graph read the same
    weights: logp_old's bits, ratio exactly 1, the clipped term's gradient that
    of -logp * A."""
    r = _two(case)
    assert bool((r["ratio1"] == 1.0).all())
    same(r["logp_train2"], r["data2"]["logp_old"], "evaluate in the training graph returns act's bits")
    assert bool((r["ratio2"] == 1.0).all()), float((r["ratio2"] - 1.0).abs().max())
    assert float(r["g_clip"]["actor.lin2.weight"].abs().sum()) > 0
    for name, g in r["g_clip"].items():
        same(r["g_logp"][name], g, name)
    assert r["step_count"] == 2 and r["opt_status"] == 0


@pytest.mark.parametrize("case", TWO)
def test_second_collection_is_the_fresh_twins(case):
    """The stepped modules collect window 2 as a fresh twin of them does on a
    second env with the same history and the same draws."""
    r = _two(case)
    a, b, B = r["buf"], r["buf_b"], r["B"]
    same(r["acts2"], r["acts2_twin"], "the collected actions")
    same(r["logp2"], r["logp2_twin"], "their log-probabilities")
    same(a.actions, r["acts2"], "the stored actions")
    same(a.actions, b.actions, "actions")
    for k in ("node_feat", "reward", "cost", "done", "edge_ptr"):
        same(getattr(a, k), getattr(b, k), k)
    for t in range(T + 1):
        assert int(a.edge_ptr[t, B]) <= a.cap
        same_graph(a.slot(t), b.slot(t), B, t)
    assert len(torch.unique(r["acts2"])) > 1
    if r["episodic"]:                                        # episode ends inside both windows and on both last slots
        for done in (r["done1"], a.done):
            assert bool(done[1:T].any()) and bool(done[T].all())


@pytest.mark.parametrize("case", TWO)
def test_buffer_seam_between_the_windows(case):
    """after_update carries every field of the last slot into slot 0; the done
    flag it carries belongs to the step before the window: masks[0] is 1 and
    the returns do not read it."""
    r = _two(case)
    buf = r["buf"]
    assert set(r["last1"]) == set(GraphRolloutBuffer.FIELDS) and r["step_after_update"] == 0
    for k in GraphRolloutBuffer.FIELDS:
        same(r["first2"][k], r["last1"][k], k)
        same(getattr(buf, k)[0], r["last1"][k], f"{k}: slot 0 after the window was collected")
    if r["episodic"]:
        assert bool(r["last1"]["done"].all()) and bool(buf.done[0].all())
    assert bool((r["masks0"] == 1.0).all())
    vals = r["values"].cpu()
    for which, stored in (("reward", buf.reward), ("cost", buf.cost)):
        want = tc.gae_ref(stored[1:].cpu(), buf.done[1:].cpu())(vals)
        got = r["ret"][which]
        assert got.shape == (T, r["B"], r["N"]) and got.dtype == torch.float32 and float(got.abs().sum()) > 0
        assert torch.equal(got.cpu().view(torch.int32), want.view(torch.int32)), which
        same(r["ret_flipped"][which], got, f"{which}: done[0] flipped")


def test_after_update_carries_assign():
    """The ragged case: ``assign`` is carried with the fields of FIELDS."""
    env, buf = _new_buffer("mixed")
    B, N = env.B, env.N
    gen = torch.Generator(device=DEV).manual_seed(5)
    for _ in range(T):
        buf.insert(torch.randint(0, 5, (B, N), dtype=torch.int32, device=DEV, generator=gen))
    last = _fields(buf, T)
    assert set(last) == set(GraphRolloutBuffer.FIELDS) | {"assign"} and bool((last["assign"] >= 0).any())
    assert not torch.equal(last["node_feat"], buf.node_feat[0])
    buf.after_update()
    assert buf.step == 0
    for k, v in last.items():
        same(buf.slot(0)[k], v, k)
        same(buf.slot(T)[k], v, k)
    buf.insert(torch.randint(0, 5, (B, N), dtype=torch.int32, device=DEV, generator=gen))
    for k, v in last.items():
        same(buf.slot(0)[k], v, f"{k}: a step writes slot 1, not slot 0")
    assert buf.step == 1 and not torch.equal(buf.node_feat[1], buf.node_feat[0])
    env.close()


@pytest.mark.parametrize("case", list(tc.SEEDS_W2))
def test_second_iteration_gradients_against_fp64(case):
    """Window 2, after the kernel step, with an old actor perturbed as in
    test_gpu_train_chain.py (seed SEEDS_W2): every parameter gradient of the
    kernel chain against fp64 autograd of the stepped modules' fp64 copy, the
    criterion of test_gradients_against_fp64_autograd unchanged."""
    r = _two(case)
    und, outside, clipped = r["shares2p"]
    print(f"{case}, second window: undecided {und:.4%}, outside the clip range {outside:.2%}, clipped value rows "
          f"{clipped}")
    assert und <= 0.01 and outside >= 0.10 and clipped >= 1
    graph, data, weight, form = r["graph2"], r["data2p"], r["weight2p"], r["form"]
    g64, _ = tc.run(r["ref64"], tc.cast_graph(graph, torch.float64), form, tc.cast_data(data, torch.float64), weight)
    scale = tc.row_scales(r["ref64"], graph, data, weight)
    gt, keep_t = tc.run(r["t32"], graph, form, data, weight)
    assert not any(w in n for n in tc.graph_names(keep_t["loss"]) for w in tg.KERNEL_NODES)
    gk = r["gk2p"]
    assert set(gk) == set(g64) == set(scale)
    worst, over = (0.0, 0.0), []
    for name, g in g64.items():
        assert gk[name] is not None and gk[name].dtype == torch.float32 and bool(torch.isfinite(gk[name]).all()), name
        assert float(g.abs().max()) > 0, name
        e_k, e_t = tc.nerr(gk[name], g, scale[name]), tc.nerr(gt[name], g, scale[name])
        print(f"{case}, second window {name}: err / row_scale  kernel chain {e_k:.3e}  fp32 torch chain {e_t:.3e}")
        worst = (max(worst[0], e_k), max(worst[1], e_t))
        if e_k > BOUND:
            over.append((name, e_k))
    print(f"{case}, second window: worst err / row_scale  kernel chain {worst[0]:.3e}  fp32 torch chain {worst[1]:.3e}")
    assert not over, over


def test_backward_across_a_step_raises():
    """A graph built before the step saved the parameters: its backward after
    the step raises, with ClippedAdam on the kernel path as with
    torch.optim.Adam on the torch formulations (torch's own rule)."""
    case = "n3"
    c = tg._case(case)
    weight = tg._ref(case)["weight"]

    def loss_of(mods):
        tg._run(case, mods)                                  # an earlier backward: the gradients the step takes
        return tc.ppo_loss(mods, tc.loss_rows(mods, c["graph"], c["form"]), c["data"], weight)
    t32 = tc.copy_of(c["mods"], torch.float32, False)
    loss = loss_of(t32)
    assert not any(w in n for n in tc.graph_names(loss) for w in tg.KERNEL_NODES)
    torch.optim.Adam(_params(t32), lr=7e-4).step()
    with pytest.raises(RuntimeError, match="modified by an inplace operation"):
        loss.backward()

    mods = tc.copy_of(c["mods"], torch.float32, True)
    loss = loss_of(mods)
    assert all(any(w in n for n in tc.graph_names(loss)) for w in ("EnvConv", "ActorEval", "CriticEval"))
    opt = ClippedAdam(_params(mods))
    assert opt.kernel
    opt.step()
    with pytest.raises(RuntimeError, match="modified by an inplace operation"):
        loss.backward()
    # a graph built after the step is the usual one
    g, _ = tg._run(case, mods)
    assert all(bool(torch.isfinite(x).all()) for x in g.values())


def test_step_follows_a_replaced_storage():
    """``p.data = ...`` between two steps: the second updates the new storage
    as a twin does that was given the same state, and leaves the old alone."""
    st = oc.make("clipped", device=DEV)
    params, opt = _instance(st)
    twin_p, twin = _instance(st)
    opt.step()
    twin.step()
    _same_state(_state(params, opt), _state(twin_p, twin), "the first step")
    old = params[0].data                                     # held to the end: live memory whatever the step writes
    old_bits = old.clone()
    params[0].data = old.clone()
    assert params[0].data_ptr() != old.data_ptr()
    before = params[0].detach().clone()
    opt.step()
    twin.step()
    _same_state(_state(params, opt), _state(twin_p, twin), "the step after the storage was replaced")
    same(opt.stats, twin.stats, "stats")
    assert not torch.equal(params[0].detach(), before)
    same(old, old_bits, "the old storage")
    assert int(opt.step_count.item()) == st["t"] + 2 and int(opt.status.item()) == 0
