"""CPU checks of tests/train_chain.py, the helpers test_gpu_train_chain.py holds
the composed HIP chain to: the fp32 torch chain against the fp64 chain on graphs
of the CPU oracle, the share conditions of every committed seed, row_scales'
rows adding up to the full gradient, and kernel=True modules off the GPU.

The bound is the GPU file's: |g - g64| <= 2e-5 * row_scale per parameter
tensor, row_scale = 1 + sum over the loss rows of |the row's own gradient|."""
import functools

import pytest
import torch

import train_chain as tc

BOUND = 2e-5
T = 4
# the shapes of the GPU cases (navigation graphs of the oracle; the mixed and the minibatch case at their sizes)
GPU_CASES = {"n3": (3, 20, "env1"), "n6-env2": (6, 12, "env2"), "n6-csr2": (6, 12, "env2"), "n24": (24, 3, "env1"),
             "mixed": (12, 24, "env1")}


@functools.lru_cache(maxsize=None)
def _setup(kind, n_agents, n_envs, form, dtype=torch.float32, kernel=False):
    """The chain ``kind`` on oracle graphs: modules, graph, data (computed by
    these modules), the reference copy and the weight it decides."""
    seed = tc.SEEDS[kind]
    slots, rew, cost, done = tc.oracle_graph(n_envs, n_agents, T, seed)
    E = slots[0]["node_feat"].shape[1]
    graph = tc.env_graph(slots, n_agents, E, T)
    mods = tc.build(kind, 1 if form == "env1" else 2, dtype, kernel)
    gae = {"reward": tc.gae_ref(rew, done), "cost": tc.gae_ref(cost, done)}
    data = tc.rollout_data(mods, tc.cast_graph(graph, dtype), form, gae, seed)
    ref = tc.copy_of(mods, torch.float64, False)
    weight, und, outside, clipped = tc.decide(ref, graph, form, data)
    return dict(mods=mods, ref=ref, graph=graph, data=data, weight=weight, shares=(und, outside, clipped), form=form)


def _ref_grads(s):
    return tc.run(s["ref"], tc.cast_graph(s["graph"], torch.float64), s["form"],
                  tc.cast_data(s["data"], torch.float64), s["weight"])


@pytest.mark.parametrize("form", ["env1", "env2"])
def test_fp32_torch_chain_against_fp64(form):
    s = _setup(form, 6, 16, form)
    assert s["data"]["ret"].shape == (2, T * 16, 6)
    g64, out = _ref_grads(s)
    assert float(out["loss"].detach()) > 0 and bool((s["graph"]["slots"][2]["edge_ptr"][-1] > 0))
    scale = tc.row_scales(s["ref"], s["graph"], s["data"], s["weight"])
    g32, _ = tc.run(s["mods"], s["graph"], form, s["data"], s["weight"])
    assert set(g32) == set(g64) == set(scale)
    for name, g in g32.items():
        assert g is not None and g.dtype == torch.float32, name
        assert float(g64[name].abs().max()) > 0, name
        e = tc.nerr(g, g64[name], scale[name])
        print(f"{form} {name}: fp32 torch chain err / row_scale = {e:.3e}")
        assert e <= BOUND, name


@pytest.mark.parametrize("kind", ["env1", "env2"] + list(GPU_CASES))
def test_share_conditions_of_the_committed_seeds(kind):
    n_agents, n_envs, form = GPU_CASES.get(kind, (6, 16, kind))
    und, outside, clipped = _setup(kind, n_agents, n_envs, form, torch.float64)["shares"]
    print(f"{kind}: undecided {und:.4%}, outside the clip range {outside:.2%}, clipped value rows {clipped}")
    assert und <= 0.01
    assert outside >= 0.10
    assert clipped >= 1


@pytest.mark.parametrize("kind", list(tc.SEEDS_W2))
def test_share_conditions_of_the_second_window_seeds(kind):
    """The second window of test_gpu_train_iterations.py, as far as the CPU has
    it: oracle graphs of 2 T steps, the fp32 torch chain, one clipped_adam_ref
    step (ClippedAdam's defaults) on the first window's gradients with the
    current actor's own logp_old, then the second window's data with
    SEEDS_W2[kind]: the fp64 copy of the stepped chain alone decides."""
    from gsmarl_amd.optim import clipped_adam_ref
    n_agents, n_envs, form = GPU_CASES[kind]
    seed = tc.SEEDS[kind]
    slots, rew, cost, done = tc.oracle_graph(n_envs, n_agents, 2 * T, seed, episode_length=T // 2)
    E = slots[0]["node_feat"].shape[1]
    assert bool(done[T - 1].all()) and bool(done[T:2 * T - 1].any())     # on the seam and inside the second window
    mods = tc.build(kind, 1 if form == "env1" else 2, torch.float32, False)
    windows = []
    for lo in (0, T):
        graph = tc.env_graph(slots[lo:lo + T + 1], n_agents, E, T)
        gae = {"reward": tc.gae_ref(rew[lo:lo + T], done[lo:lo + T]), "cost": tc.gae_ref(cost[lo:lo + T], done[lo:lo + T])}
        windows.append((graph, gae))
    graph, gae = windows[0]
    data = tc.rollout_data(mods, graph, form, gae, seed, perturb=0.0)
    grads, out = tc.run(mods, graph, form, data, tc.base_weight(data["logp_old"][..., None]))
    assert bool((out["ratio"] == 1.0).all())
    names = list(tc.named_params(mods))
    params = [tc.named_params(mods)[n] for n in names]
    zeros = [torch.zeros_like(p) for p in params]
    new_p, _, _, _, stats = clipped_adam_ref(params, [grads[n] for n in names], zeros, zeros, 0, 7e-4)
    assert float(stats[3]) == 0.0
    with torch.no_grad():
        for p, q in zip(params, new_p):
            assert not torch.equal(p, q)
            p.copy_(q)
    graph, gae = windows[1]
    data = tc.rollout_data(mods, graph, form, gae, tc.SEEDS_W2[kind])
    und, outside, clipped = tc.decide(tc.copy_of(mods, torch.float64, False), graph, form, data)[1:]
    print(f"{kind}, second window: undecided {und:.4%}, outside the clip range {outside:.2%}, clipped value rows "
          f"{clipped}")
    assert und <= 0.01
    assert outside >= 0.10
    assert clipped >= 1


@pytest.mark.parametrize("form", ["env1", "env2"])
def test_row_scales_add_up_to_the_full_gradient(form):
    s = _setup(form, 6, 16, form)
    g64, _ = _ref_grads(s)
    scale, total = tc.row_scales(s["ref"], s["graph"], s["data"], s["weight"], with_sum=True)
    for name, g in g64.items():
        assert float((total[name] - g).abs().max()) <= 1e-10, name
        assert bool((scale[name] >= 1 + g.abs() - 1e-10).all()), name


def test_undecided_rows_are_found_and_weighted_zero():
    """A row moved onto each branch point is marked; the others are not."""
    r = torch.tensor([[1.0, 0.8 + 5e-5, 1.2 - 5e-5, 0.7, 1.3, 1.0, 1.0]], dtype=torch.float64)
    v_old = torch.zeros(2, 1, 7, dtype=torch.float64)
    v = torch.zeros(2, 1, 7, dtype=torch.float64)
    ret = torch.full((2, 1, 7), 5.0, dtype=torch.float64)
    v[0, 0, 5] = 0.2 + 5e-5                     # at the value clip
    v[1, 0, 6], ret[1, 0, 6] = 0.6, 0.4         # clipped; (v - ret)^2 = (v_clip - ret)^2
    v[0, 0, 3] = 0.5                            # clipped, far from a tie: decided
    got = tc.undecided(dict(ratio=r, v=v), dict(v_old=v_old, ret=ret))
    assert got.tolist() == [[False, True, True, False, False, True, True]]


def test_kernel_modules_fall_back_to_torch_off_the_gpu():
    s = _setup("env2", 6, 16, "env2")
    k = tc.copy_of(s["mods"], torch.float32, True)
    assert k["conv"].kernel_backward and k["conv2"].kernel_backward and k["actor"].kernel_backward
    g_k, out = tc.run(k, s["graph"], "env2", s["data"], s["weight"])
    names = tc.graph_names(out["loss"])
    assert not any(w in n for n in names for w in ("EnvConv", "AttnAggregate", "ActorEval", "CriticEval"))
    g_t, _ = tc.run(s["mods"], s["graph"], "env2", s["data"], s["weight"])
    for name, g in g_t.items():
        assert torch.equal(g, g_k[name]), name

