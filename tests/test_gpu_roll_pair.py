"""The two-envs-per-wave fused rollout (gsm_roll_pair_kernel: 24 agents, 24
obstacles, the plain configuration into the bound buffers).

Every case runs one rollout launch and compares every state and output buffer
bit for bit with the per-step chain of the same actions (step kernels and emit
kernel: other code than the rollout kernels), and requires the roll status to
be 0. Shapes: a wave with one empty half (B = 1), partial workgroups (7, 9),
a full one (8), more than two (17); launches with one, two, three and five
steps (the tail alone, with and without loop emissions); the three action
formats; auto-resets inside the launch, with both halves of a wave resetting
together and on different steps; two replays of one slot back to back (epoch
and double-buffer alternation); and a config off the plain defaults, which the
generic one-env kernel runs."""
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
N = 24
KEYS = ("pos", "vel", "step_count", "episode", "node_feat", "reward", "cost", "done", "edge_count",
        "edge_ptr", "ep_acc", "ep_last", "row_mask", "contact_mask")
SEED = 29


def _env(B, **kw):
    from gsmarl_amd import EnvConfig, GpuBatchEnv
    return GpuBatchEnv(EnvConfig(n_agents=N, n_envs=B, seed=SEED, **kw), DEV)


def _acts(B, T, fmt="index"):
    gen = torch.Generator(device=DEV)
    gen.manual_seed(100 * B + T)
    idx = torch.randint(0, 5, (T, B, N), dtype=torch.int32, device=DEV, generator=gen)
    if fmt == "index":
        return idx
    if fmt == "onehot":
        return torch.nn.functional.one_hot(idx.long(), 5).to(torch.float32).contiguous()
    return (torch.rand((T, B, N, 2), device=DEV, generator=gen) * 2.0 - 1.0).contiguous()


def _start(env, stagger, nonfinite=False):
    """The seed's reset; with stagger, odd envs two steps into their episode
    (so the two halves of a wave reach the episode's end on different steps);
    with nonfinite, an agent at a NaN with its sign bit set, one at +inf and an
    obstacle at -inf, in three envs (the sweep's integer predicates assume
    finite positions: such a wave must take the float compares)."""
    env.reset(seed=SEED)
    if stagger:
        env.t["step_count"][1::2] = 2
    if nonfinite:
        pos = env.t["pos"].view(torch.int32)
        pos[2, 3, 0] = -0x400000          # 0xffc00000
        pos[4, 5, 1] = 0x7f800000
        pos[7, 2 * N + 6, 0] = -0x800000  # 0xff800000
    torch.cuda.synchronize()


def _bits(t):
    return t.view(torch.int32) if t.dtype == torch.float32 else t


def _snapshot(env):
    out = {k: env.t[k].clone() for k in KEYS}
    n = int(out["edge_ptr"][-1])
    out["edge_index"] = env.t["edge_index"][:, :n].clone()
    out["edge_attr"] = env.t["edge_attr"][:n].clone()
    return out


def _run(env, acts, K, kernels, stagger=False, replays=1, nonfinite=False):
    _start(env, stagger, nonfinite)
    slot = 1 if kernels == "roll" else 0
    env.capture(acts, K, slot=slot, kernels=kernels)
    assert env.graph_is_rollout(slot) == (kernels == "roll")
    for _ in range(replays):
        env.replay(slot)
    torch.cuda.synchronize()
    assert env.roll_gave_up() == 0
    return _snapshot(env)


def _check(B, K, fmt="index", stagger=False, replays=1, nonfinite=False, **kw):
    env = _env(B, **kw)
    acts = _acts(B, K, fmt)
    ref = _run(env, acts, K, "both", stagger, replays, nonfinite)
    got = _run(env, acts, K, "roll", stagger, replays, nonfinite)
    for k in ref:
        assert torch.equal(_bits(ref[k]), _bits(got[k])), (k, B, K, fmt)
    env.close()
    return got


@pytest.mark.parametrize("K", [1, 2, 3, 5])
@pytest.mark.parametrize("B", [1, 7, 8, 9, 17])
def test_pair_equals_chain(B, K):
    _check(B, K)


@pytest.mark.parametrize("fmt", ["index", "onehot", "cont"])
def test_pair_action_formats(fmt):
    _check(9, 5, fmt)


def test_pair_auto_reset_inside_the_launch():
    got = _check(9, 10, episode_length=4)
    assert int(got["episode"].min()) == 2


def test_pair_halves_reset_on_different_steps():
    got = _check(9, 10, stagger=True, episode_length=4)
    # even envs end episodes at steps 4 and 8, odd ones at 2, 6 and 10
    assert got["episode"][0::2].unique().tolist() == [2] and got["episode"][1::2].unique().tolist() == [3]


def test_pair_two_replays_back_to_back():
    _check(9, 5, replays=2, episode_length=4)


def test_pair_nonfinite_positions():
    got = _check(9, 3, nonfinite=True)
    assert bool(torch.isnan(got["pos"][2, 3]).any())


def test_generic_kernel_keeps_configs_off_the_plain_defaults():
    _check(9, 5, shared_reward=True, episode_length=4)

