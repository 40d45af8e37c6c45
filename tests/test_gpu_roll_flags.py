"""The fused rollout's instantiations by configuration flag.

gsm_roll_seg_kernel is compiled in a plain form for the common configuration
(no strict mode, per-agent rewards, auto-reset, no speed clamp, bound outputs,
pacing) and in a generic form for everything else; the host picks by the
launch's arguments. Here one flag at a time is moved off its default, so both
forms run, at shapes whose last workgroup is partial (B is no multiple of 4),
with several in-launch re-layouts (T > 2 * episode length) and with at least
three steps (the loop, both tail emissions, and the edge-list scan kept from
two iterations back). The packed kernels of the 3-agent shape take the same
flags as run-time branches of one instantiation per action format:
gsm_roll_pack2_kernel (stepper and emitter waves) at 9 envs (a wave with one
live env, a dead wave, more steps than the emission ring has slots) and at
1040 envs (260 waves, more than one 64-wave group), gsm_roll_pack_kernel past
8192 envs (a half-dead last workgroup, more steps than its emission lags, so
the in-loop emission and the tail both run). Every case is compared bit for
bit, over every state and output buffer, with the per-step chain of the same actions (step kernels and
emit kernel: other code than the rollout kernel). (A reset layout holds no
coincident pair, so the strict case runs the strict instantiation on inputs
where it equals the default; test_gpu_roll_states.py runs it on coincident
pairs, NaN bits compared.) Also the rollout-buffer form
(per-step redirected outputs), the one-launch eager step, and one case against
the fp64 CPU oracle."""
import numpy as np
import pytest
import torch

from oracle import batch_ref as br
from parity_tol import check_state

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
KEYS = ("pos", "vel", "step_count", "episode", "node_feat", "reward", "cost", "done", "edge_count",
        "edge_ptr", "ep_acc", "ep_last", "row_mask", "contact_mask")
SHAPES = [(24, 5, 7, 3), (12, 5, 6, 2), (6, 9, 7, 3),   # N, B, T, episode length
          (3, 9, 11, 3), (3, 1040, 11, 3), (3, 8200, 7, 3)]
MAX_SPEED = 0.3
FLAGS = {"default": {}, "shared_reward": dict(shared_reward=True), "no_auto_reset": dict(auto_reset=False),
         "max_speed": dict(max_speed=MAX_SPEED), "strict": dict(strict_degenerate=True)}
SEED = 17


def _env(**kw):
    from gsmarl_amd import EnvConfig, GpuBatchEnv
    cfg = EnvConfig(**kw)
    return GpuBatchEnv(cfg, DEV), cfg


def _acts(N, B, T):
    gen = torch.Generator(device=DEV)
    gen.manual_seed(1000 * N + B)
    return torch.randint(0, 5, (T, B, N), dtype=torch.int32, device=DEV, generator=gen)


def _same(ref, env, what):
    for k in KEYS:
        assert torch.equal(ref[k], env.t[k]), (what, k)
    n = int(ref["edge_ptr"][-1])
    assert torch.equal(ref["edge_index"][:, :n], env.t["edge_index"][:, :n]), what
    assert torch.equal(ref["edge_attr"][:n], env.t["edge_attr"][:n]), what


def _chain(env, acts, T):
    """Every buffer after the per-step chain of T steps from the seed's reset."""
    env.reset(seed=SEED)
    env.capture(acts, T, slot=0, kernels="both")
    assert not env.graph_is_rollout(0)
    env.replay(0)
    torch.cuda.synchronize()
    return {k: v.clone() for k, v in env.t.items()}


@pytest.mark.parametrize("flag", sorted(FLAGS))
@pytest.mark.parametrize("N,B,T,EL", SHAPES)
def test_roll_flag_equals_chain(N, B, T, EL, flag):
    kw = dict(n_agents=N, n_envs=B, episode_length=EL, seed=SEED, **FLAGS[flag])
    env, cfg = _env(**kw)
    acts = _acts(N, B, T)
    if flag == "max_speed":
        # the clamp fires: unclamped, the oracle's first step already exceeds the limit
        ocfg = br.make_cfg(**{k: v for k, v in cfg.replace(max_speed=0.0).to_dict().items() if k in br.DEFAULTS})
        st = br.new_state(ocfg, seed=SEED, dtype=np.float32)
        _, v1 = br.physics(ocfg, st["pos"].astype(np.float64), st["vel"].astype(np.float64),
                           acts[0].cpu().numpy(), 1, np.float64)
        assert (np.hypot(v1[..., 0], v1[..., 1]) > MAX_SPEED).any()
    ref = _chain(env, acts, T)
    env.reset(seed=SEED)
    env.capture(acts, T, slot=1, kernels="roll")
    assert env.graph_is_rollout(1)   # the default config included: the rollout form was taken
    env.replay(1)
    torch.cuda.synchronize()
    assert not env.roll_gave_up()
    _same(ref, env, flag)
    if flag == "no_auto_reset":
        assert bool(env.t["done"].all()) and int(env.t["episode"].max()) == 0
    elif T > EL:
        assert int(env.t["episode"].min()) == T // EL   # re-layouts inside the launch
    env.close()


@pytest.mark.parametrize("N,B,T,EL", SHAPES)
def test_roll_redirected_outputs_equal_chain(N, B, T, EL):
    """A rollout buffer's episode (one launch writing step j's outputs, every
    node-feature row included, into slot j + 1) against the per-step chain run
    one step at a time, its bound outputs read after every step."""
    from gsmarl_amd import GraphRolloutBuffer
    kw = dict(n_agents=N, n_envs=B, episode_length=EL, seed=SEED)
    env, _ = _env(**kw)
    ref, _ = _env(**kw)
    acts = _acts(N, B, T)
    gb = GraphRolloutBuffer(env, episode_length=T)
    gb.reset(seed=SEED)
    gb.capture(acts)
    assert env.graph_is_rollout(0)
    gb.replay()
    torch.cuda.synchronize()
    assert not env.roll_gave_up()
    ref.reset(seed=SEED)
    for t in range(T):
        ref.capture(acts[t:t + 1], 1, slot=0, kernels="both")
        ref.replay(0)
        torch.cuda.synchronize()
        for k in ("node_feat", "reward", "cost", "done", "edge_count", "edge_ptr"):
            assert torch.equal(getattr(gb, k)[t + 1], ref.t[k]), (t, k)
        n = int(ref.t["edge_ptr"][-1])
        assert torch.equal(gb.edge_index[t + 1][:, :n], ref.t["edge_index"][:, :n]), t
        assert torch.equal(gb.edge_attr[t + 1][:n], ref.t["edge_attr"][:n]), t
    for k in ("pos", "vel", "step_count", "episode", "ep_acc", "ep_last", "row_mask", "contact_mask"):
        assert torch.equal(env.t[k], ref.t[k]), k
    env.close()
    ref.close()


def test_eager_one_launch_steps_equal_chain():
    """The one-launch eager step (the default at 24 agents), T of them."""
    N, B, T, EL = SHAPES[0]
    env, _ = _env(n_agents=N, n_envs=B, episode_length=EL, seed=SEED)
    acts = _acts(N, B, T)
    ref = _chain(env, acts, T)
    env.reset(seed=SEED)
    for t in range(T):
        env.step(acts[t], sync_edges=False)
    torch.cuda.synchronize()
    assert not env.roll_gave_up()
    _same(ref, env, "eager")
    env.close()


def test_roll_flags_oracle_direct():
    """The last step of the default config's rollout against the fp64 oracle
    stepped from the identical fp32 pre-step state (as test_gpu_roll's
    test_roll_oracle_direct, at this file's first shape)."""
    N, B, T, EL = SHAPES[0]
    env, cfg = _env(n_agents=N, n_envs=B, episode_length=EL, seed=SEED)
    ocfg = br.make_cfg(**{k: v for k, v in cfg.to_dict().items() if k in br.DEFAULTS})
    acts = _acts(N, B, T)
    env.reset(seed=SEED)
    env.capture(acts, T - 1, slot=0, kernels="both")
    env.replay(0)
    torch.cuda.synchronize()
    st = {k: v.detach().cpu().numpy() for k, v in env.get_state().items()}
    ref_st = dict(pos=st["pos"].astype(np.float64), vel=st["vel"].astype(np.float64),
                  step=st["step_count"], episode=st["episode"],
                  ep_acc=st["ep_acc"].astype(np.float64), ep_last=st["ep_last"].astype(np.float64))
    nst, ob = br.step(ocfg, ref_st, acts[T - 1].cpu().numpy(), 1, np.float64, seed=SEED)
    env.reset(seed=SEED)
    env.capture(acts, T, slot=1, kernels="roll")
    env.replay(1)
    torch.cuda.synchronize()
    assert not env.roll_gave_up()
    got = {k: v.detach().cpu().numpy() for k, v in env.t.items()}
    check_state(got["pos"], nst["pos"], "pos roll")
    check_state(got["vel"], nst["vel"], "vel roll")
    assert np.array_equal(got["step_count"], nst["step"])
    assert np.array_equal(got["episode"], nst["episode"])
    assert np.array_equal(got["done"].astype(bool), ob["done"].astype(bool))
    assert np.allclose(got["reward"], ob["reward"], rtol=3e-7, atol=2e-6)
    ptr, ei, attr = br.edges(ocfg, got["pos"], np.float32)
    assert np.array_equal(got["edge_ptr"], ptr)
    assert np.array_equal(got["edge_index"][:, :ptr[-1]], ei)
    env.close()
