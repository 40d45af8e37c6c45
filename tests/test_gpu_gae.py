"""GraphRolloutBuffer.compute_returns(kernel=True) (gsm_gae: the whole GAE
recursion in one launch) is the torch loop bit for bit: every operation of the
loop is one correctly rounded fp32 operation and the kernel does the same ones
in the same order (the library is built without fp contraction). Checked
against the loop restated here on CPU copies of the same tensors, and against
compute_returns(kernel=False) on the GPU."""
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GAMMA, LAM = 0.99, 0.95


def _loop(r, values, done, gamma, lam):
    """compute_returns' loop on whatever device the tensors live on."""
    T = r.shape[0]
    masks = (1.0 - done.to(torch.float32)).unsqueeze(-1).expand(-1, -1, r.shape[2])
    ret = torch.empty_like(r)
    gae = torch.zeros_like(r[0])
    for t in reversed(range(T)):
        delta = r[t] + gamma * values[t + 1] * masks[t + 1] - values[t]
        gae = delta + gamma * lam * masks[t + 1] * gae
        ret[t] = gae + values[t]
    return ret


# the slot loop is unrolled by four: T = 2, 3, 7, 11 leave remainders 2 and 3, with and without a full trip
@pytest.mark.parametrize("N,B,T,ep", [(3, 7, 1, 100), (6, 20, 5, 2), (3, 101, 4, 2),
                                      (3, 7, 2, 100), (6, 20, 3, 2), (3, 101, 7, 3), (3, 9, 11, 4)])
def test_kernel_returns_are_the_loop_bit_for_bit(N, B, T, ep):
    from gsmarl_amd import EnvConfig, GpuBatchEnv, GraphRolloutBuffer
    env = GpuBatchEnv(EnvConfig(n_agents=N, n_envs=B, seed=8, episode_length=ep), DEV)
    buf = GraphRolloutBuffer(env, episode_length=T)
    buf.reset(seed=8)
    g = torch.Generator(device=DEV).manual_seed(2)
    for _ in range(T):
        buf.insert(torch.randint(0, 5, (B, N), dtype=torch.int32, device=DEV, generator=g))
    if ep < T:      # done flags inside the window, and on the last slot where ep divides T
        assert int(buf.done[1:T].sum()) > 0
    if T % ep == 0:
        assert bool(buf.done[T].all())
    values = torch.randn(T + 1, B, N, device=DEV, generator=g)
    for which, stored in (("reward", buf.reward), ("cost", buf.cost)):
        got = buf.compute_returns(values, GAMMA, LAM, which=which, kernel=True)
        assert got.shape == (T, B, N) and got.dtype == torch.float32
        cpu = _loop(stored[1:].cpu(), values.cpu(), buf.done.cpu(), GAMMA, LAM)
        assert torch.equal(got.cpu().view(torch.int32), cpu.view(torch.int32)), which
        ref = buf.compute_returns(values, GAMMA, LAM, which=which)
        assert torch.equal(got.view(torch.int32), ref.view(torch.int32)), which
        assert bool(got.abs().sum() > 0)
    env.close()


def test_kernel_rejects_a_wrong_value_shape():
    from gsmarl_amd import EnvConfig, GpuBatchEnv, GraphRolloutBuffer
    env = GpuBatchEnv(EnvConfig(n_agents=3, n_envs=4, seed=1), DEV)
    buf = GraphRolloutBuffer(env, episode_length=2)
    buf.reset(seed=1)
    with pytest.raises(ValueError):
        buf.compute_returns(torch.zeros(2, 4, 3, device=DEV), kernel=True)
    env.close()
