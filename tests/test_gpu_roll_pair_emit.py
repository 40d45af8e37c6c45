"""The edge emission of the two-envs-per-wave rollout (gsm_roll_pair_kernel,
24 agents + 24 obstacles): both envs' rows staged as one list and written in
one loop from env 2w's offset, the goal rows stored by their agents' lanes.

Every case runs one rollout launch and compares every state and output buffer
(edge_ptr, edge_index, edge_attr, edge_count, node features, reward, cost,
done, pos, vel, masks, counters, ep_acc / ep_last; floats by their bits) with
the per-step chain of the same actions from the same injected state, and
requires the roll status to be 0 (the helpers of test_gpu_roll_states.py).

Shapes: B = 1 (a lone half), 2 (one full wave), 3 (an odd tail wave), 9 (a
partial second workgroup) with K = 1 (the tail's last emission alone), 2 (both
tail emissions), 3 (the first loop emission), 4 and 7 (all three position
buffers in rotation). States: a loose crowd (about 250 edges per env, the
combined list several passes long); envs 2w dense and 2w + 1 sparse and the
reverse (the boundary inside the combined list off the 64-lane pass boundary);
an agent with no neighbour (its row is the goal edge alone); crowds past the
scratch bound in env 2w only, in env 2w + 1 only and in both (asserted from
the edge counts: more than 7 E edges in the intended envs, fewer in the
others, so the per-lane path runs beside or instead of the combined list);
the two halves re-laid out on different steps of a K = 7 launch; a coincident
pair in one half; and one graph replayed three times with other work between
the replays."""
import numpy as np
import pytest
import torch

import roll_states as rs
import test_gpu_roll_states as trs

pytestmark = pytest.mark.gpu

N = 24
E = 3 * N
SCRATCH_EDGES = 7 * E      # an env's list (its N goal rows included) that still fits its share of the scratch
LOOSE_L = 1.5              # half-width of the loose crowd: ~4 neighbours per row


def _mixed(B, dense_envs, L_dense, L_sparse=rs.SPREAD_L, seed=3):
    """Envs of `dense_envs` from a crowd of half-width L_dense, the others from
    one of half-width L_sparse."""
    st = rs.crowd(N, N, B, L_sparse, seed=seed)
    dense = rs.crowd(N, N, B, L_dense, seed=seed + 1)
    for b in dense_envs:
        st["pos"][b], st["vel"][b] = dense["pos"][b], dense["vel"][b]
    return st


@pytest.mark.parametrize("K", [1, 2, 3, 4, 7])
@pytest.mark.parametrize("B", [1, 2, 3, 9])
def test_combined_list_equals_chain(B, K):
    got = trs._check(N, B, rs.crowd(N, N, B, LOOSE_L, seed=B), T=K, seed=B + K, episode_length=1000)
    cnt = got["edge_count"].cpu().numpy()
    assert (cnt > 2 * 64).all() and (cnt <= SCRATCH_EDGES).all()   # several passes, all on the staged path


@pytest.mark.parametrize("dense", ["even", "odd"])
def test_uneven_lists_equal_chain(dense):
    B = 9
    envs = range(0, B, 2) if dense == "even" else range(1, B, 2)
    got = trs._check(N, B, _mixed(B, envs, 1.1), T=4, seed=5, episode_length=1000)
    cnt = got["edge_count"].cpu().numpy().astype(np.int64)
    d = np.zeros(B, bool)
    d[list(envs)] = True
    assert (cnt <= SCRATCH_EDGES).all()                  # both halves staged
    assert cnt[d].min() > cnt[~d].max() + 2 * 64         # the dense halves' lists more than two passes longer
    assert len(set((cnt[0:B - 1:2] - N) % 64)) > 1       # the boundary between the lists moves within a pass


def test_isolated_agent_row_is_its_goal_edge():
    B = 9
    st = rs.crowd(N, N, B, LOOSE_L, seed=11)
    lone = {2: 0, 5: N - 1, 8: 7}                        # env: agent (a low half, a high half, the lone last half)
    for b, a in lone.items():
        st["pos"][b, a] = (40.0 + b, -40.0)
        st["pos"][b, N + a] = (40.0 + b, -39.0)
        st["vel"][b, a] = 0.0
        st["hold"][b, a] = True
    got = trs._check(N, B, st, T=4, seed=11, episode_length=1000)
    ptr = got["edge_ptr"].cpu().numpy()
    ei = got["edge_index"].cpu().numpy()
    for b, a in lone.items():
        assert int(got["row_mask"][b, a]) == 0
        src = ei[0, ptr[b]:ptr[b + 1]]
        dst = ei[1, ptr[b]:ptr[b + 1]]
        assert dst[src == b * E + a].tolist() == [b * E + N + a]     # the agent's row: the edge to its goal
        assert not (dst[src != b * E + N + a] == b * E + a).any()    # nobody else's row holds it


@pytest.mark.parametrize("crowded", ["even", "odd", "both"])
def test_crowd_past_the_scratch_equals_chain(crowded):
    """The crowd layout of test_gpu_roll_states.py in one half of every wave
    or in both: the last step's edge counts show that the intended envs'
    lists exceed the scratch bound (a crowd of half-width 0.3 holds about
    2000 edges for the whole launch) and the others' do not."""
    B = 9
    envs = {"even": range(0, B, 2), "odd": range(1, B, 2), "both": range(B)}[crowded]
    got = trs._check(N, B, _mixed(B, envs, rs.CROWD_L[N], LOOSE_L), T=4, seed=N + B, episode_length=1000)
    cnt = got["edge_count"].cpu().numpy()
    c = np.zeros(B, bool)
    c[list(envs)] = True
    assert (cnt[c] > SCRATCH_EDGES).all(), cnt
    assert (cnt[~c] <= SCRATCH_EDGES).all() and (cnt[~c] > 64).all(), cnt


def test_halves_reset_on_different_steps_of_the_launch():
    """K = 7, episode length 8: env 2w ends its episode on step k = 1 and env
    2w + 1 on k = 3 (wave 1 the other way round), so the emissions of steps
    k - 2 run before, between and after the two re-layouts of a wave."""
    B, K, EL = 9, 7, 8
    st = rs.crowd(N, N, B, LOOSE_L, seed=17)
    sc = np.where(np.arange(B) % 2 == 0, EL - 2, EL - 4)
    sc[2], sc[3] = EL - 4, EL - 2
    st["step_count"] = sc.astype(np.int32)
    got = trs._check(N, B, st, T=K, seed=17, episode_length=EL)
    assert got["episode"].tolist() == [1] * B
    first = np.where(sc == EL - 2, K - 2, K - 4)         # steps since the re-layout
    assert got["step_count"].cpu().numpy().tolist() == first.tolist()


@pytest.mark.parametrize("where", ["lo", "hi"])
def test_coincident_pair_in_one_half(where):
    B = rs.SHAPES["pair"][1]
    st = rs.coincident(N, N, B, where, seed=N, envs_per_block=8)
    got = trs._check(N, B, st, T=7, seed=N, episode_length=1000)
    envs = rs.where_envs(where, B, 8)
    deg = got["degenerate"].cpu().numpy()
    assert (deg[envs] == 1).all() and not np.delete(deg, envs).any()


def test_three_replays_with_other_work_between():
    B, K = 9, 4
    st = rs.crowd(N, N, B, LOOSE_L, seed=23)
    env, _ = trs._env(N, B, episode_length=6)
    other, _ = trs._env(N, 5, episode_length=6)
    acts = trs._dev_actions(rs.actions(K, B, N, seed=23), st["hold"], "index")
    oacts = torch.zeros((5, N), dtype=torch.int32, device=trs.DEV)
    ref = trs._run(env, st, acts, K, "both", replays=3)
    trs._inject(env, st)
    other.reset(seed=1)
    env.capture(acts, K, slot=1, kernels="roll")
    assert env.graph_is_rollout(1)
    x = torch.ones((256, 256), device=trs.DEV)
    for _ in range(3):
        env.replay(1)
        for _ in range(3):                               # another env's steps and a matmul in the stream
            other.step(oacts, sync_edges=False)
        x = (x @ x) * (1.0 / 256.0)
    torch.cuda.synchronize()
    assert env.roll_gave_up() == 0
    got = trs._snapshot(env)
    for k in ref:
        assert torch.equal(trs._bits(ref[k]), trs._bits(got[k])), k
    assert float(x[0, 0]) == 1.0
    env.close()
    other.close()
