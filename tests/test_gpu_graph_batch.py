"""GraphRolloutBuffer.graph_batch_csr (gsm_graph_batch_ptr +
gsm_graph_batch_gather) against the torch path it stands in for, run on the same
buffer: graph_batch, then gnn.env_csr, then gnn.csr_transpose. Every tensor has
to be equal bit for bit. The error paths (truncated slot, bad index, a stored
graph that is not symmetric or leaves its env) raise, or with check=False
report a status and keep every index in range."""
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _filled(T, **kw):
    """A buffer stepped T times with random actions; (env, buf)."""
    from gsmarl_amd import EnvConfig, GpuBatchEnv, GraphRolloutBuffer
    per_env = kw.pop("edges_per_env", None)
    env = GpuBatchEnv(EnvConfig(**kw), DEV)
    buf = GraphRolloutBuffer(env, episode_length=T, edges_per_env=per_env)
    buf.reset(seed=kw.get("seed", 0))
    g = torch.Generator(device=DEV).manual_seed(5)
    for _ in range(T):
        buf.insert(torch.randint(0, 5, (env.B, env.N), dtype=torch.int32, device=DEV, generator=g))
    torch.cuda.synchronize()
    return env, buf


def _bits(x):
    return x.view(torch.int32) if x.dtype == torch.float32 else x


def _same(a, b, what):
    assert a.dtype == b.dtype and a.shape == b.shape, (what, a.dtype, b.dtype, a.shape, b.shape)
    assert torch.equal(_bits(a), _bits(b)), what


def _parent(buf, t_idx, b_idx):
    """The composition of the three torch steps."""
    from gsmarl_amd import gnn
    g = buf.graph_batch(t_idx, b_idx)
    n = len(t_idx) * buf.E
    row_ptr = gnn.env_csr(g["edge_index"], n)
    col = g["edge_index"][1].to(torch.int32)
    return g, row_ptr, col, gnn.csr_transpose(row_ptr, col)


def _check(buf, t_idx, b_idx):
    t_idx, b_idx = torch.as_tensor(t_idx), torch.as_tensor(b_idx)
    g, row_ptr, col, (t_ptr, t_edge, t_tgt) = _parent(buf, t_idx, b_idx)
    c = buf.graph_batch_csr(t_idx, b_idx)
    _same(c["node_feat"], g["node_feat"], "node_feat")
    _same(c["row_ptr"], row_ptr, "row_ptr")
    _same(c["col"], col, "col")
    _same(c["edge_attr"], g["edge_attr"], "edge_attr")
    _same(c["ptr"], g["ptr"], "ptr")
    assert c["transpose"][0] is c["row_ptr"] and c["transpose"][2] is c["col"]
    _same(c["transpose"][0], t_ptr, "t_ptr")
    _same(c["transpose"][1], t_edge, "t_edge")
    _same(c["transpose"][2], t_tgt, "t_tgt")
    assert int(c["status"].item()) == 0
    nt = buf.graph_batch_csr(t_idx, b_idx, transpose=False, check=False)
    assert nt["transpose"] is None
    _same(nt["col"], col, "col (no transpose)")
    _same(nt["row_ptr"], row_ptr, "row_ptr (no transpose)")
    return c


@pytest.fixture(scope="module")
def small():
    env, buf = _filled(3, n_agents=3, n_envs=50, seed=8, episode_length=2)
    yield buf
    env.close()


# slot 0 and slot T, env 0 and env B-1, (3, 49) twice
T7 = [0, 3, 1, 3, 0, 2, 3]
B7 = [0, 49, 17, 49, 49, 0, 5]


@pytest.mark.parametrize("K", [1, 5, 7])
def test_three_agents(small, K):
    assert small.E == 9
    _check(small, T7[:K], B7[:K])
    _check(small, T7[-K:], B7[-K:])


def test_six_agents():
    env, buf = _filled(5, n_agents=6, n_envs=20, seed=8, episode_length=4)
    _check(buf, [0, 3, 5, 5, 1], [7, 0, 19, 2, 7])
    env.close()


def test_full_rows_longer_than_the_staging_buffer():
    """24 agents laid out in a 0.3 x 0.3 world: every agent and obstacle sees
    every other, 2304 entries per env (the capacity) in rows of 47 and 48; the
    slot after a step (the contacts push them apart) is still far longer than
    the staging buffer."""
    env, buf = _filled(1, n_agents=24, n_envs=3, seed=2, world_half=0.15, edges_per_env=2304)
    assert buf.cap == 3 * 2304 and not bool(buf.overflowed())
    cnt = buf.edge_ptr[:, 1:] - buf.edge_ptr[:, :-1]
    assert bool(cnt[0].eq(2304).all()) and int(cnt[1].min()) > 512
    _check(buf, [1, 0, 1, 0, 1], [2, 0, 0, 1, 2])
    c = _check(buf, [0, 0, 0], [2, 0, 1])
    deg = c["row_ptr"][1:] - c["row_ptr"][:-1]
    assert set(deg.unique().tolist()) == {1, 47, 48}        # goals: their agent only
    env.close()


def test_eighty_agents_tile_path():
    env, buf = _filled(1, n_agents=80, n_envs=2, seed=3)
    assert buf.E == 240 and not bool(buf.overflowed())
    _check(buf, [1, 0, 1], [1, 1, 0])
    env.close()


def test_mixed_padded_nodes_and_empty_rows():
    env, buf = _filled(2, scenario="mixed", n_agents=12, n_envs=48, seed=4)
    c = _check(buf, [0, 2, 1, 2, 0, 1, 2, 2, 0], [0, 47, 13, 47, 30, 5, 21, 8, 46])
    assert bool(((c["row_ptr"][1:] - c["row_ptr"][:-1]) == 0).any())
    env.close()


def test_sample_without_entries(small):
    """A hand-written slot: its envs hold no edges."""
    keep = small.edge_ptr[2].clone()
    try:
        small.edge_ptr[2].zero_()
        c = _check(small, [2], [4])
        assert c["col"].numel() == 0 and c["row_ptr"].eq(0).all()
        _check(small, [1, 2, 2, 3, 2], [3, 0, 49, 7, 11])
        small.edge_ptr[2].fill_(5)                           # offsets 5..5: still no entries
        _check(small, [2, 0, 2], [0, 9, 49])
    finally:
        small.edge_ptr[2].copy_(keep)


# gsm_graph_batch_ptr's scan: 8 samples a thread, 512 a wave, 8192 a chunk (one
# workgroup of 1024 threads), a cross-wave sum in LDS and a carry between chunks
SCAN_WAVE, SCAN_CHUNK = 512, 8192


def _many(buf, K, seed=0):
    """K random samples of `buf`, with (0, 0) and (T, B-1) alternating at the
    first and last sample and on both sides of the first wave and chunk
    boundaries."""
    gen = torch.Generator().manual_seed(1000 + K + seed)
    t = torch.randint(0, buf.T + 1, (K,), generator=gen)
    b = torch.randint(0, buf.B, (K,), generator=gen)
    spots = [p for p in (0, SCAN_WAVE - 1, SCAN_WAVE, SCAN_CHUNK - 1, SCAN_CHUNK, K - 1) if p < K]
    for i, p in enumerate(spots):
        t[p], b[p] = (0, 0) if i % 2 == 0 else (buf.T, buf.B - 1)
    return t, b


@pytest.mark.parametrize("K", [513, 8192, 8193, 8709, 16387])
def test_scan_across_waves_and_chunks(small, K):
    """More samples than two threads hold: the wave scan beyond lane 1, the
    cross-wave sum (K > 512) and the carry into a second and a third chunk
    (K > 8192, K > 16384), each with a ragged end."""
    assert small.E == 9 and (small.T, small.B) == (3, 50)
    c = _check(small, *_many(small, K))
    assert c["ptr"].numel() == K + 1 and c["node_feat"].shape[0] == K * 9


def test_scan_with_empty_samples_at_the_boundaries(small):
    """Slot 2 without entries: about a quarter of the samples count zero, on
    both sides of the wave and chunk boundaries."""
    K = 8709
    t, b = _many(small, K, seed=1)
    for p in (SCAN_WAVE - 2, SCAN_WAVE + 1, SCAN_CHUNK - 2, SCAN_CHUNK + 1, K - 2):
        t[p] = 2
    assert int((t == 2).sum()) > K // 8
    keep = small.edge_ptr[2].clone()
    try:
        small.edge_ptr[2].zero_()
        c = _check(small, t, b)
        cnt = c["ptr"][1:] - c["ptr"][:-1]
        assert bool((cnt[(t == 2).to(cnt.device)] == 0).all()) and bool((cnt[(t != 2).to(cnt.device)] > 0).any())
    finally:
        small.edge_ptr[2].copy_(keep)


def test_bad_sample_in_the_second_chunk(small):
    """One bad index, and one truncated sample, at k = 8200 among valid ones:
    the status bits of a thread far from the first reach the host."""
    K, k_bad = 8709, 8200
    t, b = _many(small, K, seed=2)
    for tb, bb in ((4, 0), (0, 50), (-1, 3)):
        t2, b2 = t.clone(), b.clone()
        t2[k_bad], b2[k_bad] = tb, bb
        with pytest.raises(IndexError):
            small.graph_batch_csr(t2, b2)
    _check(small, t[k_bad - 3:k_bad + 3], b[k_bad - 3:k_bad + 3])   # the samples around it are valid
    env, buf = _filled(1, n_agents=24, n_envs=32, seed=5, edges_per_env=8)
    try:
        assert bool(buf.overflowed())
        whole = (buf.edge_ptr[:, 1:] <= buf.cap).nonzero()       # (t, b) of the samples inside the capacity
        cut = (buf.edge_ptr[:, 1:] > buf.cap).nonzero()
        assert whole.shape[0] >= 2 and cut.shape[0] >= 1
        pick = torch.randint(0, whole.shape[0], (K,), generator=torch.Generator().manual_seed(3))
        t, b = whole[:, 0].cpu()[pick], whole[:, 1].cpu()[pick]
        assert int(buf.graph_batch_csr(t, b)["status"].item()) == 0
        t[k_bad], b[k_bad] = int(cut[-1, 0]), int(cut[-1, 1])
        with pytest.raises(ValueError, match="capacity"):
            buf.graph_batch_csr(t, b)
    finally:
        env.close()


def test_no_samples(small):
    e = torch.zeros(0, dtype=torch.int64)
    c = small.graph_batch_csr(e, e)
    assert c["row_ptr"].tolist() == [0] and c["ptr"].tolist() == [0]
    assert c["node_feat"].shape == (0, 7) and c["col"].numel() == 0 and c["edge_attr"].numel() == 0
    assert c["col"].dtype == torch.int32 and c["transpose"][1].numel() == 0
    assert all(v.device.type == "cuda" for v in (c["node_feat"], c["row_ptr"], c["col"], c["edge_attr"]))


def test_truncated_slot_raises():
    env, buf = _filled(1, n_agents=24, n_envs=32, seed=5, edges_per_env=8)
    assert bool(buf.overflowed())
    with pytest.raises(ValueError, match="capacity"):
        buf.graph_batch_csr(torch.tensor([0]), torch.tensor([31]))
    env.close()


@pytest.mark.parametrize("t,b", [(4, 0), (0, 50), (-1, 0), (0, -1), (1 << 40, 3)])
def test_index_out_of_range_raises(small, t, b):
    with pytest.raises(IndexError):
        small.graph_batch_csr(torch.tensor([1, t, 2]), torch.tensor([5, b, 6]))


@pytest.mark.parametrize("how", ["no_reverse", "other_env"])
def test_overwritten_target_is_reported(small, how):
    """One stored dst changed in place (in-bounds data, restored afterwards):
    the graph is no longer symmetric, or an entry points into another env."""
    t, b, E = 1, 17, small.E
    lo, hi = int(small.edge_ptr[t, b]), int(small.edge_ptr[t, b + 1])
    assert hi - lo >= 2
    keep = small.edge_index[t].clone()
    src, dst = int(keep[0, lo]) - b * E, int(keep[1, lo]) - b * E
    try:
        if how == "no_reverse":
            new = next(x for x in range(E) if x not in (src, dst))
            small.edge_index[t, 1, lo] = b * E + new
        else:
            small.edge_index[t, 1, lo] = (b + 1) * E + dst
        t_idx, b_idx = torch.tensor([0, t, 3]), torch.tensor([2, b, 49])
        with pytest.raises(RuntimeError, match="invalid"):
            small.graph_batch_csr(t_idx, b_idx)
        c = small.graph_batch_csr(t_idx, b_idx, check=False)
        assert int(c["status"].item()) != 0
        n, total = 3 * E, int(c["ptr"][-1])
        assert c["col"].numel() == total and c["transpose"][1].numel() == total
        assert int(c["col"].min()) >= 0 and int(c["col"].max()) < n
        assert int(c["transpose"][1].min()) >= 0 and int(c["transpose"][1].max()) < total
        assert int(c["row_ptr"][0]) == 0 and int(c["row_ptr"][-1]) == total
        assert bool((c["row_ptr"][1:] >= c["row_ptr"][:-1]).all())
    finally:
        small.edge_index[t].copy_(keep)
    _check(small, [0, t, 3], [2, b, 49])                     # restored: clean again


def test_transformer_conv_trains_on_the_assembled_batch(small):
    """The returned transpose drives the HIP backward exactly as
    csr_transpose's arrays do: same output and parameter gradients, bitwise."""
    from gsmarl_amd import gnn
    c = small.graph_batch_csr(torch.tensor(T7), torch.tensor(B7))
    ref_tr = gnn.csr_transpose(c["row_ptr"], c["col"])
    torch.manual_seed(0)
    conv = gnn.TransformerConv(7, 16, heads=2, kernel_backward=True).to(DEV)
    w = torch.randn(c["node_feat"].shape[0], 32, device=DEV)
    runs = []
    for tr in (c["transpose"], ref_tr):
        conv.zero_grad(set_to_none=True)
        y = conv(c["node_feat"], c["row_ptr"], c["col"], c["edge_attr"].reshape(-1, 1), transpose=tr)
        assert "AttnAggregate" in type(y.grad_fn).__name__
        (y * w).sum().backward()
        runs.append([("out", y.detach().clone())] + [(k, p.grad.clone()) for k, p in conv.named_parameters()])
    assert len(runs[0]) == len(runs[1]) > 1
    for (name, a), (_, b) in zip(*runs):
        assert torch.isfinite(a).all(), name
        _same(a, b, name)
