"""bench.dump_outputs (no GPU): every array as float32, or float64 where
float32 would lose it; arrays over their share of the byte budget as a fixed
sample of their elements, the same from run to run; and the plain line's
options parse (`--full` off by default)."""
import numpy as np
import torch

import bench


def _outs():
    g = torch.Generator().manual_seed(5)
    return dict(node_feat=torch.randn(40, 9, 7, generator=g),
                done=torch.tensor([0, 1, 1, 0], dtype=torch.uint8),
                edge_ptr=torch.tensor([0, 3, 1 << 30], dtype=torch.int64),
                edge_index=torch.arange(24, dtype=torch.int32).reshape(2, 12),
                lsa_v=torch.linspace(0, 1, 7, dtype=torch.float64))


def test_dump_keeps_values_and_picks_the_float_type(tmp_path):
    outs = _outs()
    bench.dump_outputs(tmp_path, outs)
    assert sorted(p.name for p in tmp_path.iterdir()) == sorted(f"{k}.npy" for k in outs)
    for k, t in outs.items():
        a = np.load(tmp_path / f"{k}.npy")
        wide = k in ("edge_ptr", "lsa_v")   # int64 past 2^24, float64 data
        assert a.dtype == (np.float64 if wide else np.float32), k
        assert a.shape == tuple(t.shape), k
        assert np.array_equal(a, t.numpy().astype(a.dtype)), k
    assert np.load(tmp_path / "edge_ptr.npy")[2] == float(1 << 30)


def test_dump_samples_what_does_not_fit_the_same_way_every_run(tmp_path, monkeypatch):
    outs = _outs()
    monkeypatch.setattr(bench, "DUMP_BUDGET", 2000)
    bench.dump_outputs(tmp_path / "a", outs)
    bench.dump_outputs(tmp_path / "b", outs, prefix="rank1_")
    total = 0
    for k, t in outs.items():
        a = np.load(tmp_path / "a" / f"{k}.npy")
        assert np.array_equal(a, np.load(tmp_path / "b" / f"rank1_{k}.npy")), k
        total += a.nbytes
        if k != "node_feat":   # the small ones fit whole
            assert a.shape == tuple(t.shape), k
    assert total <= 2000
    s = np.load(tmp_path / "a" / "node_feat.npy")
    flat = outs["node_feat"].numpy().reshape(-1)
    assert s.ndim == 1 and 0 < s.size < flat.size
    # a sample of the array's own elements, in their order
    idx = np.sort(np.random.default_rng(0).choice(flat.size, s.size, replace=False))
    assert np.array_equal(s, flat[idx])


def test_full_is_off_by_default():
    a = bench.parse_args(["--gpus", "1", "--steps", "20", "--warmup", "5"])
    assert a.full is False and a.dump_outputs is None and a.steps == 20 and a.warmup == 5
    a = bench.parse_args(["--full", "--dump-outputs", "d"])
    assert a.full is True and a.dump_outputs == "d"
