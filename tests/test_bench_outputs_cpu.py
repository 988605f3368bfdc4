"""bench.py's --dump-outputs writer and the --full switch, on the CPU: arrays within the
budget are written whole in float32, a larger one as a fixed sample (the same indices on
every call), and the files never exceed the budget together."""
import glob
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import bench  # noqa: E402


def test_dump_writes_small_arrays_whole(tmp_path):
    g = torch.arange(12, dtype=torch.float64).reshape(3, 4) / 7
    bench.dump_outputs(str(tmp_path / "d"), {"aggregate": g, "iters": torch.tensor([5.0])})
    a = np.load(tmp_path / "d" / "aggregate.npy")
    assert a.dtype == np.float32 and a.shape == (3, 4)
    assert np.array_equal(a, g.to(torch.float32).numpy())
    assert np.array_equal(np.load(tmp_path / "d" / "iters.npy"), np.float32([5.0]))


def test_dump_samples_over_budget_the_same_way_every_time(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "DUMP_BUDGET_BYTES", 4000)          # 1000 float32 in all
    big = torch.arange(5000, dtype=torch.float32)
    arrays = {"big": big, "other": big.flip(0).clone(), "small": torch.ones(10)}
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), arrays, "_rank1")
    files = sorted(os.path.basename(f) for f in glob.glob(str(tmp_path / "a" / "*.npy")))
    assert files == ["big_rank1.npy", "other_rank1.npy", "small_rank1.npy"]
    total = 0
    for f in files:
        x, y = np.load(tmp_path / "a" / f), np.load(tmp_path / "b" / f)
        assert x.dtype == np.float32 and np.array_equal(x, y)
        total += x.nbytes
    assert total <= 4000
    assert np.load(tmp_path / "a" / "small_rank1.npy").shape == (10,)    # whole
    s = np.load(tmp_path / "a" / "big_rank1.npy")
    # the small array's unused share goes to the large ones: (1000 - 10) // 2 elements each,
    # distinct elements of the array in index order
    assert s.shape == (495,) and np.all(np.diff(s) > 0) and s.min() >= 0 and s.max() < 5000
    o = np.load(tmp_path / "a" / "other_rank1.npy")
    assert np.array_equal(o, 4999 - s)                             # the same indices


def test_full_is_off_by_default(monkeypatch):
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1", "--steps", "7", "--warmup", "2"])
    a = bench.parse()
    assert a.full is False and a.dump_outputs is None and a.steps == 7 and a.warmup == 2
    monkeypatch.setattr(sys, "argv", ["bench.py", "--full", "--dump-outputs", "x"])
    a = bench.parse()
    assert a.full is True and a.dump_outputs == "x"
