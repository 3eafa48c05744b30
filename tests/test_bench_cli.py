"""CPU: bench.py's command line - a plain run times exactly --steps steps in one region and measures nothing beyond the
headline; --full brings back the seven regions and the extra objects; --dump-outputs writes float32 .npy files, a fixed
sample of an array that is too large."""
import numpy as np
import torch

import bench


def test_plain_run_is_one_region_full_run_seven():
    a = bench.parse_args(["--gpus", "1", "--steps", "20", "--warmup", "5"])
    assert a.steps == 20 and a.warmup == 5 and a.regions == 1 and not a.full and a.dump_outputs == ""
    f = bench.parse_args(["--full", "--steps", "20"])
    assert f.full and f.regions == 7
    assert bench.parse_args(["--regions", "3"]).regions == 3
    assert bench.parse_args(["--full", "--regions", "5"]).regions == 5


def test_dump_outputs_float32_and_a_fixed_sample_of_large_arrays(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "DUMP_MAX_ELEMS", 64)
    big = torch.arange(1000, dtype=torch.float64)
    small = torch.tensor([[0.25, 0.75]], dtype=torch.float32)
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), {"big": big, "small": small, "loss": torch.tensor([0.5])})
    assert sorted(p.name for p in (tmp_path / "a").iterdir()) == ["big.npy", "loss.npy", "small.npy"]
    s = np.load(tmp_path / "a" / "small.npy")
    assert s.dtype == np.float32 and s.shape == (1, 2) and np.array_equal(s, small.numpy())
    b = np.load(tmp_path / "a" / "big.npy")
    assert b.dtype == np.float32 and b.shape == (64,)
    assert np.all(np.diff(b) > 0) and set(b.tolist()) <= set(range(1000))       # sorted distinct elements of the array
    assert np.array_equal(b, np.load(tmp_path / "b" / "big.npy"))                # the same sample every run
