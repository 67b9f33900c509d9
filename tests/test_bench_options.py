"""bench.py's options: a plain run selects the headline inference only, --full what the default run did before, and
--dump-outputs writes float32 arrays at seeded positions within the size budget.  Host logic only."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def test_plain_run_is_the_headline_only():
    import bench
    a = bench.parse_args(["--gpus", "1", "--steps", "7", "--warmup", "2"])
    assert (a.mode, a.full, a.steps, a.warmup, a.dump_outputs) == ("infer", False, 7, 2, None)


def test_full_restores_every_mode():
    import bench
    a = bench.parse_args(["--gpus", "1", "--steps", "7", "--warmup", "2", "--full"])
    assert a.mode == "both" and a.full and not a.no_sustained and not a.no_cpu_baseline
    assert bench.parse_args(["--full", "--mode", "train"]).mode == "train"
    assert bench.parse_args(["--mode", "x4"]).mode == "x4"


def test_bad_arguments_are_refused():
    import bench
    with pytest.raises(SystemExit):
        bench.parse_args(["--steps", "0"])
    with pytest.raises(SystemExit):
        bench.parse_args(["--mode", "train", "--dump-outputs", "out"])


def test_dump_outputs(tmp_path):
    import bench
    y = torch.rand((3, 3) + bench.OUT, generator=torch.Generator().manual_seed(5))
    bench.dump_outputs(y, str(tmp_path / "a"))
    bench.dump_outputs(y.clone(), str(tmp_path / "b"))
    names = sorted(os.listdir(tmp_path / "a"))
    assert names == ["output_image0.npy", "output_sample.npy"]
    total = 0
    for n in names:
        a, b = np.load(tmp_path / "a" / n), np.load(tmp_path / "b" / n)
        assert a.dtype == np.float32 and np.array_equal(a, b)           # same output -> same files (the positions are seeded)
        total += os.path.getsize(tmp_path / "a" / n)
    assert total <= 64 << 20
    assert np.array_equal(np.load(tmp_path / "a" / "output_image0.npy"), y[0].numpy())
    s = np.load(tmp_path / "a" / "output_sample.npy")
    assert s.shape == (bench.DUMP_SAMPLE,) and np.isin(s, y.numpy()).all()
