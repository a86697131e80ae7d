"""bench.py without a GPU: what a plain run switches on, what --full switches on, and the --dump-outputs writer."""
import os

import numpy as np
import torch

import bench

EXTRAS = ("parity_mode", "call_modes", "train_record", "sub_records", "stock_gpu", "measure_traffic")


def test_plain_run_leaves_every_extra_off_and_full_turns_them_on():
    a = bench.parse(["--gpus", "1", "--steps", "7", "--warmup", "3"])
    assert a.steps == 7 and a.warmup == 3 and not a.full and a.dump_outputs == ""
    assert all(getattr(a, k) == 0 for k in EXTRAS) and a.no_cpu_baseline
    f = bench.parse(["--full"])
    assert all(getattr(f, k) == 1 for k in EXTRAS) and not f.no_cpu_baseline
    # an explicit switch wins either way (the A/B and profiling command lines keep their meaning)
    g = bench.parse(["--full", "--parity-mode", "0", "--no-cpu-baseline"])
    assert g.parity_mode == 0 and g.no_cpu_baseline and g.train_record == 1
    assert bench.parse(["--call-modes", "1"]).call_modes == 1


def test_dump_outputs_writes_float32_and_samples_the_same_elements_over_budget(tmp_path):
    arrays = dict(loss=torch.tensor(2.5, dtype=torch.float64), mel=torch.randn(4, 50, 8), alpha=torch.rand(4, 6, 50).to(torch.bfloat16))
    bench.dump_outputs(str(tmp_path / "all"), arrays)
    got = {n: np.load(tmp_path / "all" / (n + ".npy")) for n in arrays}
    assert all(v.dtype == np.float32 for v in got.values())
    assert got["loss"].shape == () and float(got["loss"]) == 2.5
    assert np.array_equal(got["mel"], arrays["mel"].numpy()) and np.array_equal(got["alpha"], arrays["alpha"].float().numpy())
    budget = 2000
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), arrays, budget=budget)
    sizes = 0
    for n in arrays:
        x, y = np.load(tmp_path / "a" / (n + ".npy")), np.load(tmp_path / "b" / (n + ".npy"))
        assert x.dtype == np.float32 and np.array_equal(x, y)
        sizes += x.nbytes
    assert sizes <= budget
    mel = np.load(tmp_path / "a" / "mel.npy")
    assert 0 < mel.size < arrays["mel"].numel() and np.isin(mel, arrays["mel"].numpy()).all()
    assert sorted(os.listdir(tmp_path / "a")) == ["alpha.npy", "loss.npy", "mel.npy"]
