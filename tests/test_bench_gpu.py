"""GPU (-m gpu): a plain `bench.py` run -- exactly --steps timed steps, the headline keys only, and --dump-outputs holding what the
last timed step returned (checked against the same model called here on the same seeded inputs)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B, T1, T2 = 2, 24, 70


def test_plain_run_times_k_steps_and_dumps_the_last_outputs(tmp_path):
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
                          "--test-shape", f"{B},{T1},{T2}", "--dump-outputs", str(tmp_path)], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-3000:]
    lines = [ln for ln in out.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, out.stdout[-2000:]
    rec = json.loads(lines[0])
    assert rec["steps"] == 3 and rec["warmup"] == 1 and rec["higher_is_better"] is True and rec["unit"] == "mel-frames/s" and rec["dtype"] == "bf16"
    assert rec["ms_per_step"] > 0 and abs(rec["value"] - B * T2 / (rec["ms_per_step"] * 1e-3)) <= 1e-6 * rec["value"]
    assert not {"cpu_baseline", "parity_mode", "call_modes", "train32", "long16", "stock_gpu_baseline"} & set(rec) and rec["roofline"] is None
    shapes = dict(loss=(), mel_loss=(), duration_loss=(), imv=(B, T2), reconst_alpha=(B, T1, T2), mel_pred=(B, T2, 80))
    assert sorted(os.listdir(tmp_path)) == sorted(n + ".npy" for n in shapes)
    got = {n: np.load(tmp_path / (n + ".npy")) for n in shapes}
    for n, shp in shapes.items():
        assert got[n].dtype == np.float32 and got[n].shape == shp and np.isfinite(got[n]).all(), n
    assert float(got["loss"]) == np.float32(rec["loss"])
    # the same model, weights and inputs as bench.py's run, called once here
    import bench
    from efficient_tts_amd import EfficientTTSCNN
    dev = torch.device("cuda:0")
    text, tl, mel, sl = bench.synth(B, T1, T2, 1234, dev)
    torch.manual_seed(0)
    m = EfficientTTSCNN(num_symbols=76, dropout_rate=0.0, use_masking=True, use_weighted_masking=False, sigma=0.01, precision="bf16").to(dev).eval()
    with torch.no_grad():
        want = {k: v.float().cpu().numpy() for k, v in bench.forward_outputs(m(text, tl, mel, sl)).items()}
    for n in shapes:
        scale = max(float(np.abs(want[n]).max()), 1.0)
        assert float(np.abs(got[n] - want[n]).max()) <= 1e-4 * scale, n
