"""Timing of duration control and align() (MI355X), interleaved arms in one process, median of N calls each:

  1. inference_batch at B = 64 (T1 = 128, bf16x3): the plain call against the controlled one (a [B] length_scale of ones and
     return_durations: the efts_duration_control launch instead of efts_duration_positions, same mel length, same launch count);
  2. align() against forward() at B = 64 x (128, 800), precision bf16: align() stops after the IMV (no duration predictor, no
     decoder, no mel head, no losses).

    python tools/gpu_time_duration_control.py [--calls 30]
Prints one JSON line."""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from efficient_tts_amd import EfficientTTSCNN  # noqa: E402
from oracle import efts_oracle as O  # noqa: E402


def _model(precision):
    m = EfficientTTSCNN(num_symbols=76, dropout_rate=0.0, use_masking=True, sigma=0.01, precision=precision)
    m.load_state_dict(O.fill_params())
    return m.cuda().eval()


def _interleaved(arms, calls, warmup=3):
    """arms: name -> fn; every round runs each arm once, synchronised; returns name -> median ms"""
    for _ in range(warmup):
        for fn in arms.values():
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in arms}
    for _ in range(calls):
        for k, fn in arms.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            times[k].append((time.perf_counter() - t0) * 1e3)
    return {k: statistics.median(v) for k, v in times.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=30)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    gen = torch.Generator().manual_seed(0)
    B, T1, T2 = 64, 128, 800
    text = torch.randint(1, 76, (B, T1), generator=gen).to(dev)
    tl = torch.randint(T1 // 2, T1 + 1, (B,), generator=gen).to(dev)
    res = {}
    with torch.no_grad():
        m = _model("bf16x3")
        ones = torch.ones(B, device=dev)
        plain = m.inference_batch(text, tl)
        ctl = m.inference_batch(text, tl, length_scale=ones, return_durations=True)
        assert torch.equal(plain[1], ctl[1]) and torch.equal(plain[0], ctl[0])
        t = _interleaved({"plain": lambda: m.inference_batch(text, tl),
                          "controlled": lambda: m.inference_batch(text, tl, length_scale=ones, return_durations=True)}, a.calls)
        res["inference_batch_B64"] = dict(plain_ms=t["plain"], controlled_ms=t["controlled"], ratio=t["controlled"] / t["plain"],
                                          max_T2=int(plain[1].max()))
        del m
        m = _model("bf16")
        mel = torch.randn(B, T2, 80, generator=gen).to(dev)
        sl = torch.full((B,), T2, dtype=torch.int64, device=dev)
        tlf = torch.full((B,), T1, dtype=torch.int64, device=dev)
        t = _interleaved({"forward": lambda: m(text, tlf, mel, sl), "align": lambda: m.align(text, tlf, mel, sl)}, a.calls)
        res["align_vs_forward_B64_128x800_bf16"] = dict(forward_ms=t["forward"], align_ms=t["align"], ratio=t["align"] / t["forward"])
    print(json.dumps(res))


if __name__ == "__main__":
    main()
