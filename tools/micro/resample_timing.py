"""Time the on-device sample-rate converter against stock PyTorch on the same GPU; writes profiles/resample_timing.json.

Workload: 64 x 10 s of 48 kHz int16 PCM -> 22 050 Hz, both qualities.  Arms, interleaved inside one process after a warm-up:
  hip   : Resampler (efts_resample_pcm16: int16 in, fp32 out, one launch);
  stock : the same fp32 table applied by torch.nn.functional.conv1d at stride M after a float conversion -- the polyphase form: output
          channel j of L holds the row of phase (j M) mod L shifted by floor(j M / L) taps (kernel length K + M - 1), then a transpose
          to sample order.
Reported per arm: ms per call (median and min over the rounds); for the HIP arm also (bytes in + bytes out) / time as a fraction of the
8.0 TB/s HBM peak the design document's rooflines use.  Not a gate: nothing asserts on the times.

    python tools/micro/resample_timing.py [--items 64] [--seconds 10] [--rounds 5] [--calls 10]
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from efficient_tts_amd.resample import Resampler, resample_table  # noqa: E402

HBM_PEAK = 8.0e12


def stock_arm(table: torch.Tensor, L: int, M: int, W: int, dev):
    K = 2 * W + 1
    j = np.arange(L)
    shift, phase = (j * M) // L, (j * M) % L
    w = torch.zeros(L, 1, K + M - 1)
    for c in range(L):
        w[c, 0, shift[c]:shift[c] + K] = table[phase[c]]
    w = w.to(dev)

    def run(pcm: torch.Tensor) -> torch.Tensor:
        x = pcm.to(torch.float32) * (1.0 / 32768.0)
        n_out = (x.shape[1] * L + M - 1) // M
        blocks = (n_out + L - 1) // L
        need = (blocks - 1) * M + K + M - 1                      # padded samples the last block reads
        x = torch.nn.functional.pad(x, (W, max(0, need - W - x.shape[1])))
        y = torch.nn.functional.conv1d(x[:, None], w, stride=M)  # [B, L, blocks]
        return y.transpose(1, 2).reshape(x.shape[0], -1)[:, :n_out]
    return run


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--items", type=int, default=64)
    ap.add_argument("--seconds", type=float, default=10.0)
    ap.add_argument("--src", type=int, default=48000)
    ap.add_argument("--dst", type=int, default=22050)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", type=str, default=os.path.join(ROOT, "profiles", "resample_timing.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise RuntimeError("no MI355X (gfx950) device visible: nothing to time")
    dev = torch.device("cuda:0")
    n = int(args.seconds * args.src)
    g = torch.Generator().manual_seed(0)
    pcm = torch.randint(-32768, 32768, (args.items, n), generator=g, dtype=torch.int32).to(torch.int16).to(dev)
    lines = []
    for quality in ("best", "fast"):
        table, L, M, W = resample_table(args.src, args.dst, quality)
        hip = Resampler(dev, args.src, args.dst, quality=quality)
        arms = {"hip": lambda: hip(pcm)[0], "stock": (lambda f: (lambda: f(pcm)))(stock_arm(table, L, M, W, dev))}
        outs = {}
        for name, fn in arms.items():
            for _ in range(args.warmup):
                outs[name] = fn()
        torch.cuda.synchronize()
        diff = float((outs["hip"] - outs["stock"]).abs().max())
        times = {name: [] for name in arms}
        for _ in range(args.rounds):
            for name, fn in arms.items():
                t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                t0.record()
                for _ in range(args.calls):
                    fn()
                t1.record()
                torch.cuda.synchronize()
                times[name].append(t0.elapsed_time(t1) / args.calls)
        n_out = outs["hip"].shape[1]
        nbytes = args.items * (2 * n + 4 * n_out)
        for name in arms:
            med = statistics.median(times[name])
            line = dict(leg=f"{name}_{quality}", ms_median=round(med, 4), ms_min=round(min(times[name]), 4), ms_rounds=[round(t, 4) for t in times[name]],
                        calls=args.calls, warmup=args.warmup, items=args.items, samples_in=n, samples_out=n_out, L=L, M=M, K=2 * W + 1)
            if name == "hip":
                line.update(bytes_in_plus_out=nbytes, bytes_per_s=nbytes / (med * 1e-3), share_of_hbm_peak=nbytes / (med * 1e-3) / HBM_PEAK)
            lines.append(line)
        hip_ms, stock_ms = statistics.median(times["hip"]), statistics.median(times["stock"])
        lines.append(dict(summary=quality, hip_ms=round(hip_ms, 4), stock_torch_ms=round(stock_ms, 4), stock_over_hip=round(stock_ms / hip_ms, 3),
                          hip_share_of_hbm_peak=nbytes / (hip_ms * 1e-3) / HBM_PEAK, hip_vs_stock_max_abs_diff=diff,
                          device=torch.cuda.get_device_name(0)))
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        for line in lines:
            f.write(json.dumps(line) + "\n")
            print(json.dumps(line), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
