"""Time the on-device multi-resolution STFT distance against torch.stft plus the same sums on the same GPU; writes profiles/mrstft_timing.json.

Workload: 64 x 10 s of 22 050 Hz, the candidate fp32 against the recording as int16 PCM, the three default resolutions
(1024, 120, 600), (2048, 240, 1200), (512, 50, 240).  Arms, interleaved inside one process after a warm-up:
  hip   : MultiResolutionSTFTDistance (efts_stft_dist: per resolution one fused launch and one small float64 reduction; no spectrogram in memory);
  stock : per resolution torch.stft of both signals (the int16 one converted to fp32 first), sqrt(clamp(re^2 + im^2, 1e-7)), and the three
          sums per item in float64.
Reported per arm: ms per call (median and min over the rounds, events around `--calls` calls) and the bytes the arm READS over the call time as
a share of the 8.0 TB/s HBM peak the design document's rooflines use.  hip reads both signals once per resolution plus the frame sums it
wrote; stock reads the signals, and then every spectrogram it wrote: the complex spectrum once, the magnitudes for each of the three sums
(what a perfectly fused elementwise chain would still have to read; the real chain reads more).  The two arms' sums are compared.
Not a gate: nothing asserts on the times.

    python tools/micro/mrstft_timing.py [--items 64] [--seconds 10] [--rounds 5] [--calls 10]
"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from efficient_tts_amd.stft import DEFAULT_RESOLUTIONS, MultiResolutionSTFTDistance, hann_window  # noqa: E402

HBM_PEAK = 8.0e12


def stock_arm(dev, max_wav_value: float = 32768.0):
    wins = {W: torch.from_numpy(hann_window(W)).to(dev) for _, _, W in DEFAULT_RESOLUTIONS}

    def run(x: torch.Tensor, y16: torch.Tensor):
        y = y16.to(torch.float32) * (1.0 / max_wav_value)
        sums = []
        for N, H, W in DEFAULT_RESOLUTIONS:
            mags = []
            for s in (x, y):
                spec = torch.stft(s, N, H, W, wins[W], return_complex=True)
                mags.append(torch.sqrt(torch.clamp(spec.real ** 2 + spec.imag ** 2, min=1e-7)))
            mx, my = mags
            sums.append(torch.stack([((my - mx) ** 2).sum(dim=(1, 2), dtype=torch.float64), (my ** 2).sum(dim=(1, 2), dtype=torch.float64),
                                     (torch.log(my) - torch.log(mx)).abs().sum(dim=(1, 2), dtype=torch.float64)], dim=1))
        return torch.stack(sums, dim=1)                              # [B, R, 3]
    return run


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--items", type=int, default=64)
    ap.add_argument("--seconds", type=float, default=10.0)
    ap.add_argument("--rate", type=int, default=22050)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", type=str, default=os.path.join(ROOT, "profiles", "mrstft_timing.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise RuntimeError("no MI355X (gfx950) device visible: nothing to time")
    dev = torch.device("cuda:0")
    B, n = args.items, int(args.seconds * args.rate)
    g = torch.Generator().manual_seed(0)
    t = torch.arange(n, dtype=torch.float64)
    clean = 0.3 * torch.sin(2 * torch.pi * 220.0 / args.rate * t) + 0.2 * torch.sin(2 * torch.pi * 3100.0 / args.rate * t)
    y16 = torch.round((clean[None, :] + 0.02 * torch.randn(B, n, generator=g, dtype=torch.float64)) * 32768.0).clamp(-32768, 32767).to(torch.int16).to(dev)
    x = (0.9 * clean[None, :] + 0.03 * torch.randn(B, n, generator=g, dtype=torch.float64)).to(torch.float32).to(dev)
    hip = MultiResolutionSTFTDistance(dev)
    stock = stock_arm(dev)
    arms = {"hip": lambda: hip(x, y16)["sums"], "stock": lambda: stock(x, y16)}
    outs = {}
    for name, fn in arms.items():
        for _ in range(args.warmup):
            outs[name] = fn()
    torch.cuda.synchronize()
    rel = float(((outs["hip"] - outs["stock"]).abs() / outs["stock"]).max())
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
    cells = [(1 + n // H) * (N // 2 + 1) for N, H, _ in DEFAULT_RESOLUTIONS]
    signal_bytes = B * n * (4 + 2)
    bytes_read = {
        "hip": sum(signal_bytes + B * (1 + n // H) * 12 for _, H, _ in DEFAULT_RESOLUTIONS),
        # the int16 conversion, then per resolution both signals, both complex spectra (8 bytes a cell) and the magnitudes for the three sums (2 + 1 + 2 reads of 4 bytes)
        "stock": B * n * 2 + sum(B * n * 8 + B * c * (2 * 8 + 5 * 4) for c in cells),
    }
    lines = []
    for name in arms:
        med = statistics.median(times[name])
        lines.append(dict(leg=name, ms_median=round(med, 4), ms_min=round(min(times[name]), 4), ms_rounds=[round(v, 4) for v in times[name]], calls=args.calls,
                          warmup=args.warmup, items=B, samples=n, resolutions=[list(r) for r in DEFAULT_RESOLUTIONS], bytes_read=bytes_read[name],
                          share_of_hbm_peak_read=bytes_read[name] / (med * 1e-3) / HBM_PEAK))
    hip_ms, stock_ms = statistics.median(times["hip"]), statistics.median(times["stock"])
    flops = sum(2 * B * ((1 + n // H + 1) // 2) * 5 * N * (N.bit_length() - 1) for N, H, _ in DEFAULT_RESOLUTIONS)     # two signals, one complex transform per frame pair
    lines.append(dict(summary="mrstft", hip_ms=round(hip_ms, 4), stock_torch_ms=round(stock_ms, 4), stock_over_hip=round(stock_ms / hip_ms, 3),
                      hip_vs_stock_max_rel_diff_of_sums=rel, hip_fft_gflop=round(flops / 1e9, 2), hip_fft_tflops=round(flops / (hip_ms * 1e-3) / 1e12, 2),
                      bound="the kernel reads its samples from cache many times over (N / H times each) and writes 12 bytes a frame: its HBM traffic is a "
                            "few per cent of the peak, and the time goes to the fp32 FFT arithmetic and the LDS transposes of the transform, not to bytes",
                      device=torch.cuda.get_device_name(0)))
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        for line in lines:
            f.write(json.dumps(line) + "\n")
            print(json.dumps(line), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
