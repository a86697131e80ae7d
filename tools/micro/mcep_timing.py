"""Time the waveform mel-cepstra on an MI355X: 64 x 10 s of 22 050 Hz fp32, order 24, hop 256, three arms interleaved in one process --

    fused     MelCepstrum: efts_logspec_project, one launch, no spectrogram in memory
    composed  the same result from what the library had before it: efts_stft_mag (STFTMagnitude), then torch log (twice the log of the
              magnitude) and matmul with the same table.  This arm writes and re-reads the [B, T, 513] fp32 spectrogram (113 MB here)
    stock     torch.stft, |.|^2, clamp, log and matmul on the same device

Hip events around `--calls` calls, `--rounds` rounds, median and range; writes profiles/mcep_timing.json (one JSON object per line).

    python tools/micro/mcep_timing.py [--items 64] [--seconds 10] [--rounds 5] [--calls 10]
"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

from efficient_tts_amd.mcep import MelCepstrum   # noqa: E402
from efficient_tts_amd.stft import STFTMagnitude, hann_window   # noqa: E402

HBM_PEAK = 8.0e12


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--items", type=int, default=64)
    ap.add_argument("--seconds", type=float, default=10.0)
    ap.add_argument("--rate", type=int, default=22050)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", type=str, default=os.path.join(ROOT, "profiles", "mcep_timing.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise RuntimeError("no MI355X (gfx950) device visible: nothing to time")
    dev = torch.device("cuda:0")
    B, n, N, H = args.items, int(args.seconds * args.rate), 1024, 256
    g = torch.Generator().manual_seed(0)
    t = torch.arange(n, dtype=torch.float64) / args.rate
    f0 = 110.0 + 5.0 * torch.arange(B, dtype=torch.float64)[:, None]
    voice = sum(torch.sin(2 * torch.pi * h * f0 * t[None]) / h for h in range(1, 13))
    x = (0.2 * voice + 2e-3 * torch.randn(B, n, generator=g, dtype=torch.float64)).float().to(dev)     # harmonics, white noise 40 dB down
    fused = MelCepstrum(dev, args.rate, hop_size=H)
    mag = STFTMagnitude(dev, N, H, N)
    window, table = fused._on(dev)
    table_t = table.t().contiguous()
    win = torch.from_numpy(hann_window(N)).to(dev)

    def composed():
        m, frames = mag(x)
        return (2.0 * torch.log(m)) @ table_t

    def stock():
        s = torch.stft(x, N, hop_length=H, win_length=N, window=win, center=True, pad_mode="reflect", return_complex=True)
        return torch.log((s.real ** 2 + s.imag ** 2).clamp(min=1e-7)).transpose(1, 2) @ table_t

    arms = {"fused": lambda: fused(x)[0], "composed": composed, "stock": stock}
    outs = {}
    for name, fn in arms.items():
        for _ in range(args.warmup):
            outs[name] = fn()
    torch.cuda.synchronize()
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
    T = 1 + n // H
    # what each arm has to move: the samples in (every sample lies in four frames: read once from memory, again from the caches), the
    # cepstra out, the table (L2-resident); the composed arm also writes the spectrogram and reads it back, and writes and reads its log
    bytes_fused = B * n * 4 + B * T * fused.order * 4 + table.numel() * 4
    spectrogram = B * T * (N // 2 + 1) * 4
    lines = []
    for name in arms:
        med = statistics.median(times[name])
        nbytes = bytes_fused + (4 * spectrogram if name == "composed" else 0)
        line = dict(leg=name, ms_median=round(med, 4), ms_min=round(min(times[name]), 4), ms_max=round(max(times[name]), 4),
                    ms_rounds=[round(v, 4) for v in times[name]], calls=args.calls, warmup=args.warmup, items=B, samples=n, rate=args.rate, frames=B * T,
                    order=fused.order)
        if name != "stock":
            line.update(bytes_design=nbytes, share_of_hbm_peak_design=nbytes / (med * 1e-3) / HBM_PEAK)
        lines.append(line)
    med = {name: statistics.median(v) for name, v in times.items()}
    lines.append(dict(summary="mcep", fused_ms=round(med["fused"], 4), composed_ms=round(med["composed"], 4), stock_ms=round(med["stock"], 4),
                      composed_over_fused=round(med["composed"] / med["fused"], 3), stock_over_fused=round(med["stock"] / med["fused"], 3),
                      spectrogram_bytes=spectrogram, fused_vs_composed_max_abs_diff=float((outs["fused"] - outs["composed"]).abs().max()),
                      fused_vs_stock_max_abs_diff=float((outs["fused"] - outs["stock"]).abs().max()),
                      largest_abs_coefficient=float(outs["fused"].abs().max()), frame_pairs_per_second=B * ((T + 1) // 2) / (med["fused"] * 1e-3),
                      device=torch.cuda.get_device_name(0)))
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        for line in lines:
            f.write(json.dumps(line) + "\n")
            print(json.dumps(line), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
