"""Time the spectral gate on an MI355X: 64 x 10 s of 22 050 Hz fp32 -- a 220 Hz tone of peak 0.5 over white noise 50 dB below it, with
0.5 s of the noise alone at both ends -- five arms interleaved in one process --

    profile   efts_noise_profile alone (NoiseProfile): four launches
    gate      efts_spectral_gate alone (SpectralGate with the measured profiles given): one launch
    whole     the whole SpectralGate call: profile, bypass flags (torch), gate
    denoise   efts_denoise on the same batch (BiasDenoiser with item 0's profile as the bias): the kernel body that the gate shares
    torch     the same result in stock torch ops on the same device: torch.stft, energies, masked mean, gain, torch.istft

Hip events around `--calls` calls, `--rounds` rounds, median and range; writes profiles/gate_timing.json (one JSON object per line).

    python tools/micro/gate_timing.py [--items 64] [--seconds 10] [--rounds 5] [--calls 10]
"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from denoise_timing import kernels_of             # noqa: E402
from efficient_tts_amd.denoise import BiasDenoiser, NoiseProfile, SpectralGate   # noqa: E402
from efficient_tts_amd.stft import hann_window    # noqa: E402

HBM_PEAK = 8.0e12
N, H, BINS = 1024, 256, 513


def torch_arm(dev, n, strength, floor, ratio, min_frames):
    window = torch.from_numpy(hann_window(N)).to(dev)

    def run(audio):
        X = torch.stft(audio, N, H, N, window=window, center=True, pad_mode="reflect", return_complex=True)        # [B, 513, T]
        m = X.abs()
        frames = torch.nn.functional.pad(audio[:, None], (N // 2, N // 2), mode="reflect")[:, 0].unfold(1, N, H)     # [B, T, 1024]
        e = ((frames * window).double() ** 2).sum(dim=2)                                                             # [B, T]
        noise = e * ratio < e.max(dim=1, keepdim=True).values
        K = noise.sum(dim=1)
        profile = (m.double() * noise[:, None, :]).sum(dim=2) / K.clamp(min=1)[:, None]
        d = m - strength * profile.float()[:, :, None]
        g = torch.where(d > 0, d / m.clamp(min=1e-30), torch.zeros_like(m)).clamp(min=floor)
        out = torch.istft(X * g, N, H, N, window=window, center=True, length=n)
        return torch.where((K < min_frames)[:, None], audio, out)
    return run


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--items", type=int, default=64)
    ap.add_argument("--seconds", type=float, default=10.0)
    ap.add_argument("--rate", type=int, default=22050)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", type=str, default=os.path.join(ROOT, "profiles", "gate_timing.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise RuntimeError("no MI355X (gfx950) device visible: nothing to time")
    dev = torch.device("cuda:0")
    B, n = args.items, int(args.seconds * args.rate)
    g = torch.Generator().manual_seed(0)
    t = torch.arange(n, dtype=torch.float64) / args.rate
    edge = int(0.5 * args.rate)
    tone = 0.5 * torch.sin(2 * torch.pi * 220.0 * t)
    tone[:edge] = 0.0
    tone[n - edge:] = 0.0
    audio = (tone[None] + 0.5 * 10.0 ** (-50.0 / 20.0) * torch.randn(B, n, generator=g, dtype=torch.float64)).float().to(dev)
    measure, gate = NoiseProfile(dev), SpectralGate(dev)
    stats = measure(audio)
    profiles = stats["profile"].clone()
    denoiser = BiasDenoiser(dev, profiles[0], strength=1.0)
    stock = torch_arm(dev, n, gate.strength, gate.floor, measure.ratio, measure.min_frames)
    arms = {"profile": lambda: measure(audio)["profile"], "gate": lambda: gate(audio, profile=profiles), "whole": lambda: gate(audio),
            "denoise": lambda: denoiser(audio), "torch": lambda: stock(audio)}
    outs = {}
    for name, fn in arms.items():
        for _ in range(args.warmup):
            outs[name] = fn()
    torch.cuda.synchronize()
    noise_frames = stats["noise_frames"].tolist()
    diff_torch = float((outs["whole"] - outs["torch"]).abs().max())
    same = bool(torch.equal(outs["whole"], outs["gate"]))
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
    lines = []
    for name, fn in arms.items():
        med = statistics.median(times[name])
        line = dict(leg=name, ms_median=round(med, 4), ms_min=round(min(times[name]), 4), ms_max=round(max(times[name]), 4),
                    ms_rounds=[round(v, 4) for v in times[name]], calls=args.calls, warmup=args.warmup, items=B, samples=n, rate=args.rate,
                    kernel_us=kernels_of(fn))
        if name in ("gate", "denoise"):
            line.update(bytes_design=B * n * 8, share_of_hbm_peak_design=B * n * 8 / (med * 1e-3) / HBM_PEAK)
        if name == "profile":
            # the samples once from memory (the energies' four-fold read of every sample is served by the caches), the energies and flags out and
            # in, one partial row per run with a noise frame out and in
            runs = sum(min(-(-T // 16), -(-k // 16) + 2) for k in noise_frames)
            design = B * n * 4 + B * T * (8 + 8 + 4 + 4) + runs * BINS * 8 * 2
            line.update(bytes_design=design, share_of_hbm_peak_design=design / (med * 1e-3) / HBM_PEAK, frames=B * T, noise_frames=sum(noise_frames),
                        runs_with_a_noise_frame_upper_bound=runs)
        lines.append(line)
    med = {name: statistics.median(v) for name, v in times.items()}
    lines.append(dict(summary="gate", **{f"{k}_ms": round(v, 4) for k, v in med.items()}, gate_over_denoise=round(med["gate"] / med["denoise"], 3),
                      torch_over_whole=round(med["torch"] / med["whole"], 3), whole_vs_torch_max_abs_diff=diff_torch,
                      whole_equals_gate_with_given_profiles=same, noise_frames_min=min(noise_frames), noise_frames_max=max(noise_frames),
                      device=torch.cuda.get_device_name(0)))
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        for line in lines:
            f.write(json.dumps(line) + "\n")
            print(json.dumps(line), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
