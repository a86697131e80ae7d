"""Timing of the Griffin-Lim vocoder (efficient_tts_amd/griffinlim.py): one 800-frame utterance and a batch of 8 at 32 iterations,
and in the same process the same loop written with stock torch ops on the same GPU: torch.stft, and torch.fft.irfft + fold for the inverse
(torch.istft refuses this framing: the periodic Hann window is 0 at the first sample, which only frame 0 covers).  The baseline lives in this tool only.
Each leg: warm-up calls (the vocoder's third call replays its hipGraph), then HIP events around `--calls` calls (>= 50); the legs take
turns for `--rounds` rounds and the median per leg is reported.  One JSON line per leg and a summary line per batch size.
Usage: python tools/gpu_time_griffinlim.py [--rounds 5] [--calls 50] [--warmup 5] [--iters 32] [--out profiles/griffinlim_timing.json]
       python tools/gpu_time_griffinlim.py --one-call      # a single B = 1 call after warm-up without graphs (for a kernel trace)"""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from efficient_tts_amd.frontend import slaney_mel_filterbank  # noqa: E402
from efficient_tts_amd.griffinlim import GriffinLimVocoder  # noqa: E402

N_FFT, HOP, PAD = 1024, 256, 384


def stock_griffinlim(pinv, window, n_iter, momentum):
    """the same iteration with stock torch ops: torch.matmul for the mel inversion, irfft + fold / torch.stft (center=False on the
    padded signal: the same framing) for steps 3 and 4"""
    w2 = (window * window)[None, :, None]

    def ola(frames, n):                                  # [B, 1024, T] -> [B, n]
        return torch.nn.functional.fold(frames, (1, n), (1, N_FFT), stride=(1, HOP))[:, 0, 0]

    def istft(X, n, inv_wss):
        return ola(torch.fft.irfft(X, n=N_FFT, dim=1) * window[None, :, None], n) * inv_wss

    def run(mel):                                        # [B, 80, T]
        M = torch.matmul(pinv, torch.exp(mel)).clamp_min(1e-5)                    # [B, 513, T]
        X = M.to(torch.complex64)
        prev = torch.zeros_like(X)
        n = HOP * mel.shape[2] + N_FFT - HOP
        inv_wss = 1.0 / ola(w2.expand(1, N_FFT, mel.shape[2]), n).clamp_min(1e-8)      # once per call, outside the loop
        for _ in range(n_iter):
            Y = torch.stft(istft(X, n, inv_wss), N_FFT, HOP, N_FFT, window, center=False, return_complex=True)
            C = Y + momentum * (Y - prev)
            X = C * (M / C.abs().clamp_min(1e-8))
            prev = Y
        return istft(X, n, inv_wss)[:, PAD:n - PAD]
    return run


def timed(fn, calls, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(calls):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / calls


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--iters", type=int, default=32)
    ap.add_argument("--frames", type=int, default=800)
    ap.add_argument("--one-call", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(0)
    mels = {B: (torch.randn(B, 80, args.frames, generator=g) * 1.5 - 5.0).to(dev) for B in (1, 8)}
    if args.one_call:
        voc = GriffinLimVocoder(dev, n_iter=args.iters, graphs=False)
        with torch.no_grad():
            voc(mels[1])
            torch.cuda.synchronize()
            voc(mels[1])
            torch.cuda.synchronize()
        print(json.dumps(dict(one_call=True, calls=2, iters=args.iters, frames=args.frames, loop_launches_per_call=2 * args.iters)))
        return
    fb = slaney_mel_filterbank(22050, N_FFT, 80, 0.0, 8000.0).astype(np.float64)
    pinv = torch.from_numpy(np.linalg.pinv(fb).astype(np.float32)).to(dev)
    window = torch.hann_window(N_FFT, dtype=torch.float32).to(dev)
    voc = GriffinLimVocoder(dev, n_iter=args.iters)
    stock = stock_griffinlim(pinv, window, args.iters, 0.99)
    legs = {}
    for B, mel in mels.items():
        legs[f"hip_B{B}"] = (lambda mel=mel: voc(mel))
        legs[f"stock_torch_B{B}"] = (lambda mel=mel: stock(mel))
    res = {k: [] for k in legs}
    with torch.no_grad():
        one = GriffinLimVocoder(dev, n_iter=1, precision="fp32")(mels[1])[0, 0]
        ref = stock_griffinlim(pinv, window, 1, 0.99)(mels[1])[0]
        agree = float((one - ref).abs().max() / ref.abs().max())     # the two loops compute the same thing (one iteration: float32 rounding grows along the loop)
        for _ in range(args.rounds):
            for name, fn in legs.items():
                res[name].append(timed(fn, args.calls, args.warmup))
    lines = [dict(leg=name, ms_median=round(statistics.median(v), 4), ms_min=round(min(v), 4), ms_rounds=[round(x, 4) for x in v], calls=args.calls,
                  warmup=args.warmup, iters=args.iters, frames=args.frames) for name, v in res.items()]
    for B in mels:
        hip, st = statistics.median(res[f"hip_B{B}"]), statistics.median(res[f"stock_torch_B{B}"])
        lines.append(dict(summary=f"B{B}", hip_ms=round(hip, 4), stock_torch_ms=round(st, 4), stock_over_hip=round(st / hip, 2),
                          hip_us_per_iteration=round(hip * 1e3 / max(args.iters, 1), 2), audio_seconds=round(B * args.frames * HOP / 22050, 2),
                          hip_vs_stock_rel_diff_after_1_iteration=round(agree, 6), device=torch.cuda.get_device_name(0)))
    text_out = "\n".join(json.dumps(x) for x in lines)
    print(text_out, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text_out + "\n")


if __name__ == "__main__":
    main()
