"""Time the bias denoiser on an MI355X: 64 x 10 s of 22 050 Hz fp32 at strength 0.01, three arms interleaved in one process --

    hip       efts_denoise (BiasDenoiser): one launch, no spectrum in memory
    composed  what the library offered before: reflect padding (torch) -> efts_gl_analysis (signal mode) -> gain (torch) -> efts_gl_synthesis ->
              efts_gl_overlap_add, on the first 256 * (n // 256) samples (that route frames only multiples of the hop)
    torch     torch.stft -> gain -> torch.istft on the same device

Hip events around `--calls` calls, `--rounds` rounds, median and range; writes profiles/denoise_timing.json (one JSON object per line).

    python tools/micro/denoise_timing.py [--items 64] [--seconds 10] [--rounds 5] [--calls 10]
"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

from efficient_tts_amd import lib as L_          # noqa: E402
from efficient_tts_amd import ops as O           # noqa: E402
from efficient_tts_amd.denoise import BiasDenoiser   # noqa: E402
from efficient_tts_amd.stft import hann_window   # noqa: E402

HBM_PEAK = 8.0e12
N, H, BINS = 1024, 256, 513


def gain(spec, sb):
    m = spec.abs()
    d = m - sb
    return spec * torch.where(d > 0, d / m.clamp(min=1e-30), torch.zeros_like(m))


def composed_arm(dev, bias, strength, B, n):
    lib = L_.load()
    T = n // H + 1
    window = torch.from_numpy(hann_window(N)).to(dev)
    frames = torch.full((B,), T, dtype=torch.int32, device=dev)
    spec = torch.empty(B, T, BINS, dtype=torch.complex64, device=dev)
    wf = torch.empty(B, T, N, dtype=torch.float32, device=dev)
    out = torch.empty(B, n + H, dtype=torch.float32, device=dev)
    sb = (strength * bias).to(dev)

    def run(audio):
        padded = torch.nn.functional.pad(audio[:, None], (N // 2, N // 2), mode="reflect")[:, 0].contiguous()
        with O.stream_scope():
            L_.check(lib.efts_gl_analysis(None, padded.data_ptr(), padded.shape[1], frames.data_ptr(), window.data_ptr(), None, None, spec.data_ptr(), 0.0,
                                          B, T, N, H, O._stream()), "efts_gl_analysis")
        s2 = gain(spec, sb).contiguous()
        with O.stream_scope():
            L_.check(lib.efts_gl_synthesis(s2.data_ptr(), frames.data_ptr(), window.data_ptr(), wf.data_ptr(), B, T, N, H, O._stream()), "efts_gl_synthesis")
            L_.check(lib.efts_gl_overlap_add(wf.data_ptr(), frames.data_ptr(), window.data_ptr(), out.data_ptr(), n + H, 384, n + H, B, T, N, H, O._stream()),
                     "efts_gl_overlap_add")
        return out[:, 128:128 + n]
    return run


def torch_arm(dev, bias, strength, n):
    window = torch.from_numpy(hann_window(N)).to(dev)
    sb = (strength * bias).to(dev)[:, None]

    def run(audio):
        X = torch.stft(audio, N, H, N, window=window, center=True, pad_mode="reflect", return_complex=True)
        return torch.istft(gain(X, sb), N, H, N, window=window, center=True, length=n)
    return run


def kernels_of(fn):
    """{kernel name: device microseconds} of one call, from torch's profiler in a pass of its own"""
    try:
        from torch.profiler import ProfilerActivity, profile
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        rows = {}
        for ev in prof.events():
            if str(getattr(ev, "device_type", "")).endswith("CUDA") and "memcpy" not in ev.name.lower() and "memset" not in ev.name.lower():
                t = float(getattr(ev, "device_time_total", 0.0) or getattr(ev, "cuda_time_total", 0.0) or 0.0)
                rows[ev.name[:80]] = round(rows.get(ev.name[:80], 0.0) + t, 2)
        return rows or None
    except Exception as exc:                                   # the profiler is a convenience here, the times do not depend on it
        print(f"profiler not available: {exc!r}", flush=True)
        return None


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--items", type=int, default=64)
    ap.add_argument("--seconds", type=float, default=10.0)
    ap.add_argument("--rate", type=int, default=22050)
    ap.add_argument("--strength", type=float, default=0.01)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", type=str, default=os.path.join(ROOT, "profiles", "denoise_timing.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise RuntimeError("no MI355X (gfx950) device visible: nothing to time")
    dev = torch.device("cuda:0")
    B, n = args.items, int(args.seconds * args.rate)
    n256 = n // H * H
    g = torch.Generator().manual_seed(0)
    t = torch.arange(n, dtype=torch.float64) / args.rate
    audio = (0.3 * torch.sin(2 * torch.pi * 220.0 * t)[None] + 0.05 * torch.randn(B, n, generator=g, dtype=torch.float64)).float().to(dev)
    audio256 = audio[:, :n256].contiguous()
    bias = 2.0 * torch.randn(BINS, generator=g).abs()
    hip = BiasDenoiser(dev, bias, strength=args.strength)
    composed, stock = composed_arm(dev, bias, args.strength, B, n256), torch_arm(dev, bias, args.strength, n)
    arms = {"hip": lambda: hip(audio), "composed": lambda: composed(audio256), "torch": lambda: stock(audio)}
    outs = {}
    for name, fn in arms.items():
        for _ in range(args.warmup):
            outs[name] = fn()
    torch.cuda.synchronize()
    diff_torch = float((outs["hip"] - outs["torch"]).abs().max())
    diff_composed = float((hip(audio256) - outs["composed"]).abs().max())
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
    lines = []
    for name, fn in arms.items():
        med = statistics.median(times[name])
        line = dict(leg=name, ms_median=round(med, 4), ms_min=round(min(times[name]), 4), ms_max=round(max(times[name]), 4),
                    ms_rounds=[round(v, 4) for v in times[name]], calls=args.calls, warmup=args.warmup, items=B, samples=n256 if name == "composed" else n,
                    rate=args.rate, strength=args.strength, kernel_us=kernels_of(fn))
        if name == "hip":
            frames_needed = B * (1 + n // H)
            runs = B * -(-n // (16 * H))
            line.update(bytes_design=B * n * 8, share_of_hbm_peak_design=B * n * 8 / (med * 1e-3) / HBM_PEAK, frames=frames_needed,
                        frames_transformed_upper_bound=runs * 20, transforms_per_pair=2)
        lines.append(line)
    med = {name: statistics.median(v) for name, v in times.items()}
    lines.append(dict(summary="denoise", hip_ms=round(med["hip"], 4), composed_ms=round(med["composed"], 4), torch_ms=round(med["torch"], 4),
                      composed_over_hip=round(med["composed"] / med["hip"], 3), torch_over_hip=round(med["torch"] / med["hip"], 3),
                      hip_vs_torch_max_abs_diff=diff_torch, hip_vs_composed_max_abs_diff=diff_composed, device=torch.cuda.get_device_name(0)))
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        for line in lines:
            f.write(json.dumps(line) + "\n")
            print(json.dumps(line), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
