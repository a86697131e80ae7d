"""Time the intelligibility scores on an MI355X: 64 x 10 s of 22 050 Hz fp32, the clean signals against noisy copies, three arms interleaved
in one process --

    hip       ShortTimeIntelligibility(22050): efts_resample twice (22 050 -> 10 000 Hz), then efts_stoi
    hip_10k   efts_stoi alone (`score_10k`) on the resampler's outputs
    stock     the same definition in stock torch ops on the same device and the same 10 kHz signals: unfold, a stable argsort for the kept
              frames, torch.fft.rfft, a matmul for the bands, float64 segments -- batched, masked, no host read-back.  torch has no
              resampler of its own, so this arm is to be compared with hip_10k

Hip events around `--calls` calls, `--rounds` rounds, median and range; writes profiles/stoi_timing.json (one JSON object per line).

    python tools/micro/stoi_timing.py [--items 64] [--seconds 10] [--rounds 5] [--calls 10]
"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

from efficient_tts_amd.stoi import BANDS, FRAME, HOP, N_FFT, SEGMENT, ShortTimeIntelligibility, stoi_window   # noqa: E402

HBM_PEAK = 8.0e12
BAND_EDGES = (7, 9, 11, 14, 17, 22, 27, 34, 43, 55, 69, 87, 109, 138, 174, 219)
EPS = 2.0 ** -52


def stock_arm(dev, n):
    """(x, y, lengths) -> (stoi, estoi, kept), the definition of include/efts_abi.h in torch ops"""
    w = torch.from_numpy(stoi_window()).to(dev)
    F = (n - FRAME) // HOP + 1
    band = torch.zeros(N_FFT // 2 + 1, BANDS, device=dev)
    for j in range(BANDS):
        band[BAND_EDGES[j]:BAND_EDGES[j + 1], j] = 1.0
    ar = torch.arange(F, device=dev)[None]
    clip = 1.0 + 10.0 ** (15.0 / 20.0)

    def unit(a, dim):
        a = a - a.mean(dim=dim, keepdim=True)
        return a / (a.norm(dim=dim, keepdim=True) + EPS)

    def spectra(frames):
        s = torch.zeros(frames.shape[0], F + 1, HOP, device=dev)
        s[:, :F] += frames[:, :, :HOP]
        s[:, 1:] += frames[:, :, HOP:]
        p = torch.fft.rfft(s.reshape(frames.shape[0], -1).unfold(1, FRAME, HOP) * w, N_FFT).abs() ** 2
        return (p @ band).sqrt().unfold(1, SEGMENT, 1).double()         # [B, F - 29, 15, 30]

    def run(x, y, lengths):
        Fb = torch.where(lengths >= FRAME, (lengths - FRAME) // HOP + 1, torch.zeros_like(lengths))
        xf, yf = x.unfold(1, FRAME, HOP) * w, y.unfold(1, FRAME, HOP) * w
        e = (xf * xf).sum(-1).masked_fill(ar >= Fb[:, None], 0.0)
        keep = (e.double() * 1e4 > e.max(1, keepdim=True).values.double()) & (ar < Fb[:, None])
        K = keep.sum(1)
        order = torch.argsort((~keep).to(torch.int8), dim=1, stable=True)[:, :, None].expand(-1, -1, FRAME)
        live = (ar < K[:, None])[:, :, None]
        X, Y = spectra(torch.gather(xf, 1, order) * live), spectra(torch.gather(yf, 1, order) * live)
        M = (K - SEGMENT).clamp(min=0)
        seg = torch.arange(X.shape[1], device=dev)[None] < M[:, None]
        c = X.norm(dim=3, keepdim=True) / (Y.norm(dim=3, keepdim=True) + EPS)
        d = (unit(X, 3) * unit(torch.minimum(c * Y, X * clip), 3)).sum((2, 3))
        q = (unit(unit(X, 3), 2) * unit(unit(Y, 3), 2)).sum((2, 3))
        nan = torch.full_like(M, float("nan"), dtype=torch.float64)
        stoi = torch.where(M > 0, (d * seg).sum(1) / (BANDS * M.clamp(min=1)), nan)
        estoi = torch.where(M > 0, (q * seg).sum(1) / (SEGMENT * M.clamp(min=1)), nan)
        return stoi, estoi, K
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
    ap.add_argument("--snr_db", type=float, default=5.0)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", type=str, default=os.path.join(ROOT, "profiles", "stoi_timing.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise RuntimeError("no MI355X (gfx950) device visible: nothing to time")
    dev = torch.device("cuda:0")
    B, n = args.items, int(args.seconds * args.rate)
    g = torch.Generator().manual_seed(0)
    t = torch.arange(n, dtype=torch.float64) / args.rate
    f0 = 110.0 + 5.0 * torch.arange(B, dtype=torch.float64)[:, None]
    voice = sum(torch.sin(2 * torch.pi * h * f0 * t[None]) / h for h in range(1, 13))
    env = torch.sin(2 * torch.pi * 1.3 * t)[None].clamp(min=0.0) ** 2               # syllables: about half of the frames are silent
    x = (0.2 * env * voice + 1e-4 * torch.randn(B, n, generator=g, dtype=torch.float64)).float()
    y = (x + x.pow(2).mean().sqrt() * 10.0 ** (-args.snr_db / 20.0) * torch.randn(B, n, generator=g)).float()
    x, y = x.to(dev), y.to(dev)
    hip = ShortTimeIntelligibility(dev, args.rate)
    lengths = torch.full((B,), n, device=dev)
    x10, n10 = hip.resampler(x, lengths)
    y10, _ = hip.resampler(y, lengths)
    m = int(x10.shape[1])
    stock = stock_arm(dev, m)
    arms = {"hip": lambda: hip(x, y), "hip_10k": lambda: hip.score_10k(x10, y10, n10), "stock": lambda: stock(x10, y10, n10)}
    outs = {}
    for name, fn in arms.items():
        for _ in range(args.warmup):
            outs[name] = fn()
    torch.cuda.synchronize()
    same = all(torch.equal(outs["hip"][k].view(torch.int64), outs["hip_10k"][k].view(torch.int64)) for k in ("stoi", "estoi", "kept"))
    diff = max(float((outs["hip_10k"]["stoi"] - outs["stock"][0]).abs().max()), float((outs["hip_10k"]["estoi"] - outs["stock"][1]).abs().max()))
    kept_equal = bool(torch.equal(outs["hip_10k"]["kept"], outs["stock"][2]))
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
    F = (m - FRAME) // HOP + 1
    kept = int(outs["hip_10k"]["kept"].sum())
    # what the algorithm has to move: the resampler reads both signals and writes both; efts_stoi reads x for the energies, the kept frames
    # of x and y once more (every sample of a kept frame lies in two frames: read twice at most, from the caches), and writes and reads
    # energies, the frame list, the band rows (64 B per spectral frame and signal) and 16 B per segment
    bytes_resample = 2 * B * (n + m) * 4
    bytes_core = B * m * 4 + 2 * kept * FRAME * 4 * 2 + 2 * (B * F * 8 + 2 * kept * 64 + max(kept - B * SEGMENT, 0) * 16)
    lines = []
    for name, fn in arms.items():
        med = statistics.median(times[name])
        line = dict(leg=name, ms_median=round(med, 4), ms_min=round(min(times[name]), 4), ms_max=round(max(times[name]), 4),
                    ms_rounds=[round(v, 4) for v in times[name]], calls=args.calls, warmup=args.warmup, items=B, samples=n if name == "hip" else m,
                    rate=args.rate if name == "hip" else 10000, snr_db=args.snr_db, kernel_us=kernels_of(fn))
        if name != "stock":
            nbytes = bytes_core + (bytes_resample if name == "hip" else 0)
            line.update(bytes_design=nbytes, share_of_hbm_peak_design=nbytes / (med * 1e-3) / HBM_PEAK, frames=B * F, kept_frames=kept)
        lines.append(line)
    med = {name: statistics.median(v) for name, v in times.items()}
    lines.append(dict(summary="stoi", hip_ms=round(med["hip"], 4), hip_10k_ms=round(med["hip_10k"], 4), stock_ms=round(med["stock"], 4),
                      stock_over_hip_10k=round(med["stock"] / med["hip_10k"], 3), hip_equals_hip_10k_bits=same, kept_frames_equal_stock=kept_equal,
                      hip_10k_vs_stock_max_abs_diff=diff, mean_stoi=float(outs["hip"]["stoi"].nanmean()), mean_estoi=float(outs["hip"]["estoi"].nanmean()),
                      device=torch.cuda.get_device_name(0)))
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        for line in lines:
            f.write(json.dumps(line) + "\n")
            print(json.dumps(line), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
