"""Time on-device loudness normalisation against the same algorithm in stock PyTorch ops on the same GPU; writes profiles/loudness_timing.json.

Workload: 64 x 10 s of 22 050 Hz int16 PCM (uniform noise, every second half second 30 dB down), target -23 LUFS, ceiling 0.99.  Arms,
interleaved inside one process after a warm-up:
  hip   : LoudnessNormalizer (efts_loudness_pcm16: int16 in, fp32 out, three launches);
  stock : the same definition from stock ops in float64 -- the K-weighting filter by `torchaudio.functional.lfilter` when torchaudio can be
          imported, else the same segmented recurrence (512 samples behind 0.2 s of warm-up, every segment of every item at once) advanced
          one sample per step with elementwise ops; then sub-block sums, the 400 ms blocks, both gates, the gain and the scaled copy.
Reported per arm: ms per call (median and min over the rounds) and the device kernels of one call as the profiler lists them.  For the HIP
arm also the bytes that the design moves from HBM -- the input read twice (filter, copy), the output written once; what the segments' warm-up
re-reads comes from the caches -- over the time, as a share of the 8.0 TB/s HBM peak that the design document's rooflines use, and the fp64
operations of the filter launch, warm-up included, over its time.  The loudness of the two arms is compared.  Not a gate: nothing asserts on
the times.

    python tools/micro/loudness_timing.py [--items 64] [--seconds 10] [--rounds 5] [--calls 10] [--stock_calls 1]
"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from efficient_tts_amd.loudness import LoudnessNormalizer, k_weighting  # noqa: E402

HBM_PEAK = 8.0e12
SEG = 512
GAMMA_A = 10.0 ** ((-70.0 + 0.691) / 10.0)


def _filter_lfilter(x, coef):
    import torchaudio.functional as F
    c = torch.as_tensor(coef, dtype=torch.float64, device=x.device)
    one = torch.ones(1, dtype=torch.float64, device=x.device)
    v = F.lfilter(x, torch.cat([one, c[3:5]]), c[0:3], clamp=False)
    return F.lfilter(v, torch.cat([one, c[8:10]]), c[5:8], clamp=False)


def _filter_steps(x, coef, h):
    """every segment of every item from zero state behind 2 h samples of warm-up, one sample per step"""
    B, n = x.shape
    nseg, W = -(-n // SEG), 2 * h
    xp = torch.nn.functional.pad(x, (W, nseg * SEG - n))
    seg = xp.unfold(1, W + SEG, SEG).reshape(B * nseg, W + SEG)                       # row s: samples s SEG - W .. s SEG + SEG - 1
    sb0, sb1, sb2, sa1, sa2, hb0, hb1, hb2, ha1, ha2 = [float(c) for c in coef]
    s1 = torch.zeros(B * nseg, dtype=torch.float64, device=x.device)
    s2, t1, t2 = s1.clone(), s1.clone(), s1.clone()
    y = torch.empty(B * nseg, SEG, dtype=torch.float64, device=x.device)
    for i in range(W + SEG):
        xi = seg[:, i]
        v = sb0 * xi + s1
        s1 = sb1 * xi - sa1 * v + s2
        s2 = sb2 * xi - sa2 * v
        o = hb0 * v + t1
        t1 = hb1 * v - ha1 * o + t2
        t2 = hb2 * v - ha2 * o
        if i >= W:
            y[:, i - W] = o
    return y.reshape(B, nseg * SEG)[:, :n]


def stock_arm(rate: int, target: float, ceiling: float, scale: float, use_lfilter: bool):
    coef, h = k_weighting(rate), rate // 10

    def run(pcm: torch.Tensor, lengths: torch.Tensor):
        B, n = pcm.shape
        dev = pcm.device
        pos = torch.arange(n, device=dev)
        inside = pos[None, :] < lengths[:, None]
        xf = pcm.to(torch.float32)
        x = torch.where(inside, xf.double() * scale, torch.zeros((), dtype=torch.float64, device=dev))
        y = _filter_lfilter(x, coef) if use_lfilter else _filter_steps(x, coef, h)
        nsub = n // h
        sub = (y[:, :nsub * h] ** 2).reshape(B, nsub, h).sum(dim=2)
        z = sub.unfold(1, 4, 1).sum(dim=2) / (4.0 * h)
        j = torch.arange(z.shape[1], device=dev)
        real = j[None, :] < (torch.div(lengths, h, rounding_mode="floor") - 3)[:, None]
        A = real & (z > GAMMA_A)
        nA = A.sum(dim=1)
        gamma_r = 0.1 * (z * A).sum(dim=1) / nA.clamp(min=1)
        G = A & (z > gamma_r[:, None])
        lufs = -0.691 + 10.0 * torch.log10((z * G).sum(dim=1) / G.sum(dim=1).clamp(min=1))
        lufs = torch.where(nA > 0, lufs, torch.full_like(lufs, float("-inf")))
        g = torch.where(nA > 0, 10.0 ** ((target - lufs) / 20.0), torch.ones_like(lufs))
        p = x.abs().max(dim=1).values
        g = torch.where((nA > 0) & (g * p > ceiling), ceiling / p.clamp(min=1e-300), g)
        gain = (g * scale).to(torch.float32)
        out = torch.where(inside, xf * gain[:, None], torch.zeros((), device=dev))
        return out, lufs, gain
    return run


def kernels_of(fn):
    """(count, {kernel name: device us}) of one call as torch.profiler lists it, or (None, None) when it is not available"""
    try:
        from torch.profiler import ProfilerActivity, profile
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        rows = {}
        count = 0
        for ev in prof.events():
            if str(getattr(ev, "device_type", "")).endswith("CUDA") and "memcpy" not in ev.name.lower() and "memset" not in ev.name.lower():
                t = float(getattr(ev, "device_time_total", 0.0) or getattr(ev, "cuda_time_total", 0.0) or 0.0)
                count += 1
                rows[ev.name[:96]] = round(rows.get(ev.name[:96], 0.0) + t, 2)
        return (count, rows) if count else (None, None)
    except Exception as exc:                                   # the profiler is a convenience here, the times above do not depend on it
        print(f"profiler not available: {exc!r}", flush=True)
        return None, None


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--items", type=int, default=64)
    ap.add_argument("--seconds", type=float, default=10.0)
    ap.add_argument("--rate", type=int, default=22050)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--stock_calls", type=int, default=1, help="calls per round of the stock arm (one call of the stepped recurrence is thousands of launches)")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", type=str, default=os.path.join(ROOT, "profiles", "loudness_timing.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise RuntimeError("no MI355X (gfx950) device visible: nothing to time")
    dev = torch.device("cuda:0")
    n = int(args.seconds * args.rate)
    g = torch.Generator().manual_seed(0)
    amp = torch.where((torch.arange(n) // (args.rate // 2)) % 2 == 0, 8000.0, 8000.0 * 10.0 ** (-30.0 / 20.0))
    pcm = torch.round((torch.rand(args.items, n, generator=g) * 2.0 - 1.0) * amp).to(torch.int16).to(dev)
    lengths = torch.full((args.items,), n, dtype=torch.int64, device=dev)
    target, ceiling = -23.0, 0.99
    try:
        import torchaudio.functional  # noqa: F401
        use_lfilter = True
    except Exception:
        use_lfilter = False
    hip = LoudnessNormalizer(dev, args.rate, target_lufs=target, peak_ceiling=ceiling)
    stock = stock_arm(args.rate, target, ceiling, 1.0 / 32768.0, use_lfilter)
    arms = {"hip": (lambda: hip(pcm, lengths, return_stats=True), args.calls, args.warmup),
            "stock": (lambda: stock(pcm, lengths), args.stock_calls, 1)}
    outs = {}
    for name, (fn, _, warm) in arms.items():
        for _ in range(warm):
            outs[name] = fn()
    torch.cuda.synchronize()
    lufs_diff = float((outs["hip"][1] - outs["stock"][1]).abs().max())
    out_diff = float((outs["hip"][0] - outs["stock"][0]).abs().max())
    times = {name: [] for name in arms}
    for _ in range(args.rounds):
        for name, (fn, calls, _) in arms.items():
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            for _ in range(calls):
                fn()
            t1.record()
            torch.cuda.synchronize()
            times[name].append(t0.elapsed_time(t1) / calls)
    h = args.rate // 10
    bytes_design = args.items * (2 * n + 2 * n + 4 * n)          # the filter reads every sample, the copy reads it again, every output is written
    nseg = -(-n // SEG)
    filter_samples = args.items * sum(min(s * SEG, 2 * h) + min(SEG, n - s * SEG) for s in range(nseg))
    lines = []
    for name, (fn, calls, warm) in arms.items():
        med = statistics.median(times[name])
        count, rows = kernels_of(fn) if (name == "hip" or use_lfilter) else (None, None)       # (a profile of the stepped arm is thousands of rows)
        line = dict(leg=name, ms_median=round(med, 4), ms_min=round(min(times[name]), 4), ms_rounds=[round(t, 4) for t in times[name]], calls=calls,
                    warmup=warm, items=args.items, samples=n, rate=args.rate, launches=count, kernel_us=rows)
        if name == "hip":
            line.update(bytes_design=bytes_design, share_of_hbm_peak_design=bytes_design / (med * 1e-3) / HBM_PEAK, segment=SEG, warmup_samples=2 * h,
                        filter_samples_with_warmup=filter_samples, filter_fp64_ops=13 * filter_samples)
            if rows:
                us = [t for k, t in rows.items() if "loud_filter" in k]
                if us:
                    line.update(filter_us=us[0], filter_fp64_gops=round(13 * filter_samples / (us[0] * 1e-6) / 1e9, 2),
                                filter_share_of_hbm_peak=args.items * 2 * n / (us[0] * 1e-6) / HBM_PEAK)
        else:
            line.update(filter="torchaudio.functional.lfilter" if use_lfilter else "segmented recurrence, one sample per step")
        lines.append(line)
    hip_ms, stock_ms = statistics.median(times["hip"]), statistics.median(times["stock"])
    lines.append(dict(summary="loudness", hip_ms=round(hip_ms, 4), stock_torch_ms=round(stock_ms, 4), stock_over_hip=round(stock_ms / hip_ms, 3),
                      hip_vs_stock_max_abs_lufs_diff=lufs_diff, hip_vs_stock_max_abs_diff=out_diff,
                      mean_lufs=float(outs["hip"][1].mean()), device=torch.cuda.get_device_name(0)))
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        for line in lines:
            f.write(json.dumps(line) + "\n")
            print(json.dumps(line), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
