"""Time the on-device look-ahead limiter and the true-peak meter against the same algorithm in stock PyTorch ops on the same GPU; writes
profiles/limiter_timing.json.

Workload: 64 x 10 s of 22 050 Hz fp32 (uniform noise of amplitude 0.3 with a full-scale sample every 4001), ceiling -1 dBTP, hold = smooth =
33.  Arms, interleaved inside one process after a warm-up:
  hip   : PeakLimiter (efts_peak_limit: two launches) and TruePeakMeter (efts_true_peak: two launches);
  stock : `conv1d` with the three phases as output channels, `max_pool1d` on -r for the hold, `avg_pool1d` for the mean, elementwise ops for
          the rest (its box sum is in another order than the definition's: the outputs are compared, not expected to be equal).
Reported per arm: ms per call (median, min and every round) and the device kernels of one call as the profiler lists them.  For the HIP arms
also the bytes that the design moves from HBM -- the limiter reads every sample once and writes it once, the meter reads it once; what the
chunks' halos re-read comes from the caches -- over the time, as a share of the 8.0 TB/s HBM peak.  Not a gate: nothing asserts on the times.
Not measured: int16 input, other holds than 33, other batch shapes, and the cost inside the synthesis command line.

    python tools/micro/limiter_timing.py [--items 64] [--seconds 10] [--rounds 5] [--calls 10]
"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from efficient_tts_amd.limiter import PeakLimiter, TruePeakMeter, true_peak_table  # noqa: E402

HBM_PEAK = 8.0e12


def stock_arm(ceiling: float, hold: int, smooth: int, dev):
    taps = torch.from_numpy(true_peak_table()[1:].copy()).to(dev)[:, None, :]              # [3, 1, 25]: cross-correlation, as the definition

    def run(x: torch.Tensor):
        phases = torch.nn.functional.conv1d(x[:, None, :], taps, padding=12)
        p = torch.maximum(x.abs(), phases.abs().amax(dim=1))
        r = torch.where(p > ceiling, ceiling / p.clamp(min=1e-30), torch.ones((), device=dev))
        # m on -smooth .. n + smooth - 1 with r = 1 outside the item, then the mean over 2 smooth + 1
        rp = torch.nn.functional.pad(r, (hold + smooth, hold + smooth), value=1.0)
        m = -torch.nn.functional.max_pool1d(-rp[:, None, :], 2 * hold + 1, stride=1)
        mean = torch.nn.functional.avg_pool1d(m, 2 * smooth + 1, stride=1)[:, 0, :]
        g = torch.minimum(r, mean)
        return x * g, g.amin(dim=1), (g < 1).sum(dim=1), p.amax(dim=1)
    return run


def kernels_of(fn):
    """(count, {kernel name: device us}) of one call as torch.profiler lists it, or (None, None) when it is not available"""
    try:
        from torch.profiler import ProfilerActivity, profile
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        rows, count = {}, 0
        for ev in prof.events():
            if str(getattr(ev, "device_type", "")).endswith("CUDA") and "memcpy" not in ev.name.lower() and "memset" not in ev.name.lower():
                t = float(getattr(ev, "device_time_total", 0.0) or getattr(ev, "cuda_time_total", 0.0) or 0.0)
                count += 1
                rows[ev.name[:96]] = round(rows.get(ev.name[:96], 0.0) + t, 2)
        return (count, rows) if count else (None, None)
    except Exception as exc:                                   # the profiler is a convenience here, the times do not depend on it
        print(f"profiler not available: {exc!r}", flush=True)
        return None, None


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--items", type=int, default=64)
    ap.add_argument("--seconds", type=float, default=10.0)
    ap.add_argument("--rate", type=int, default=22050)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", type=str, default=os.path.join(ROOT, "profiles", "limiter_timing.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise RuntimeError("no MI355X (gfx950) device visible: nothing to time")
    dev = torch.device("cuda:0")
    n = int(args.seconds * args.rate)
    g = torch.Generator().manual_seed(0)
    x = (torch.rand(args.items, n, generator=g) * 2.0 - 1.0) * 0.3
    x[:, 1000::4001] = 1.0
    x = x.to(dev)
    hip = PeakLimiter(dev, args.rate, ceiling_dbtp=-1.0)
    meter = TruePeakMeter(dev)
    stock = stock_arm(hip.ceiling, hip.hold, hip.smooth, dev)
    arms = {"hip_limiter": lambda: hip(x, return_stats=True), "hip_meter": lambda: meter(x), "stock_limiter": lambda: stock(x)}
    outs = {}
    for name, fn in arms.items():
        for _ in range(args.warmup):
            outs[name] = fn()
    torch.cuda.synchronize()
    out_diff = float((outs["hip_limiter"][0] - outs["stock_limiter"][0]).abs().max())
    limited = (int(outs["hip_limiter"][2].sum()), int(outs["stock_limiter"][2].sum()))
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
    design = {"hip_limiter": args.items * n * 8, "hip_meter": args.items * n * 4}
    lines = []
    for name, fn in arms.items():
        med = statistics.median(times[name])
        count, rows = kernels_of(fn)
        line = dict(leg=name, ms_median=round(med, 4), ms_min=round(min(times[name]), 4), ms_max=round(max(times[name]), 4),
                    ms_rounds=[round(t, 4) for t in times[name]], calls=args.calls, warmup=args.warmup, items=args.items, samples=n, rate=args.rate,
                    launches=count, kernel_us=rows)
        if name in design:
            line.update(bytes_design=design[name], share_of_hbm_peak_design=design[name] / (med * 1e-3) / HBM_PEAK)
        lines.append(line)
    hip_ms, stock_ms = statistics.median(times["hip_limiter"]), statistics.median(times["stock_limiter"])
    lines.append(dict(summary="limiter", hip_ms=round(hip_ms, 4), stock_torch_ms=round(stock_ms, 4), stock_over_hip=round(stock_ms / hip_ms, 3),
                      hip_vs_stock_max_abs_diff=out_diff, limited_samples_hip_stock=limited, hold=hip.hold, smooth=hip.smooth, ceiling=hip.ceiling,
                      not_measured="int16 input, other holds, other batch shapes, the cost inside bin/inference.py",
                      device=torch.cuda.get_device_name(0)))
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        for line in lines:
            f.write(json.dumps(line) + "\n")
            print(json.dumps(line), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
