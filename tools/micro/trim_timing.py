"""Time the on-device silence trimmer against the same algorithm in stock PyTorch ops on the same GPU; writes profiles/trim_timing.json.

Workload: 64 x 10 s of 22 050 Hz int16 PCM, about 0.3 s of low-level noise (52 dB under the middle) at both ends of every item; frame 1024,
hop 256, top_db 40, 2 frames kept, peak 0.95.  Arms, interleaved inside one process after a warm-up:
  hip   : SilenceTrimmer (efts_trim_pcm16: int16 in, fp32 out, three launches);
  stock : float64 cumulative sum of the squares -> frame energies as differences, the same fp64 threshold decision, argmax bounds, a masked
          abs-max peak, a gather copy with the gain.
Reported per arm: ms per call (median and min over the rounds) and the device kernels of one call as the profiler lists them (count and
time per kernel name; None when the profiler is not available).  For the HIP arm also the bytes its design moves -- the input read twice
(energies, copy), the output written once -- over the time, as a share of the 8.0 TB/s HBM peak the design document's rooflines use, and the
same for the least any algorithm must move (input once, output once).  Bounds and lengths of the two arms are compared with ==.
Not a gate: nothing asserts on the times.

    python tools/micro/trim_timing.py [--items 64] [--seconds 10] [--rounds 5] [--calls 10]
"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from efficient_tts_amd.trim import SilenceTrimmer  # noqa: E402

HBM_PEAK = 8.0e12


def stock_arm(W: int, H: int, ratio: float, keep: int, peak: float):
    pad = (W - H) // 2

    def run(pcm: torch.Tensor, lengths: torch.Tensor):
        B, n = pcm.shape
        x = pcm.to(torch.float32)
        pos = torch.arange(n, device=pcm.device)
        x = torch.where(pos[None, :] < lengths[:, None], x, torch.zeros((), device=pcm.device))
        cs = torch.nn.functional.pad(torch.cumsum(x.double() ** 2, dim=1), (1, 0))               # cs[i] = sum of the first i squares
        T = -(-n // H)
        t = torch.arange(T, device=pcm.device)
        lo, hi = (t * H - pad).clamp(0, n), (t * H - pad + W).clamp(0, n)
        energy = cs[:, hi] - cs[:, lo]
        frames = torch.div(lengths + (H - 1), H, rounding_mode="floor")
        energy = torch.where(t[None, :] < frames[:, None], energy, torch.zeros((), dtype=torch.float64, device=pcm.device))
        e_max = energy.max(dim=1, keepdim=True).values
        sound = (energy * ratio > e_max) & (e_max > 0)
        any_sound = sound.any(dim=1)
        first = torch.argmax(sound.to(torch.int8), dim=1)
        last = T - 1 - torch.argmax(sound.flip(1).to(torch.int8), dim=1)
        start = torch.where(any_sound, ((first - keep) * H).clamp(min=0), torch.zeros_like(first))
        end = torch.where(any_sound, torch.minimum((last + 1 + keep) * H, lengths), lengths)
        kept = (pos[None, :] >= start[:, None]) & (pos[None, :] < end[:, None])
        p = torch.where(kept, x.abs(), torch.zeros((), device=pcm.device)).max(dim=1).values
        gain = torch.where(p > 0, torch.tensor(peak, dtype=torch.float32, device=pcm.device) / p, torch.ones((), device=pcm.device))
        idx = (start[:, None] + pos[None, :]).clamp(max=n - 1)
        out = torch.where(pos[None, :] < (end - start)[:, None], torch.gather(x, 1, idx) * gain[:, None], torch.zeros((), device=pcm.device))
        return out, end - start, start, gain
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
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", type=str, default=os.path.join(ROOT, "profiles", "trim_timing.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise RuntimeError("no MI355X (gfx950) device visible: nothing to time")
    dev = torch.device("cuda:0")
    n, quiet = int(args.seconds * args.rate), int(0.3 * args.rate)
    g = torch.Generator().manual_seed(0)
    amp = torch.full((n,), 8000.0)
    amp[:quiet] = amp[n - quiet:] = 20.0
    pcm = torch.round((torch.rand(args.items, n, generator=g) * 2.0 - 1.0) * amp).to(torch.int16).to(dev)
    lengths = torch.full((args.items,), n, dtype=torch.int64, device=dev)
    W, H, keep, peak = 1024, 256, 2, 0.95
    hip = SilenceTrimmer(dev, W, H, top_db=40.0, keep_frames=keep, peak=peak)
    stock = stock_arm(W, H, hip.ratio, keep, peak)
    arms = {"hip": lambda: hip(pcm, lengths, return_bounds=True), "stock": lambda: stock(pcm, lengths)}
    outs = {}
    for name, fn in arms.items():
        for _ in range(args.warmup):
            outs[name] = fn()
    torch.cuda.synchronize()
    same_bounds = bool(torch.equal(outs["hip"][1], outs["stock"][1]) and torch.equal(outs["hip"][2], outs["stock"][2]))
    diff = float((outs["hip"][0] - outs["stock"][0]).abs().max())
    removed = float((lengths - outs["hip"][1]).double().mean()) / args.rate
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
    kept = int(outs["hip"][1].sum())
    bytes_design = args.items * (2 * n) + 2 * kept + args.items * 4 * n          # energies read every sample, the copy reads the kept ones, every output is written
    bytes_least = args.items * (2 * n + 4 * n)
    lines = []
    for name, fn in arms.items():
        med = statistics.median(times[name])
        count, rows = kernels_of(fn)
        line = dict(leg=name, ms_median=round(med, 4), ms_min=round(min(times[name]), 4), ms_rounds=[round(t, 4) for t in times[name]], calls=args.calls,
                    warmup=args.warmup, items=args.items, samples=n, frame_length=W, hop=H, launches=count, kernel_us=rows)
        if name == "hip":
            line.update(bytes_design=bytes_design, share_of_hbm_peak_design=bytes_design / (med * 1e-3) / HBM_PEAK, bytes_least=bytes_least,
                        share_of_hbm_peak_least=bytes_least / (med * 1e-3) / HBM_PEAK)
        lines.append(line)
    hip_ms, stock_ms = statistics.median(times["hip"]), statistics.median(times["stock"])
    lines.append(dict(summary="trim", hip_ms=round(hip_ms, 4), stock_torch_ms=round(stock_ms, 4), stock_over_hip=round(stock_ms / hip_ms, 3),
                      same_bounds=same_bounds, hip_vs_stock_max_abs_diff=diff, mean_seconds_removed=round(removed, 4),
                      device=torch.cuda.get_device_name(0)))
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        for line in lines:
            f.write(json.dumps(line) + "\n")
            print(json.dumps(line), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
