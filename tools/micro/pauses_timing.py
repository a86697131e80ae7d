"""Time the on-device pause shortener against the same algorithm in stock PyTorch ops on the same GPU and against the silence trimmer on the
same batch; writes profiles/pauses_timing.json.

Workload: 64 x 10 s of 22 050 Hz, as int16 PCM and as fp32: noise at 8000 counts with three pauses of 0.2, 0.5 and 1.0 s (20 counts, 52 dB
under it) inside every item; frame 1024, hop 256, top_db 40, max_pause_ms 300 (26 hops), 64 samples of fade.  Arms, interleaved inside one
process after a warm-up, events around `--calls` calls, `--rounds` rounds:
  hip_pcm16, hip_fp32   : PauseShortener (efts_pauses_pcm16 / efts_pauses: three launches);
  stock_pcm16           : frame energies by unfold in float64, the same fp64 threshold decision, run lengths by cummax / flip, the cumsum of the
                          keep flags, scatters for chunk_src and the joints, a gather copy with the fade.  Its plan (new lengths, removed,
                          pauses, chunk_src) is compared with the kernel's by ==, its samples by the largest difference;
  trim_pcm16, trim_fp32 : SilenceTrimmer on the same batch, the in-house yardstick: it moves the same bytes (input read twice, output
                          written once).
Reported per arm: ms per call (median and min over the rounds) and the device kernels of one call as the profiler lists them (count and time
per kernel name; None when the profiler is not available) -- the per-launch times.  For the HIP arms also the bytes the design moves (every
input sample read by the energies, the kept ones read by the copy, every output written) over the time, as a share of the 8.0 TB/s HBM peak.
Not a gate: nothing asserts on the times.  Hardware counters: not collected.

    python tools/micro/pauses_timing.py [--items 64] [--seconds 10] [--rounds 5] [--calls 10]
"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from efficient_tts_amd.pauses import PauseShortener, fade_table  # noqa: E402
from efficient_tts_amd.trim import SilenceTrimmer  # noqa: E402

HBM_PEAK = 8.0e12


def stock_arm(W: int, H: int, ratio: float, M: int, F: int, scale: float):
    pad = (W - H) // 2
    head, tail = (M + 1) // 2, M // 2

    def run(pcm: torch.Tensor, lengths: torch.Tensor):
        B, n = pcm.shape
        dev = pcm.device
        pos = torch.arange(n, device=dev)
        inside = pos[None, :] < lengths[:, None]
        sq = torch.where(inside, pcm.double() ** 2, torch.zeros((), dtype=torch.float64, device=dev))
        T = -(-n // H)
        energy = torch.nn.functional.pad(sq, (pad, W + H)).unfold(1, W, H)[:, :T].sum(dim=2)
        t = torch.arange(T, device=dev)
        frames = torch.div(lengths + (H - 1), H, rounding_mode="floor")
        real = t[None, :] < frames[:, None]
        energy = torch.where(real, energy, torch.zeros((), dtype=torch.float64, device=dev))
        e_max = energy.max(dim=1, keepdim=True).values
        sound = energy * ratio > e_max
        prev = torch.cummax(torch.where(sound, t[None, :], torch.full((), -1, device=dev)), dim=1).values
        nxt = torch.cummin(torch.where(sound, t[None, :], torch.full((), T, device=dev)).flip(1), dim=1).values.flip(1)
        in_pause = ~sound & (prev >= 0) & (nxt < T)
        length, at = nxt - prev - 1, t[None, :] - prev - 1
        cut = in_pause & (length > M)
        drop = cut & (at >= head) & (at < length - tail)
        joint = cut & (at == head - 1)
        keep = real & ~drop
        dst = torch.cumsum(keep, dim=1) - keep.long()
        slot = torch.where(keep, dst, torch.full((), T, device=dev))
        chunk_src = torch.full((B, T + 1), -1, dtype=torch.long, device=dev).scatter_(1, slot, t[None, :].expand(B, T))[:, :T]
        fade_into = torch.full((B, T + 1), -1, dtype=torch.long, device=dev).scatter_(
            1, slot, torch.where(joint, (nxt - tail) * H, torch.full((), -1, device=dev)))[:, :T]
        removed = (frames - keep.sum(dim=1)) * H
        new_len = lengths - removed
        x = pcm.to(torch.float32) * scale if pcm.dtype == torch.int16 else pcm
        j, k = torch.div(pos, H, rounding_mode="floor"), pos % H
        sc, jb = chunk_src[:, j], fade_into[:, j]
        xa = torch.gather(x, 1, (sc * H + k[None, :]).clamp(0, n - 1))
        kk = k - (H - F)
        faded = (jb >= 0) & (kk >= 0)[None, :]
        out = xa
        if F > 0:
            w = torch.from_numpy(fade_table(F)).to(dev)
            xb = torch.gather(x, 1, (jb - F + kk[None, :]).clamp(0, n - 1))
            out = torch.where(faded, xa + w[kk.clamp(min=0)][None, :] * (xb - xa), xa)
        out = torch.where(pos[None, :] < new_len[:, None], out, torch.zeros((), device=dev))
        return out, new_len, {"removed": removed, "pauses": joint.sum(dim=1), "chunk_src": chunk_src.to(torch.int32)}
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


def workload(items: int, n: int, rate: int) -> torch.Tensor:
    g = torch.Generator().manual_seed(0)
    amp = torch.full((n,), 8000.0)
    at = n // 8
    for seconds in (0.2, 0.5, 1.0):
        amp[at:at + int(seconds * rate)] = 20.0
        at += int(seconds * rate) + n // 5
    return torch.round((torch.rand(items, n, generator=g) * 2.0 - 1.0) * amp).to(torch.int16)


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--items", type=int, default=64)
    ap.add_argument("--seconds", type=float, default=10.0)
    ap.add_argument("--rate", type=int, default=22050)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", type=str, default=os.path.join(ROOT, "profiles", "pauses_timing.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise RuntimeError("no MI355X (gfx950) device visible: nothing to time")
    dev = torch.device("cuda:0")
    n = int(args.seconds * args.rate)
    pcm = workload(args.items, n, args.rate).to(dev)
    f32 = pcm.to(torch.float32) * (1.0 / 32768.0)
    lengths = torch.full((args.items,), n, dtype=torch.int64, device=dev)
    W, H, F = 1024, 256, 64
    hip = PauseShortener(dev, args.rate, max_pause_ms=300.0, frame_length=W, hop_size=H, top_db=40.0, fade=F)
    trim = SilenceTrimmer(dev, W, H, top_db=40.0, keep_frames=2)
    stock = stock_arm(W, H, hip.ratio, hip.chunks, F, 1.0 / 32768.0)
    arms = {"hip_pcm16": lambda: hip(pcm, lengths, return_stats=True), "hip_fp32": lambda: hip(f32, lengths, return_stats=True),
            "stock_pcm16": lambda: stock(pcm, lengths), "trim_pcm16": lambda: trim(pcm, lengths), "trim_fp32": lambda: trim(f32, lengths)}
    outs = {}
    for name, fn in arms.items():
        for _ in range(args.warmup):
            outs[name] = fn()
    torch.cuda.synchronize()
    a, b = outs["hip_pcm16"], outs["stock_pcm16"]
    same_plan = bool(torch.equal(a[1], b[1]) and all(torch.equal(a[2][k], b[2][k]) for k in ("removed", "pauses", "chunk_src")))
    diff = float((a[0] - b[0]).abs().max())
    twin = outs["hip_fp32"]
    same_twin = bool(torch.equal(a[1], twin[1]) and all(torch.equal(a[2][k], twin[2][k]) for k in ("removed", "pauses", "chunk_src")))
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
    kept = int(a[1].sum())
    lines = []
    for name, fn in arms.items():
        med = statistics.median(times[name])
        count, rows = kernels_of(fn)
        line = dict(leg=name, ms_median=round(med, 4), ms_min=round(min(times[name]), 4), ms_rounds=[round(t, 4) for t in times[name]], calls=args.calls,
                    warmup=args.warmup, items=args.items, samples=n, frame_length=W, hop=H, launches=count, kernel_us=rows)
        if name.startswith("hip"):
            size = 2 if name.endswith("pcm16") else 4
            moved = args.items * size * n + size * kept + args.items * 4 * n
            line.update(bytes_design=moved, share_of_hbm_peak_design=moved / (med * 1e-3) / HBM_PEAK)
        lines.append(line)
    med = {name: statistics.median(times[name]) for name in arms}
    lines.append(dict(summary="pauses", hip_pcm16_ms=round(med["hip_pcm16"], 4), hip_fp32_ms=round(med["hip_fp32"], 4),
                      stock_torch_pcm16_ms=round(med["stock_pcm16"], 4), trim_pcm16_ms=round(med["trim_pcm16"], 4), trim_fp32_ms=round(med["trim_fp32"], 4),
                      stock_over_hip=round(med["stock_pcm16"] / med["hip_pcm16"], 3), hip_over_trim_pcm16=round(med["hip_pcm16"] / med["trim_pcm16"], 3),
                      hip_over_trim_fp32=round(med["hip_fp32"] / med["trim_fp32"], 3), stock_plan_equals_hip=same_plan, fp32_plan_equals_pcm16=same_twin,
                      hip_vs_stock_max_abs_diff=diff, pauses_cut_per_item=float(a[2]["pauses"].double().mean()),
                      mean_seconds_removed=round(float(a[2]["removed"].double().mean()) / args.rate, 4), max_pause_chunks=hip.chunks,
                      hardware_counters="not measured", device=torch.cuda.get_device_name(0)))
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        for line in lines:
            f.write(json.dumps(line) + "\n")
            print(json.dumps(line), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
