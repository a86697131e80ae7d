"""Time the on-device IIR filter against the same segmented recurrence in stock PyTorch ops on the same GPU, and beside the filter launch
of the loudness meter; writes profiles/iir_timing.json.

Workload: 64 x 10 s of 22 050 Hz fp32 (uniform noise of amplitude 0.3 on a DC offset of 0.1).  Arms, interleaved inside one process after
a warm-up:
  hip_highpass4   : IIRFilter with the order-4 Butterworth high-pass at 20 Hz (two sections; efts_iir: three launches);
  hip_deemphasis  : IIRFilter with de-emphasis 0.97 (one section);
  stock_highpass4 : the same scheme from stock ops in float64 -- every segment of 256 samples from zero state, one sample per step over all
                    segments at once; the state carried across the segments by a log-step scan with M^(2^k) (M from the recurrence, the
                    powers by squaring); every segment again from its start state.  Its sums are in another order: the outputs are compared,
                    not expected to be equal.  torchaudio is not installed, so there is no `lfilter` arm.
  loudness        : for context only, one LoudnessNormalizer call on the same batch, of which the filter launch is read off the profile.
Reported per arm: ms per call (median, min, max and every round) and the device kernels of one call as the profiler lists them -- for the HIP
arms that is the time per launch.  For the HIP arms also the bytes that the design moves from HBM -- launch A reads every sample, launch C
reads it again and writes the output: 12 bytes per sample, plus 64 bytes per segment written and read back by each of A, B and C -- over
the time, as a share of the 8.0 TB/s HBM peak, and the dependent fp64 operations that bound the launches by the code: A and C are chains of
256 samples x 2 dependent fma per section per thread (the sections of one sample overlap), B is 7 matrix-vector products per 64 segments
of one wave.  Not a gate: nothing asserts on the times.  Not measured: hardware counters, int16 input, other lengths and batch shapes.

    python tools/micro/iir_timing.py [--items 64] [--seconds 10] [--rounds 5] [--calls 10] [--stock_calls 1]
"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from efficient_tts_amd.iir import SEGMENT, IIRFilter, deemphasis_sos, highpass_sos  # noqa: E402
from efficient_tts_amd.loudness import LoudnessNormalizer  # noqa: E402

HBM_PEAK = 8.0e12


def _steps(sos, state, x, keep: bool):
    """the cascade over x [rows, steps] from state [2K, rows]; returns (y [rows, steps] or None, state)"""
    y = torch.empty_like(x) if keep else None
    state = list(state)
    for i in range(x.shape[1]):
        v = x[:, i]
        for q, (b0, b1, b2, a1, a2) in enumerate(sos):
            o = b0 * v + state[2 * q]
            state[2 * q] = b1 * v - a1 * o + state[2 * q + 1]
            state[2 * q + 1] = b2 * v - a2 * o
            v = o
        if keep:
            y[:, i] = v
    return y, torch.stack(state)


def stock_arm(sos, dev):
    sos = [tuple(float(c) for c in row) for row in sos]
    n_state = 2 * len(sos)
    eye = torch.eye(n_state, dtype=torch.float64, device=dev)
    m = _steps(sos, eye, torch.zeros(n_state, SEGMENT, dtype=torch.float64, device=dev), False)[1]       # column i: from e_i

    def run(x: torch.Tensor):
        B, n = x.shape
        nseg = -(-n // SEGMENT)
        seg = torch.nn.functional.pad(x.double(), (0, nseg * SEGMENT - n)).reshape(B * nseg, SEGMENT)
        zero = torch.zeros(n_state, B * nseg, dtype=torch.float64, device=dev)
        p = _steps(sos, zero, seg, False)[1].reshape(n_state, B, nseg)                                   # end states from zero state
        power, d = m, 1
        while d < nseg:                                                                                  # inclusive scan along the segments
            shifted = torch.nn.functional.pad(p[:, :, :-d], (d, 0))
            p = p + torch.einsum("ij,jbs->ibs", power, shifted)
            power, d = power @ power, 2 * d
        start = torch.nn.functional.pad(p[:, :, :-1], (1, 0)).reshape(n_state, B * nseg)
        y = _steps(sos, start, seg, True)[0]
        return y.reshape(B, nseg * SEGMENT)[:, :n].float()
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
    ap.add_argument("--stock_calls", type=int, default=1, help="calls per round of the stock arm (one call is thousands of launches)")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", type=str, default=os.path.join(ROOT, "profiles", "iir_timing.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise RuntimeError("no MI355X (gfx950) device visible: nothing to time")
    dev = torch.device("cuda:0")
    n = int(args.seconds * args.rate)
    g = torch.Generator().manual_seed(0)
    x = ((torch.rand(args.items, n, generator=g) * 2.0 - 1.0) * 0.3 + 0.1).to(dev)
    hp = highpass_sos(args.rate, 20.0, 4)
    hip_hp, hip_de = IIRFilter(dev, hp), IIRFilter(dev, deemphasis_sos(0.97))
    stock = stock_arm(hp, dev)
    loud = LoudnessNormalizer(dev, args.rate, target_lufs=-23.0)
    arms = {"hip_highpass4": (lambda: hip_hp(x), args.calls, args.warmup), "hip_deemphasis": (lambda: hip_de(x), args.calls, args.warmup),
            "loudness": (lambda: loud(x), args.calls, args.warmup), "stock_highpass4": (lambda: stock(x), args.stock_calls, 1)}
    outs = {}
    for name, (fn, _, warmup) in arms.items():
        for _ in range(warmup):
            outs[name] = fn()
    torch.cuda.synchronize()
    out_diff = float((outs["hip_highpass4"] - outs["stock_highpass4"]).abs().max())
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
    nseg = -(-n // SEGMENT)
    bytes_design = args.items * (n * 12 + nseg * 64 * 4)
    lines, loud_filter_us, launch_us = [], None, {}
    for name, (fn, calls, warmup) in arms.items():
        med = statistics.median(times[name])
        count, rows = kernels_of(fn) if name != "stock_highpass4" else (None, None)        # (a profile of the stepped arm is thousands of rows)
        line = dict(leg=name, ms_median=round(med, 4), ms_min=round(min(times[name]), 4), ms_max=round(max(times[name]), 4),
                    ms_rounds=[round(t, 4) for t in times[name]], calls=calls, warmup=warmup, items=args.items, samples=n, rate=args.rate,
                    launches=count, kernel_us=rows)
        if name.startswith("hip_"):
            sections = hip_hp.sections if name == "hip_highpass4" else hip_de.sections
            line.update(sections=sections, bytes_design=bytes_design, share_of_hbm_peak_design=bytes_design / (med * 1e-3) / HBM_PEAK,
                        dependent_fma_per_thread_launch_a_and_c=2 * sections * SEGMENT,
                        dependent_matvec_per_item_launch_b=7 * -(-nseg // 64), bound_by="the dependent fp64 chain of a thread (A, C) and of the "
                        "one wave per item (B), by the code; no counter was read")
            if rows:
                launch_us[name] = {k: v for k, v in rows.items() if "iir_" in k}
        if name == "loudness" and rows:
            us = [t for k, t in rows.items() if "loud_filter" in k]
            loud_filter_us = us[0] if us else None
            line.update(filter_launch_us=loud_filter_us)
        lines.append(line)
    hip_ms, de_ms, stock_ms = (statistics.median(times[k]) for k in ("hip_highpass4", "hip_deemphasis", "stock_highpass4"))
    lines.append(dict(summary="iir", hip_highpass4_ms=round(hip_ms, 4), hip_deemphasis_ms=round(de_ms, 4), stock_torch_ms=round(stock_ms, 4),
                      stock_over_hip=round(stock_ms / hip_ms, 3), hip_vs_stock_max_abs_diff=out_diff, launch_us=launch_us,
                      loudness_filter_launch_ms=None if loud_filter_us is None else round(loud_filter_us * 1e-3, 4),
                      hip_highpass4_over_loudness_filter_launch=None if loud_filter_us is None else round(hip_ms / (loud_filter_us * 1e-3), 4),
                      not_measured="hardware counters, int16 input, other lengths and batch shapes, the cost inside the training and synthesis commands",
                      device=torch.cuda.get_device_name(0)))
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        for line in lines:
            f.write(json.dumps(line) + "\n")
            print(json.dumps(line), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
