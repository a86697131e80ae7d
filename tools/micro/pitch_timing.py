"""Time the pitch tracker, its smoother and the path-returning DTW on the GPU; writes profiles/pitch_timing.json and
profiles/pitch_viterbi_timing.json.

Three measurements, every arm warmed up first and the arms of one measurement interleaved round by round inside one process:
  yin      : efts_yin_pcm16 on 64 items x 800 frames of int16 PCM (n_fft 1024, hop 256, 60 .. 600 Hz: lags 36 .. 367), against the same YIN on
             stock torch ops on the same GPU -- `unfold` for the frames, a broadcast difference per block of lags, `cumsum` for the running sum,
             the decision by masks and `gather`.  The stock arm cannot hold [B, T, lags, W] at once (64 x 800 x 367 x 512 floats = 38 GB), so it
             walks the batch in slices of `--stock_items` items and 32 lags, as a user of stock ops would have to.
  dtw_path : efts_dtw_path against efts_dtw on the 64 ragged pairs of tools/micro/score_timing.py: what the move record and the back-trace cost.
  f0_error : efts_f0_path_error on those paths (one small launch).
  viterbi  : (its own file) efts_f0_viterbi on the 64 x 800 frames of d' that the yin measurement's kernel wrote, lags 36 .. 367, against the same
             integer recurrence on stock torch ops on the same GPU -- per frame one broadcast add [B, S + 1, S + 1] and one min over the
             predecessors, then the back-trace by `gather` -- and the tracker's call with and without `smooth=True`: what smoothing adds to it.
Reported per arm: ms per call (median and min over the rounds); for yin also the fused multiply-adds of the difference function per second,
counted from the shapes (frames x lags x W), which is what bounds the kernel.  Not a gate: nothing asserts on the times.

    python tools/micro/pitch_timing.py [--items 64] [--frames 800] [--rounds 5] [--measure all|viterbi]
"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from efficient_tts_amd.pitch import Q16, PitchTracker, ViterbiSmoother, log2_table  # noqa: E402
from efficient_tts_amd.score import F0Error, dtw, dtw_path  # noqa: E402

SR, N_FFT, HOP = 22050, 1024, 256


def stock_yin(audio, lengths, tau_min, tau_max, threshold, items_per_slice):
    """f0 [B, T] by stock ops (int16 in, frames as the front-end's: reflect padding per item is replaced by one reflect pad of the padded batch,
    which only changes the last frames of the shorter items: the arm is a yardstick for time, and is compared on full-length items)"""
    B, n = audio.shape
    W, pad = N_FFT // 2, (N_FFT - HOP) // 2
    T = n // HOP
    out = torch.zeros(B, T, device=audio.device)
    taus = torch.arange(1, tau_max + 1, device=audio.device)
    for b0 in range(0, B, items_per_slice):
        x = audio[b0:b0 + items_per_slice].float() / 32768.0
        x = torch.nn.functional.pad(x[:, None], (pad, pad), mode="reflect")[:, 0]
        fr = x.unfold(1, N_FFT, HOP)[:, :T]                                     # [b, T, N]
        d = torch.empty(fr.shape[0], T, tau_max, device=audio.device)
        for t0 in range(0, tau_max, 32):
            k = taus[t0:t0 + 32]
            idx = torch.arange(W, device=audio.device)[None, :] + k[:, None]     # [k, W]
            d[:, :, t0:t0 + 32] = ((fr[:, :, None, :W] - fr[:, :, idx]) ** 2).sum(-1)
        run = d.cumsum(-1)
        dp = torch.where(run > 0, d * taus / run.clamp_min(1e-30), torch.ones_like(d))      # dp[..., k] = d'(k + 1)
        under = dp[..., tau_min - 1:tau_max - 1] < threshold
        first = torch.where(under.any(-1), under.float().argmax(-1) + tau_min, torch.zeros_like(under[..., 0], dtype=torch.long))
        tau = first.clone()
        for _ in range(8):                                                                   # the walk to the local minimum, a few steps at most
            nxt = (tau + 1).clamp(max=tau_max - 1)
            go = (tau > 0) & (nxt > tau) & (dp.gather(-1, (nxt - 1)[..., None])[..., 0] < dp.gather(-1, (tau - 1).clamp_min(0)[..., None])[..., 0])
            tau = torch.where(go, nxt, tau)
        tc = tau.clamp_min(2)
        s0, s1, s2 = (dp.gather(-1, (tc - 1 + o)[..., None])[..., 0] for o in (-1, 0, 1))
        den = (s0 - s1) + (s2 - s1)
        shift = torch.where(den != 0, 0.5 * (s0 - s2) / den, torch.zeros_like(den)).clamp(-1, 1)
        out[b0:b0 + items_per_slice] = torch.where(tau > 0, SR / (tc + shift), torch.zeros_like(shift))
    return out


def stock_viterbi(cmnd, tau_min, tau_max, costs_q):
    """lag [B, T] of full-length items by stock ops: the recurrence of include/efts_abi.h in int64, one broadcast add and one min per frame"""
    B, T, _ = cmnd.shape
    S = tau_max - tau_min
    uq, oq, jq, vq = costs_q
    lg = log2_table(tau_max).to(cmnd.device).long()[tau_min:tau_max]
    x = cmnd[:, :, tau_min:tau_max]
    obs = torch.where(x < 4.0, torch.round(x.clamp(-4.0, 4.0) * 65536.0), torch.full_like(x, 4.0 * Q16)).long() + ((oq * (lg - lg[0])) >> 16)
    obs = torch.cat([obs, torch.full((B, T, 1), uq, dtype=torch.long, device=cmnd.device)], dim=2)
    trans = torch.full((S + 1, S + 1), vq, dtype=torch.long, device=cmnd.device)
    trans[:S, :S] = (jq * (lg[None, :] - lg[:, None]).abs()) >> 16
    trans[S, S] = 0
    C = obs[:, 0]
    back = torch.empty(B, T, S + 1, dtype=torch.long, device=cmnd.device)
    for t in range(1, T):
        best, back[:, t] = (C[:, :, None] + trans[None]).min(dim=1)             # the first, i.e. lowest, index among equal minima is not promised by
        C = obs[:, t] + best                                                    # torch.min: the arm is a yardstick for time
    state = C.argmin(dim=1, keepdim=True)
    states = [state]
    for t in range(T - 1, 0, -1):
        state = back[:, t].gather(1, state)
        states.append(state)
    states = torch.cat(states[::-1], dim=1)
    return torch.where(states < S, states + tau_min, torch.zeros_like(states))


def timed(arms, calls, rounds):
    times = {name: [] for name in arms}
    for _ in range(rounds):
        for name, fn in arms.items():
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            for _ in range(calls[name]):
                fn()
            t1.record()
            torch.cuda.synchronize()
            times[name].append(t0.elapsed_time(t1) / calls[name])
    return times


def viterbi(args, dev, tracker, pcm, lengths):
    B, T = args.items, args.frames
    cmnd, frames = tracker(pcm, lengths, return_cmnd=True)[3], torch.full((B,), T, dtype=torch.int32, device=dev)
    smoother = ViterbiSmoother(dev, SR, tracker.tau_min, tracker.tau_max)
    smooth_tracker = PitchTracker(dev, sampling_rate=SR, n_fft=N_FFT, hop_size=HOP, smooth=True)
    arms = {"hip": lambda: smoother(cmnd, frames), "stock": lambda: stock_viterbi(cmnd, tracker.tau_min, tracker.tau_max, smoother.costs_q),
            "tracker": lambda: tracker(pcm, lengths), "tracker_smooth": lambda: smooth_tracker(pcm, lengths)}
    outs = {}
    for name, fn in arms.items():
        for _ in range(args.warmup):
            outs[name] = fn()
    torch.cuda.synchronize()
    hip_lag, stock_lag = outs["hip"][2].long(), outs["stock"]
    agree = float((hip_lag == stock_lag).float().mean())
    calls = {"hip": args.hip_calls, "stock": args.stock_calls, "tracker": args.hip_calls, "tracker_smooth": args.hip_calls}
    times = timed(arms, calls, args.rounds)
    lines = [dict(measurement="viterbi", leg=name, ms_median=round(statistics.median(times[name]), 4), ms_min=round(min(times[name]), 4),
                  ms_rounds=[round(v, 4) for v in times[name]], calls=calls[name], warmup=args.warmup, items=B, frames=T) for name in arms]
    med = {name: statistics.median(times[name]) for name in arms}
    S = tracker.tau_max - tracker.tau_min
    lines.append(dict(summary="viterbi", hip_ms=round(med["hip"], 4), stock_torch_ms=round(med["stock"], 4), stock_over_hip=round(med["stock"] / med["hip"], 2),
                      tracker_ms=round(med["tracker"], 4), tracker_smooth_ms=round(med["tracker_smooth"], 4),
                      smooth_over_plain_tracker=round(med["tracker_smooth"] / med["tracker"], 3),
                      us_per_frame_of_the_chain=round(med["hip"] * 1e3 / T, 3), state_pairs_unpruned=B * (T - 1) * (S + 1) * (S + 1),
                      lags=[tracker.tau_min, tracker.tau_max], voiced_share=round(float((hip_lag > 0).float().mean()), 4),
                      lag_agreement_with_stock=round(agree, 5), device=torch.cuda.get_device_name(0)))
    os.makedirs(os.path.dirname(args.viterbi_out), exist_ok=True)
    with open(args.viterbi_out, "w") as fh:
        for line in lines:
            fh.write(json.dumps(line) + "\n")
            print(json.dumps(line), flush=True)


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--items", type=int, default=64)
    ap.add_argument("--frames", type=int, default=800)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--hip_calls", type=int, default=100, help="kernel calls per round")
    ap.add_argument("--stock_calls", type=int, default=1, help="stock-torch YIN calls per round")
    ap.add_argument("--stock_items", type=int, default=4, help="items per slice of the stock-torch YIN")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", type=str, default=os.path.join(ROOT, "profiles", "pitch_timing.json"))
    ap.add_argument("--viterbi_out", type=str, default=os.path.join(ROOT, "profiles", "pitch_viterbi_timing.json"))
    ap.add_argument("--measure", type=str, default="all", choices=["all", "viterbi"], help="viterbi: only the smoother's measurement and its file")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise RuntimeError("no MI355X (gfx950) device visible: nothing to time")
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(0)
    B, T = args.items, args.frames
    n = T * HOP
    # voiced-like PCM: a gliding harmonic tone per item plus noise
    t = torch.arange(n, dtype=torch.float64)[None, :]
    f = 90.0 + 300.0 * torch.rand(B, 1, generator=g, dtype=torch.float64) + 20.0 * t / n
    phase = 2.0 * torch.pi * torch.cumsum(f / SR, dim=1)
    wave = sum(a * torch.sin((h + 1) * phase) for h, a in enumerate((1.0, 0.5, 0.25, 0.125))) / 1.875
    pcm = (wave * 20000.0 + 300.0 * torch.randn(B, n, generator=g, dtype=torch.float64)).round().clamp(-32768, 32767).to(torch.int16).to(dev)
    lengths = torch.full((B,), n)
    tracker = PitchTracker(dev, sampling_rate=SR, n_fft=N_FFT, hop_size=HOP)
    viterbi(args, dev, tracker, pcm, lengths)
    if args.measure == "viterbi":
        return 0
    lines = []

    arms = {"hip": lambda: tracker(pcm, lengths), "stock": lambda: stock_yin(pcm, lengths, tracker.tau_min, tracker.tau_max, 0.15, args.stock_items)}
    outs = {}
    for name, fn in arms.items():
        for _ in range(args.warmup):
            outs[name] = fn()
    torch.cuda.synchronize()
    hip_f0, stock_f0 = outs["hip"][0][:, 2:-2], outs["stock"][:, 2:-2]          # the frames whose samples need no reflection
    both = (hip_f0 > 0) & (stock_f0 > 0)
    agree = float(((hip_f0 > 0) == (stock_f0 > 0)).float().mean())
    rel = float(((hip_f0 - stock_f0).abs() / stock_f0.clamp_min(1.0))[both].median()) if bool(both.any()) else float("nan")
    calls = {"hip": args.hip_calls, "stock": args.stock_calls}
    times = timed(arms, calls, args.rounds)
    for name in arms:
        lines.append(dict(measurement="yin", leg=name, ms_median=round(statistics.median(times[name]), 4), ms_min=round(min(times[name]), 4),
                          ms_rounds=[round(v, 4) for v in times[name]], calls=calls[name], warmup=args.warmup, items=B, frames=T))
    hip_ms, stock_ms = statistics.median(times["hip"]), statistics.median(times["stock"])
    fma = B * T * tracker.tau_max * (N_FFT // 2)
    lines.append(dict(summary="yin", hip_ms=round(hip_ms, 4), stock_torch_ms=round(stock_ms, 4), stock_over_hip=round(stock_ms / hip_ms, 2),
                      difference_fma=fma, hip_gfma_per_s=round(fma / hip_ms / 1e6, 1), lags=[tracker.tau_min, tracker.tau_max],
                      voicing_agreement_with_stock=round(agree, 5), median_rel_f0_diff_with_stock=rel, device=torch.cuda.get_device_name(0)))

    # the pairs of tools/micro/score_timing.py
    g = torch.Generator().manual_seed(0)
    x = torch.randn(B, T, 13, generator=g).cumsum(1).to(dev)
    y = torch.randn(B, T, 13, generator=g).cumsum(1).to(dev)
    xl = torch.randint(T - T // 5, T + 1, (B,), generator=g).to(torch.int32).to(dev)
    yl = torch.randint(T - T // 5, T + 1, (B,), generator=g).to(torch.int32).to(dev)
    xl[0], yl[0] = T, T
    arms = {"dtw": lambda: dtw(x, xl, y, yl), "dtw_path": lambda: dtw_path(x, xl, y, yl)}
    for name, fn in arms.items():
        for _ in range(args.warmup):
            outs[name] = fn()
    torch.cuda.synchronize()
    same = bool(torch.equal(outs["dtw"][0], outs["dtw_path"][0]) and torch.equal(outs["dtw"][1], outs["dtw_path"][1]))
    calls = {"dtw": args.hip_calls, "dtw_path": args.hip_calls}
    times = timed(arms, calls, args.rounds)
    for name in arms:
        lines.append(dict(measurement="dtw_path", leg=name, ms_median=round(statistics.median(times[name]), 4), ms_min=round(min(times[name]), 4),
                          ms_rounds=[round(v, 4) for v in times[name]], calls=calls[name], warmup=args.warmup, pairs=B, frames=T, dim=13))
    a, b = statistics.median(times["dtw"]), statistics.median(times["dtw_path"])
    lines.append(dict(summary="dtw_path", dtw_ms=round(a, 4), dtw_path_ms=round(b, 4), path_over_plain=round(b / a, 3), record_and_backtrace_ms=round(b - a, 4),
                      cost_and_path_len_bit_equal=same, mean_path_len=round(float(outs["dtw_path"][1].float().mean()), 1),
                      workspace_mib=round(B * ((T + 1023) // 1024) * (T + 255) * 256 / 2 ** 20, 1)))

    _, plen, path = outs["dtw_path"]
    f0_a, f0_b = outs["hip"][0][:, :T].contiguous(), outs["hip"][0].flip(0)[:, :T].contiguous()
    err = F0Error(dev)
    arms = {"f0_error": lambda: err(f0_a, f0_b, path, plen)}
    for _ in range(args.warmup):
        arms["f0_error"]()
    torch.cuda.synchronize()
    times = timed(arms, {"f0_error": args.hip_calls}, args.rounds)
    lines.append(dict(measurement="f0_error", leg="hip", ms_median=round(statistics.median(times["f0_error"]), 4), ms_min=round(min(times["f0_error"]), 4),
                      ms_rounds=[round(v, 4) for v in times["f0_error"]], calls=args.hip_calls, items=B))
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        for line in lines:
            fh.write(json.dumps(line) + "\n")
            print(json.dumps(line), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
