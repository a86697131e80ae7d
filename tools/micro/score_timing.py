"""Time the on-device DTW against the same recurrence on stock PyTorch ops on the same GPU; writes profiles/score_timing.json.

Workload: 64 pairs of 13-dimensional features (Gaussian random walks), about 800 x 800 frames, ragged (lengths 640 .. 800).  Arms,
interleaved inside one process after a warm-up:
  hip   : efficient_tts_amd.score.dtw (efts_dtw: one launch, one workgroup per pair);
  stock : the local costs by torch.cdist, then one anti-diagonal of the whole batch per step -- gather the three predecessors from the
          two previous diagonals, choose by the tie rule, add -- about Tx + Ty steps of a dozen small launches each.  It keeps the
          [B, Tx, Ty] local-cost matrix in memory, which the kernel never forms.
Reported per arm: ms per call (median and min over the rounds); for the HIP arm also the time per wavefront step of the longest pair
(Ty + ceil(Tx / 4) - 1 steps of one barrier each), which is what bounds the kernel.  Not a gate: nothing asserts on the times.

    python tools/micro/score_timing.py [--pairs 64] [--frames 800] [--rounds 5] [--calls 3] [--hip_calls 200]
"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from efficient_tts_amd.score import dtw  # noqa: E402

ROWS_PER_LANE = 4                        # DTW_ROWS of csrc/efts_score.hip


def stock_dtw(x, xl, y, yl):
    """(cost, path_len) by stock ops: diagonal s holds the cells i + j = s of every pair, indexed by i"""
    B, Tx, _ = x.shape
    Ty = y.shape[1]
    dev = x.device
    d = torch.cdist(x, y)                                                      # [B, Tx, Ty]
    inf = torch.full((B, Tx + 1), float("inf"), device=dev)                    # slot i + 1 holds row i; slot 0 is the border above row 0
    zero = torch.zeros(B, Tx + 1, dtype=torch.int32, device=dev)
    prev2_a, prev2_l = inf.clone(), zero.clone()
    prev2_a[:, 0] = 0.0                                                        # the cell in front of (0, 0)
    prev_a, prev_l = inf.clone(), zero.clone()
    rows = torch.arange(Tx, device=dev)
    cost = torch.full((B,), float("nan"), device=dev)
    plen = torch.zeros(B, dtype=torch.int32, device=dev)
    last = (xl + yl - 2).to(torch.int64)
    for s in range(Tx + Ty - 1):
        cols = s - rows
        ok = (cols >= 0) & (cols < Ty)
        local = d[:, rows, cols.clamp(0, Ty - 1)]
        best, ln = prev2_a[:, :-1], prev2_l[:, :-1]                            # (i-1, j-1): diagonal s - 2, row i - 1
        up_a, up_l = prev_a[:, :-1], prev_l[:, :-1]                            # (i-1, j):   diagonal s - 1, row i - 1
        take = up_a < best
        best, ln = torch.where(take, up_a, best), torch.where(take, up_l, ln)
        take = prev_a[:, 1:] < best                                            # (i, j-1):   diagonal s - 1, row i
        best, ln = torch.where(take, prev_a[:, 1:], best), torch.where(take, prev_l[:, 1:], ln)
        cur_a, cur_l = inf.clone(), zero.clone()
        cur_a[:, 1:] = torch.where(ok, local + best, inf[:, 1:])
        cur_l[:, 1:] = ln + 1
        done = last == s
        cost = torch.where(done, cur_a.gather(1, xl.to(torch.int64)[:, None])[:, 0], cost)
        plen = torch.where(done, cur_l.gather(1, xl.to(torch.int64)[:, None])[:, 0], plen)
        prev2_a, prev2_l, prev_a, prev_l = prev_a, prev_l, cur_a, cur_l
    return cost, plen


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=64)
    ap.add_argument("--frames", type=int, default=800)
    ap.add_argument("--dim", type=int, default=13)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--calls", type=int, default=3, help="stock calls per round")
    ap.add_argument("--hip_calls", type=int, default=200, help="kernel calls per round (a window of a fraction of a second, like the stock arm's)")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", type=str, default=os.path.join(ROOT, "profiles", "score_timing.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise RuntimeError("no MI355X (gfx950) device visible: nothing to time")
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(0)
    T = args.frames
    x = torch.randn(args.pairs, T, args.dim, generator=g).cumsum(1).to(dev)
    y = torch.randn(args.pairs, T, args.dim, generator=g).cumsum(1).to(dev)
    xl = torch.randint(T - T // 5, T + 1, (args.pairs,), generator=g).to(torch.int32).to(dev)
    yl = torch.randint(T - T // 5, T + 1, (args.pairs,), generator=g).to(torch.int32).to(dev)
    xl[0], yl[0] = T, T
    # the stock arm has no notion of a padded row: the frames behind an item's end only feed cells that are never chosen from
    arms = {"hip": lambda: dtw(x, xl, y, yl), "stock": lambda: stock_dtw(x, xl, y, yl)}
    outs = {}
    for name, fn in arms.items():
        for _ in range(args.warmup):
            outs[name] = fn()
    torch.cuda.synchronize()
    rel = float(((outs["hip"][0] - outs["stock"][0]).abs() / outs["stock"][0]).max())
    same_len = int((outs["hip"][1] == outs["stock"][1]).sum())
    times = {name: [] for name in arms}
    calls = {"hip": args.hip_calls, "stock": args.calls}
    for _ in range(args.rounds):
        for name, fn in arms.items():
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            for _ in range(calls[name]):
                fn()
            t1.record()
            torch.cuda.synchronize()
            times[name].append(t0.elapsed_time(t1) / calls[name])
    lines = []
    for name in arms:
        lines.append(dict(leg=name, ms_median=round(statistics.median(times[name]), 4), ms_min=round(min(times[name]), 4),
                          ms_rounds=[round(t, 4) for t in times[name]], calls=calls[name], warmup=args.warmup, pairs=args.pairs, frames=T, dim=args.dim))
    hip_ms, stock_ms = statistics.median(times["hip"]), statistics.median(times["stock"])
    steps = T + (T + ROWS_PER_LANE - 1) // ROWS_PER_LANE - 1
    lines.append(dict(summary="dtw", hip_ms=round(hip_ms, 4), stock_torch_ms=round(stock_ms, 4), stock_over_hip=round(stock_ms / hip_ms, 2),
                      wavefront_steps_longest_pair=steps, hip_us_per_step=round(hip_ms * 1e3 / steps, 4), hip_vs_stock_max_rel_cost_diff=rel,
                      path_len_equal=f"{same_len}/{args.pairs}", device=torch.cuda.get_device_name(0)))
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        for line in lines:
            f.write(json.dumps(line) + "\n")
            print(json.dumps(line), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
