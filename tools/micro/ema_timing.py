"""Time the parameter EMA (efficient_tts_amd/ema.py): the launch alone, and what it adds to the graphed training step; writes
profiles/ema_timing.json.

Two measurements, each with its arms interleaved inside one process after a warm-up, over `--rounds` rounds:
  launch : efts_ema_update on the shipped model's parameter count (3 words per element: p and e read, e written), `--launches` back-to-back
           launches between two device events.  Beside it, as the yardstick of what a streaming kernel of this shape reaches here,
           efts_optim_step (RAdam, clip on: 7 words per element) on buffers of the same size.  Reported: median time per launch, the
           bytes the algorithm has to move per second, and their share of the 8.0 TB/s HBM peak.  p and e together are 165 MB, which the
           256 MB last-level cache can hold from one launch to the next: a rate over the HBM peak would say that it did, not that the
           clock is wrong -- inside a training step ~190 other launches run in between.
  step   : the flagship training step (bench.py's: batch 32, T1 128, T2 800, Adam-amsgrad, WarmupLR) as GraphedStep replays, with and
           without an attached ParamEMA.  ONE model, optimizer and captured graph: the arm without is `optimizer.ema = None`, which is
           the step of the commit before the EMA existed (step() and __call__ test that attribute and do nothing else).  `--steps`
           replays per window between two device events, ending in a synchronise.
Not a gate: nothing asserts on the times.  Not measured: the eager loop, data parallel runs, other batch shapes, whether the averaged
weights synthesise better.

    python tools/micro/ema_timing.py [--rounds 5] [--launches 50] [--steps 30] [--precision bf16]
"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from efficient_tts_amd import EfficientTTSCNN, lib as L, ops as P  # noqa: E402
from efficient_tts_amd.ema import ParamEMA  # noqa: E402
from efficient_tts_amd.optim import EftsAdam, WarmupLR  # noqa: E402
from efficient_tts_amd.step_graph import GraphedStep  # noqa: E402

HBM_PEAK = 8.0e12


def window(fn, count):
    """seconds per call of `count` back-to-back calls between two device events"""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(count):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e-3 / count


def time_launch(n, dev, rounds, launches):
    lib = L.load()
    gen = torch.Generator(device=dev).manual_seed(0)
    p, e, g = (torch.randn(n, device=dev, generator=gen) for _ in range(3))
    g *= 1e-3
    m, v = torch.zeros(n, device=dev), torch.zeros(n, device=dev)
    sumsq = (g.double() ** 2).sum().float().reshape(1)
    count = [0]

    def ema():
        L.check(lib.efts_ema_update(e.data_ptr(), p.data_ptr(), n, 1e-3, P._stream()), "efts_ema_update")

    def radam():
        count[0] += 1
        a = L.OptimArgs()
        a.p, a.g, a.m, a.v, a.n, a.vmax = p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), n, None
        a.sumsq, a.max_norm, a.gscale, a.algo, a.amsgrad = sumsq.data_ptr(), 1.0, 1.0, L.OPTIM_RADAM, 0
        a.lr, a.beta1, a.beta2, a.eps, a.weight_decay, a.step = 1e-3, 0.9, 0.99, 1e-9, 1e-5, count[0]
        L.check(lib.efts_optim_step(a, P._stream()), "efts_optim_step")

    arms = [("efts_ema_update", ema, 3), ("efts_optim_step_radam", radam, 7)]
    times = {name: [] for name, _, _ in arms}
    with P.stream_scope():
        for _, fn, _ in arms:
            for _ in range(10):
                fn()
        torch.cuda.synchronize()
        for r in range(rounds):
            for name, fn, _ in (arms if r % 2 == 0 else arms[::-1]):
                times[name].append(window(fn, launches))
    assert bool(torch.isfinite(e).all()) and bool(torch.isfinite(p).all())
    out = {}
    for name, _, words in arms:
        med = statistics.median(times[name])
        out[name] = dict(words_per_element=words, bytes_design=words * 4 * n, us_median=med * 1e6, us_min=min(times[name]) * 1e6,
                         us_max=max(times[name]) * 1e6, us_rounds=[t * 1e6 for t in times[name]], bytes_per_s=words * 4 * n / med,
                         share_of_hbm_peak=words * 4 * n / med / HBM_PEAK, us_at_hbm_peak=words * 4 * n / HBM_PEAK * 1e6)
    out["ema_bytes_per_s_over_optim_step"] = out["efts_ema_update"]["bytes_per_s"] / out["efts_optim_step_radam"]["bytes_per_s"]
    return out


def time_step(dev, rounds, steps, precision):
    B, T1, T2 = 32, 128, 800
    torch.manual_seed(0)
    model = EfficientTTSCNN(num_symbols=76, dropout_rate=0.0, use_masking=True, use_weighted_masking=False, sigma=0.01, precision=precision).to(dev).train()
    opt = EftsAdam(model, lr=1e-3, betas=(0.9, 0.99), eps=1e-9, weight_decay=1e-5, amsgrad=True, grad_norm=1.0)
    ema = ParamEMA(opt, decay=0.999, warmup=True)
    graphed = GraphedStep(model, opt, WarmupLR(opt, warmup_steps=4000))
    g = torch.Generator().manual_seed(1234)
    text, mel = torch.randint(0, 76, (B, T1), generator=g).to(dev), torch.randn(B, T2, 80, generator=g).to(dev)
    tl, sl = torch.full((B,), T1, dtype=torch.int64, device=dev), torch.full((B,), T2, dtype=torch.int64, device=dev)
    for _ in range(3):
        graphed(text, tl, mel, sl)
    bufs = graphed.inputs(text, tl, mel, sl)               # the batch resident in the buffers the captured launches read, as bench.py has it
    assert bufs is not None, "the step was not captured"
    for s_, t in zip(bufs, (text, tl, mel, sl)):
        s_.copy_(t)

    def run():
        graphed(*bufs)
    arms = [("without_ema", None), ("with_ema", ema)]
    for _, attached in arms:
        opt.ema = attached
        for _ in range(5):
            run()
    torch.cuda.synchronize()
    times = {name: [] for name, _ in arms}
    for r in range(rounds):
        for name, attached in (arms if r % 2 == 0 else arms[::-1]):
            opt.ema = attached
            replays0 = graphed.replays
            times[name].append(window(run, steps))
            assert graphed.replays == replays0 + steps, "the timed steps were not graph replays"
    opt.ema = ema
    torch.cuda.synchronize()
    assert bool(torch.isfinite(ema.flat[:opt.eng.numel]).all()) and bool(torch.isfinite(opt.flat_p[:opt.eng.numel]).all())
    out = dict(batch=B, phoneme_len=T1, mel_len=T2, precision=precision, steps_per_window=steps, numel=opt.eng.numel, ema_updates=ema.updates)
    for name, _ in arms:
        out[name] = dict(ms_median=statistics.median(times[name]) * 1e3, ms_min=min(times[name]) * 1e3, ms_max=max(times[name]) * 1e3,
                         ms_rounds=[t * 1e3 for t in times[name]])
    a, b = out["without_ema"]["ms_median"], out["with_ema"]["ms_median"]
    out.update(added_ms=b - a, added_share_of_step=(b - a) / a)
    return out, opt.eng.numel


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--launches", type=int, default=50)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--precision", type=str, default="bf16", choices=["bf16", "bf16x3"])
    ap.add_argument("--out", type=str, default=os.path.join(ROOT, "profiles", "ema_timing.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise RuntimeError("no MI355X (gfx950) device visible: nothing to time")
    dev = torch.device("cuda:0")
    L.require_device()
    step, n = time_step(dev, args.rounds, args.steps, args.precision)
    launch = time_launch(n, dev, args.rounds, args.launches)
    out = dict(device=torch.cuda.get_device_name(0), rounds=args.rounds, launches_per_window=args.launches, hbm_peak_bytes_per_s=HBM_PEAK, numel=n,
               launch=launch, step=step,
               not_measured="the eager loop, data parallel runs, other batch shapes, whether the averaged weights synthesise better")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out, indent=1), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
