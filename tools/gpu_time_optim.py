#!/usr/bin/env python3
"""Times the fused optimizer kernels at the model's own flat size (GPU box):

    python tools/gpu_time_optim.py [--rounds 20] [--launches 50] [--out profiles/optim_timing.json]

Arms: efts_adam_amsgrad (the recipe's kernel, 9 words per parameter) and every efts_optim_step variant (Adam / AdamW with and without
amsgrad, RAdam: 7 words, 9 with amsgrad), each with the clip on.  The arms are interleaved inside one process -- every round times every
arm once, `launches` back-to-back launches between two device events -- so that whatever else the box is doing lands on all of them alike.
Reports the median time per launch, the bytes the algorithm has to move (words * 4 * n) per second, their share of the measured HBM
copy rate (6.29 TB/s; 8.0 TB/s peak) and the ratio to the amsgrad kernel."""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from efficient_tts_amd import EfficientTTSCNN, lib as L, ops as P  # noqa: E402
from efficient_tts_amd.train import TrainEngine  # noqa: E402

HBM_MEASURED, HBM_PEAK = 6.29e12, 8.0e12
ARMS = [("efts_adam_amsgrad", None, True), ("adam", L.OPTIM_ADAM, False), ("adam_amsgrad", L.OPTIM_ADAM, True), ("adamw", L.OPTIM_ADAMW, False),
        ("adamw_amsgrad", L.OPTIM_ADAMW, True), ("radam", L.OPTIM_RADAM, False)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--launches", type=int, default=50)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "optim_timing.json"))
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    lib = L.load()
    L.require_device()
    n = TrainEngine(EfficientTTSCNN(num_symbols=76, use_masking=True).to(dev)).numel
    gen = torch.Generator(device=dev).manual_seed(0)
    p, g = torch.randn(n, device=dev, generator=gen), torch.randn(n, device=dev, generator=gen) * 1e-3
    m, v, vmax = torch.zeros(n, device=dev), torch.zeros(n, device=dev), torch.zeros(n, device=dev)
    sumsq = (g.double() ** 2).sum().float().reshape(1)
    steps = {name: 0 for name, _, _ in ARMS}

    def launch(name, algo, ams):
        steps[name] += 1
        if algo is None:
            L.check(lib.efts_adam_amsgrad(p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), vmax.data_ptr(), n, sumsq.data_ptr(), 1.0, 1.0,
                                          1e-3, 0.9, 0.99, 1e-9, 1e-5, steps[name], P._stream()), name)
            return
        a = L.OptimArgs()
        a.p, a.g, a.m, a.v, a.n, a.vmax = p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), n, vmax.data_ptr() if ams else None
        a.sumsq, a.max_norm, a.gscale, a.algo, a.amsgrad = sumsq.data_ptr(), 1.0, 1.0, algo, int(ams)
        a.lr, a.beta1, a.beta2, a.eps, a.weight_decay, a.step = 1e-3, 0.9, 0.99, 1e-9, 1e-5, steps[name]
        L.check(lib.efts_optim_step(a, P._stream()), name)

    times = {name: [] for name, _, _ in ARMS}
    with P.stream_scope():
        for arm in ARMS:                                   # warm up: code objects loaded, clocks up
            for _ in range(10):
                launch(*arm)
        torch.cuda.synchronize()
        for r in range(args.rounds):
            order = ARMS[r % len(ARMS):] + ARMS[:r % len(ARMS)]      # (no arm always runs behind the same neighbour)
            for arm in order:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(args.launches):
                    launch(*arm)
                e1.record()
                e1.synchronize()
                times[arm[0]].append(e0.elapsed_time(e1) * 1e-3 / args.launches)
    assert bool(torch.isfinite(p).all())
    base = statistics.median(times["efts_adam_amsgrad"])
    out = dict(numel=n, rounds=args.rounds, launches_per_window=args.launches, hbm_measured_copy_bytes_per_s=HBM_MEASURED, hbm_peak_bytes_per_s=HBM_PEAK, arms={})
    for name, algo, ams in ARMS:
        words = 9 if ams else 7
        med = statistics.median(times[name])
        out["arms"][name] = dict(words_per_parameter=words, median_us=med * 1e6, min_us=min(times[name]) * 1e6, max_us=max(times[name]) * 1e6,
                                 bytes_per_s=words * 4 * n / med, share_of_measured_hbm=words * 4 * n / med / HBM_MEASURED,
                                 share_of_peak_hbm=words * 4 * n / med / HBM_PEAK, ratio_to_efts_adam_amsgrad=med / base)
        print(f"{name:18s} {med * 1e6:8.1f} us  {words * 4 * n / med / 1e12:5.2f} TB/s  x{med / base:.3f}")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
    print(args.out)


if __name__ == "__main__":
    main()
