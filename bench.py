#!/usr/bin/env python3
"""bench.py -- the driver's measurement contract for the EFTS-CNN hot path.

    python bench.py --gpus N --steps K --warmup W [--dump-outputs DIR] [--full]
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N ... bench.py --gpus N ...

One "step" = one pass of the hot path over one synthetic batch.  Default workload = BASELINE.json configs[1]: the EFTS-CNN
teacher-forced forward (the reference's EfficientTTSCNN.forward under no_grad, nntts/models/efficient_tts.py:120-228) at batch 64 /
phoneme-len 128 / mel-len 800 / 80 bins per MI355X, bf16 MFMA operands with fp32 accumulate; the residual stream between the layers
of the mel-length stacks is a pair of bf16 planes (hi + lo = 16 mantissa bits).  Inputs are resident in HBM
before the timed region.

`--gpus N` with N > 1: one process per GPU.  Under a launcher (WORLD_SIZE set: torch.distributed.run) the ranks are the
launcher's and must number N; WITHOUT one this script launches the N ranks itself (re-executing under torch.distributed.run on
127.0.0.1) and fails unless N ranks come up -- it never silently measures one GPU.  The forward has no exchange step, so its
N-GPU value is N replicas (weak scaling, frames of all ranks / max-over-ranks time).  With --full the line then carries `train32`:
BASELINE configs 3 / 4, the data-parallel training step at batch 32 per GPU with the bucketed RCCL gradient all-reduce overlapped
with the backward (efficient_tts_amd/bench_train.py), with its `dp` record (backend, ranks, bytes and time per bucket, exposed wait,
RCCL's own topology lines, bit-exact replica check).  `--workload train32` times only that step.  At N > 1 the forward result is
protected from that record: an exception in it costs the record (`train32.error`), a hang is cut after EFTS_BENCH_DP_TIMEOUT
(240) seconds by a watchdog that prints the line with what there is and ends every rank.

A plain run of the forward workloads does only what its headline needs: it sets up, warms up, times exactly K steps, writes the last step's outputs with
--dump-outputs DIR (float32 .npy files, fixed seeded inputs and weights: two builds run with the same arguments can be compared output
for output) and prints the line: metric, value, unit, higher_is_better, dtype, ms_per_step (one timed step, in milliseconds).

With --full the line (N = 1, fwd64) carries every BASELINE config under the one invocation: `parity_mode` (bf16x3, the 1e-3 grade,
same K / W), `long16` (config 5: B=16 x (128, 1200), both precisions), `infer64` (config 2-ii: batched free-running inference), `infer_lj` (config 1: ten
LJSpeech utterances one by one, + end-to-end with the vocoder), `train32` (config 3, + its parity mode), each with ms_per_step, roofline, the oracle as
checker (hip_vs_oracle_mel_max_abs) and a bounded CPU leg; and `stock_gpu_baseline`: the oracle's plain torch ops on THIS GPU (MIOpen / hipBLASLt, fp32 and
bf16 autocast; forward B=64 and training step B=32) -- a second baseline leg beside `cpu_baseline`, never the product.

Prints ONE JSON line on rank 0; with --full it holds `roofline` for the dominant kernel (the k5 Conv1d contraction at mel length, measured with HIP
events on the launch stream over eager steps after the timed region; `traffic` from two rocprofv3 PMC child passes) and `cpu_baseline` (the
oracle's CPU restatement timed on this box's host cores on a bounded sample).
"""
import argparse
import glob
import json
import os
import shutil
import sqlite3
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

PEAK_MFMA_BF16_TFLOPS = 2500.0        # dense bf16 MFMA peak, MI355X_MICROARCH.md "Chip-level parameters"
PEAK_HBM_GBS = 8000.0
FWD_FLOP_PER_ITEM = 21.43e9           # SURVEY.md 8d, (T1, T2) = (128, 800)


def parse(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    # defaults: long enough for the clock governor to settle (the chip runs this workload at its 1 400 W cap and ramps for tens of
    # milliseconds: 5 + 20 steps measure 1-2 % slower than the sustained rate, profiles/bench_ramp_r04.txt); ~0.3 s of timed work
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=30)
    ap.add_argument("--precision", default="bf16", choices=["bf16", "bf16x3"])
    ap.add_argument("--workload", default="fwd64", choices=["fwd64", "fwd16_long", "train32", "infer_lj", "infer64", "logmel64", "vocoder", "vocoder8", "stock_gpu", "rendezvous"])
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--train-set", action="append", default=[], metavar="NAME=INT",
                    help="train32 A/B runs: set a hook of efficient_tts_amd.train (_RESCONV_DGRAD=3, _SIGN_MIN_ROWS=0, ...)")
    ap.add_argument("--dp-algo", default="allreduce", choices=["allreduce", "rs_ag"], help="train32, N > 1: per-bucket all_reduce, or reduce_scatter + all_gather (point-to-point xGMI)")
    ap.add_argument("--side-stream", type=int, default=1, help="0: text-length work on the main stream (A/B)")
    ap.add_argument("--resconv", type=int, default=1, help="0: residual stacks on efts_gemm + fp32 stream (A/B)")
    ap.add_argument("--fuse-prenet", type=int, default=1, help="A/B: 0 = efts_pack_rows + efts_gemm instead of efts_frame_linear")
    ap.add_argument("--fuse-soft-index", type=int, default=1, help="A/B: 0 = scores stored + efts_attn_soft_index instead of the softmax epilogue of the q.k^T launch")
    ap.add_argument("--resconv-min-rows", type=int, default=-1, help="A/B: row-space size from which the stacks run on efts_resconv5")
    ap.add_argument("--graph", type=int, default=0, help="forward workloads. 0 (default): the timed step is a plain model(...) call, as a drop-in caller issues it (the model replays a per-shape hipGraph internally); 1: a bench-level hipGraph of the eager launches")
    ap.add_argument("--model-graphs", type=int, default=1, help="0 with --graph 0: the model's internal graph cache off = every kernel launched eagerly")
    ap.add_argument("--full", action="store_true", help="everything beside the headline as well: the CPU and stock-GPU baselines, the parity-grade mode, call modes, "
                    "the other BASELINE configs, the training record, roofline and PMC traffic (each switch below defaults to 1 with --full, 0 without; "
                    "an explicit value wins). Without it the run sets up, warms up, times --steps steps and prints the line")
    ap.add_argument("--dump-outputs", default="", metavar="DIR", help="forward workloads: after the timed steps, write what the last timed step returned "
                    "(loss, mel_loss, duration_loss, imv, reconst_alpha, mel_pred) as DIR/<name>.npy, float32, at most 64 MB in all")
    ap.add_argument("--parity-mode", type=int, default=None, help="forward workloads in bf16: also time the bf16x3 parity-grade mode (same K / W) -> `parity_mode` in the JSON line")
    ap.add_argument("--train-graph", type=int, default=1, help="train32, one process: the step as one hipGraph replay (0: eager launches)")
    ap.add_argument("--call-modes", type=int, default=None, help="forward workloads, N=1: 10 extra steps per call mode (plain call / bench graph / eager) -> `call_modes`")
    ap.add_argument("--train-record", type=int, default=None, help="fwd64: also time BASELINE config 3 (training step B=32, 40 steps) under the same invocation -> `train32` in the JSON line")
    ap.add_argument("--sub-records", type=int, default=None, help="fwd64, N=1: also time BASELINE configs 5, 2-ii and 1 under the same invocation -> `long16`, `infer64`, `infer_lj` in the JSON line")
    ap.add_argument("--stock-gpu", type=int, default=None, help="fwd64, N=1: also time the oracle's plain torch ops on this GPU (MIOpen / hipBLASLt, fp32 and bf16 autocast) -> `stock_gpu_baseline`")
    ap.add_argument("--stock-find", type=int, default=0, help="stock_gpu_baseline: 1 = torch.backends.cudnn.benchmark = True (MIOpen's exhaustive solver search, as nntts/bin/train.py:60 sets it; tens of seconds per new shape)")
    ap.add_argument("--measure-traffic", type=int, default=None, help="forward workloads, N=1, with --full: roofline.traffic from two rocprofv3 PMC passes (FETCH_SIZE, WRITE_SIZE) over a 2-step child run, when rocprofv3 is installed; 0: the committed profiles/traffic.json")
    ap.add_argument("--test-shape", default="", metavar="B,T1,T2", help="PLUMBING TESTS ONLY (tests/test_dist_gpu.py: eight ranks sharing one GPU over gloo): fwd64 / train32 at this shape "
                    "instead of BASELINE's, the training record at --steps / --warmup; the line says so in config.workload")
    ap.add_argument("--rc-kernel", type=int, default=0, help="A/B: efts_resconv5_args.kernel of every launch: 0 the 8-wave ping-pong kernel (default), 2 the one-wave-per-SIMD kernel where it applies")
    a = ap.parse_args(argv)
    for k in ("parity_mode", "call_modes", "train_record", "sub_records", "stock_gpu", "measure_traffic"):
        if getattr(a, k) is None:
            setattr(a, k, int(a.full))
    a.no_cpu_baseline = a.no_cpu_baseline or not a.full
    return a


WORKLOADS = {
    "fwd64": dict(B=64, T1=128, T2=800, desc="EFTS-CNN forward (teacher-forced, no_grad) B=64 phon=128 mel=800 80-bin"),
    "fwd16_long": dict(B=16, T1=128, T2=1200, desc="EFTS-CNN forward B=16 phon=128 mel=1200 (long-sequence stress)"),
    "train32": dict(B=32, T1=128, T2=800, desc="EFTS-CNN training step fwd+bwd+clip+Adam B=32/GPU"),
}


def synth(B, T1, T2, seed, dev):
    g = torch.Generator().manual_seed(seed)
    text = torch.randint(0, 76, (B, T1), generator=g).to(dev)
    mel = torch.randn(B, T2, 80, generator=g).to(dev)
    tl = torch.full((B,), T1, dtype=torch.int64, device=dev)
    sl = torch.full((B,), T2, dtype=torch.int64, device=dev)
    return text, tl, mel, sl


DUMP_BUDGET_BYTES = 64 * 10 ** 6


def dump_outputs(path, arrays, budget=DUMP_BUDGET_BYTES):
    """--dump-outputs: write each tensor of `arrays` (name -> tensor) as path/<name>.npy in float32.  When the whole exceeds `budget`, every
    array is cut to its share of it by a fixed sample (seed 0, sorted flat indices, the same for the same shape): two builds run with the same
    arguments write the same elements."""
    import numpy as np
    os.makedirs(path, exist_ok=True)
    host = {k: v.detach().float().cpu().numpy() for k, v in arrays.items()}
    total = sum(v.nbytes for v in host.values())
    for name, v in host.items():
        if total > budget and v.size > 1:
            keep = max(1, int(v.size * budget // total))
            v = v.reshape(-1)[np.unique(np.random.default_rng(0).integers(0, v.size, keep))]
        np.save(os.path.join(path, name + ".npy"), np.asarray(v, dtype=np.float32))


def forward_outputs(out):
    """what a caller of model(text, tl, mel, sl) receives, by name (the last element, the input mel handed back, is left out)"""
    loss, stats, imv, ralpha, mel_pred, _ = out
    return dict(loss=loss, mel_loss=torch.as_tensor(stats["mel_loss"]), duration_loss=torch.as_tensor(stats["duration_loss"]), imv=imv,
                reconst_alpha=ralpha, mel_pred=mel_pred)


def cpu_baseline(T1, T2, hip_check=None, Bc=64, threads=None, passes=3):
    """the oracle (CPU port of the reference path) timed on this box's host cores in the same
    invocation: forward under no_grad, fp32, B=64 x (T1, T2), median of 3 after 1 warm-up, torch.set_num_threads(os.cpu_count()).
    torch's CPU convolution (oneDNN) does not always scale to every hardware thread of a 2-socket host, so 16 and 32 threads
    are timed as well and the FASTEST is reported (`cores` = the threads it used; every measurement is in `by_threads`): the
    scan can only flatter the CPU.  hip_check(P, text, tl, mel, sl) -> mel_pred of the HIP model with the oracle's parameters on
    the first 2 items; the oracle then acts as the checker and the measured max-abs difference is reported too."""
    from oracle import efts_oracle as O          # the cpu_baseline leg: oracle as the thing timed
    cores = os.cpu_count() or 1
    P = O.fill_params()
    g = torch.Generator().manual_seed(1234)
    text = torch.randint(0, 76, (Bc, T1), generator=g)
    mel = torch.randn(Bc, T2, 80, generator=g)
    tl = torch.full((Bc,), T1, dtype=torch.int64)
    sl = torch.full((Bc,), T2, dtype=torch.int64)
    best, by = None, {}
    # 16 and 32 threads on the full batch; every hardware thread (what BASELINE.md section 3 names) on the full batch too unless the
    # host is so wide that oneDNN collapses there (256 threads: ~25 s per forward), in which case that point is taken on B=16
    # (sub-records of the default line pass `threads` = the fwd64 leg's fastest choice and passes = 1: one bounded pass each)
    for nt in (sorted({min(cores, 16), min(cores, 32), cores}) if threads is None else threads):
        bn = Bc if nt <= 64 else min(Bc, 16)
        torch.set_num_threads(nt)
        times = []
        with torch.no_grad():
            t0 = time.perf_counter()
            O.forward(P, text[:bn], tl[:bn], mel[:bn], sl[:bn])
            warm = time.perf_counter() - t0
            for _ in range(passes if warm < 4.0 else 1):
                t0 = time.perf_counter()
                O.forward(P, text[:bn], tl[:bn], mel[:bn], sl[:bn])
                times.append(time.perf_counter() - t0)
        med = sorted(times)[len(times) // 2]
        by[f"{nt} threads, B={bn}"] = bn * T2 / med
        if best is None or bn * T2 / med > best[2]:
            best = (med, nt, bn * T2 / med, bn)
    med, nt, _, bn = best
    res = dict(value=bn * T2 / med, unit="mel-frames/s", cores=nt, host_cpus=cores, kind="port", by_threads=by,
               sample=(f"oracle forward fp32, (T1={T1}, T2={T2}), 1 warm-up then the median of 3 (1 if a pass takes > 4 s) at 16 / 32 / all {cores} host "
                       f"threads; B={Bc} (BASELINE.md section 3: the full config-2 batch; B=16 at more than 64 threads); fastest = {nt} threads, B={bn} "
                       f"({med:.3f} s/iter)") if threads is None else
                      f"oracle forward fp32, B={bn} x (T1={T1}, T2={T2}), 1 warm-up then {len(times)} timed pass(es) at {nt} threads (the fwd64 leg's fastest choice) ({med:.3f} s/iter)")
    if hip_check is not None:
        with torch.no_grad():
            ref = O.forward(P, text[:2], tl[:2], mel[:2], sl[:2])
        got = hip_check(P, text[:2], tl[:2], mel[:2], sl[:2])
        res["hip_vs_oracle_mel_max_abs"] = float((got.detach().cpu() - ref["mel_pred"]).abs().max())
        res["hip_vs_oracle_note"] = "same parameters and inputs (2 items, full length); north_star tolerance 1e-3 applies to the bf16x3 mode"
        res["_ref_mel"] = ref["mel_pred"]
    return res


def cpu_train_baseline(T1, T2):
    """the oracle (CPU restatement of the reference path, torch autograd for the backward)
    timed on this box's host cores for one training step -- fwd + bwd + clip 1.0 + Adam-amsgrad -- at the config's own batch,
    B = 32 full-length items: 1 warm-up step, then the median of 3 (one timed step if a step takes more than 8 s, so that the
    default bench run stays bounded)."""
    from oracle import efts_oracle as O          # the cpu_baseline leg: oracle as the thing timed
    cores = os.cpu_count() or 1
    nt = min(cores, 32)
    torch.set_num_threads(nt)
    P = {k: v.clone().requires_grad_(v.is_floating_point()) for k, v in O.fill_params().items()}
    params = [v for v in P.values() if v.requires_grad]
    opt = torch.optim.Adam(params, lr=1e-3, betas=(0.9, 0.99), eps=1e-9, weight_decay=1e-5, amsgrad=True)
    Bc = 32
    g = torch.Generator().manual_seed(1234)
    text = torch.randint(0, 76, (Bc, T1), generator=g)
    mel = torch.randn(Bc, T2, 80, generator=g)
    tl = torch.full((Bc,), T1, dtype=torch.int64)
    sl = torch.full((Bc,), T2, dtype=torch.int64)

    def one():
        t0 = time.perf_counter()
        out = O.forward(P, text, tl, mel, sl)
        opt.zero_grad()
        out["loss"].backward()
        torch.nn.utils.clip_grad_norm_(params, 1.0)
        opt.step()
        return time.perf_counter() - t0
    warm = one()
    times = [one() for _ in range(3 if warm <= 8.0 else 1)]
    med = sorted(times)[len(times) // 2]
    return dict(value=Bc * T2 / med, unit="mel-frames/s", cores=nt, host_cpus=cores, kind="port",
                sample=f"oracle training step fp32 (forward, autograd backward, clip 1.0, torch Adam-amsgrad), B={Bc} x (T1={T1}, T2={T2}) = BASELINE.md "
                       f"section 3's config-3 batch, median of {len(times)} after 1 warm-up ({med:.3f} s/step at {nt} threads)")


def stock_gpu_baseline(dev, find=False, budget_s=45.0, T1=128, T2=800):
    """A second baseline leg beside `cpu_baseline`: the oracle's plain torch ops moved to THIS GPU -- what a user of the
    reference gets on this box without this library: MIOpen convolutions, hipBLASLt / rocBLAS matmuls, the [B, T1, T2] temporaries of the
    unfused alignment block, torch autograd, clip_grad_norm_ and torch.optim.Adam(amsgrad).  fp32 as the reference is written, and under
    torch.autocast(bfloat16).  Config 2 (forward, no_grad, B = 64) and config 3 (training step, B = 32), full lengths, 2 warm-up + 5 timed passes
    each, synchronize on both sides.  A baseline, never the product: efficient_tts_amd/ does not import it.  MIOpen's solver search
    (`torch.backends.cudnn.benchmark`, which nntts/bin/train.py:60 switches on) costs tens of seconds per new convolution shape, so the default
    line runs MIOpen's immediate mode and says so; `python bench.py --workload stock_gpu --stock-find 1` is the searched figure
    (profiles/bench_stock_gpu_r06.json).  Legs that do not fit `budget_s` are skipped and named."""
    from oracle import efts_oracle as O          # a baseline leg: the oracle as the thing timed
    t_start = time.perf_counter()
    keep_bench = torch.backends.cudnn.benchmark
    torch.backends.cudnn.benchmark = bool(find)
    out = dict(kind="port on stock torch-ROCm ops (the oracle's torch calls on the GPU: MIOpen Conv1d, hipBLASLt / rocBLAS matmul, torch autograd + "
                    "clip_grad_norm_ + torch.optim.Adam(amsgrad))", unit="mel-frames/s",
               miopen="solver search (torch.backends.cudnn.benchmark = True, as nntts/bin/train.py:60)" if find else
                      "immediate mode (torch.backends.cudnn.benchmark = False; the searched figure: profiles/bench_stock_gpu_r06.json)",
               torch=torch.__version__, skipped=[])
    g = torch.Generator().manual_seed(1234)
    text64 = torch.randint(0, 76, (64, T1), generator=g).to(dev)
    mel64 = torch.randn(64, T2, 80, generator=g).to(dev)

    def lens(B):
        return torch.full((B,), T1, dtype=torch.int64, device=dev), torch.full((B,), T2, dtype=torch.int64, device=dev)

    def timed(fn, n=5, warm=2):
        for _ in range(warm):
            fn()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(n):
            fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / n

    try:
        P = {k: v.to(dev) for k, v in O.fill_params().items()}     # (filled on the host: the fill's generators are CPU generators)
        with torch.device(dev):                  # the oracle's torch.arange / zeros land on the GPU
            tl, sl = lens(64)
            for name, ac in (("fwd64_fp32", False), ("fwd64_bf16_autocast", True)):
                if time.perf_counter() - t_start > budget_s:
                    out["skipped"].append(name)
                    continue

                def fwd():
                    with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16, enabled=ac):
                        return O.forward(P, text64, tl, mel64, sl)
                dt = timed(fwd)
                out[name] = dict(value=64 * T2 / dt, ms_per_step=dt * 1e3)
            Pt = {k: v.clone().requires_grad_(v.is_floating_point()) for k, v in P.items()}
            params = [v for v in Pt.values() if v.requires_grad]
            tl, sl = lens(32)
            for name, ac in (("train32_fp32", False), ("train32_bf16_autocast", True)):
                if time.perf_counter() - t_start > budget_s:
                    out["skipped"].append(name)
                    continue
                opt = torch.optim.Adam(params, lr=1e-3, betas=(0.9, 0.99), eps=1e-9, weight_decay=1e-5, amsgrad=True)

                def step():
                    with torch.autocast("cuda", dtype=torch.bfloat16, enabled=ac):
                        loss = O.forward(Pt, text64[:32], tl, mel64[:32], sl)["loss"]
                    opt.zero_grad()
                    loss.backward()
                    torch.nn.utils.clip_grad_norm_(params, 1.0)
                    opt.step()
                dt = timed(step)
                out[name] = dict(value=32 * T2 / dt, ms_per_step=dt * 1e3)
                del opt
    except Exception as exc:                                           # noqa: BLE001 -- a baseline leg must not cost the line
        out["error"] = f"{type(exc).__name__}: {exc}"[:300]
    finally:
        torch.backends.cudnn.benchmark = keep_bench
    out["wall_s"] = time.perf_counter() - t_start
    out["sample"] = (f"oracle forward (no_grad) B=64 and training step B=32 at (T1={T1}, T2={T2}), full lengths, fp32 and torch.autocast(bfloat16): 2 warm-up + 5 timed "
                     f"passes each; legs past {budget_s:.0f} s of wall time skipped: {out['skipped'] or 'none'}")
    torch.cuda.empty_cache()
    return out


_SUSTAINED = {}


def sustained_mfma_tflops():
    """what THIS box gives a bare register-to-register bf16 MFMA stream on random operands with every CU issuing (tools/micro/mfma_ceiling.hip,
    built with hipcc on the spot): the part runs such a stream at its power cap, 1.68-1.70 GHz instead of 2.4 (DESIGN.md 4a'), so this -- not the
    nominal 2.5 PF -- is the ceiling a kernel on real data can approach.  (value, source); falls back to the committed round-5 figure."""
    if "v" in _SUSTAINED:
        return _SUSTAINED["v"]
    val, src = 1757.6, "profiles/mfma_ceiling_r05.txt (not measured in this run: no hipcc / the micro benchmark failed)"
    try:
        cc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
        tmp = tempfile.mkdtemp(prefix="efts_ceil_", dir="/tmp")
        try:
            exe = os.path.join(tmp, "mfma_ceiling")
            subprocess.run([cc, "--offload-arch=gfx950", "-O3", os.path.join(ROOT, "tools", "micro", "mfma_ceiling.hip"), "-o", exe],
                           check=True, timeout=120, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
            # the child runs on THIS rank's GPU (it would otherwise open device 0 from every rank); only rank 0 at N = 1 calls this at all
            env = dict(os.environ, HIP_VISIBLE_DEVICES=os.environ.get("LOCAL_RANK", "0")) if "HIP_VISIBLE_DEVICES" not in os.environ else None
            out = subprocess.run([exe, "quick"], check=True, timeout=60, capture_output=True, text=True, env=env).stdout
        finally:
            shutil.rmtree(tmp, ignore_errors=True)
        import re
        m = re.search(r"random operands: [0-9.]+ ms\s+([0-9.]+) TFLOP/s", out)
        if m:
            val, src = float(m.group(1)), "measured in this run: tools/micro/mfma_ceiling.hip, 512 workgroups, random bf16 operands, 5 launches of 40 000 x 16 MFMAs"
    except Exception:                                    # noqa: BLE001 -- the fallback figure is stated as such
        pass
    _SUSTAINED["v"] = (val, src)
    return _SUSTAINED["v"]


def measure_traffic(a, precision, workload=None):
    """HBM-side bytes per launch of the dominant kernel from the PMC counters, collected as MI355X_MICROARCH.md prescribes:
    FETCH_SIZE and WRITE_SIZE in SEPARATE rocprofv3 passes (--kernel-trace --pmc only), each over a 2-step child run of this very
    workload; FETCH_SIZE doubled (gfx950 tallies the 128-byte requests of wide streaming reads at 64 B), both in KiB.
    Returns (bytes per launch, description) or None when rocprofv3 is missing / a pass fails (the caller then falls back to
    the committed profiles/traffic.json)."""
    exe = shutil.which("rocprofv3") or ("/opt/rocm/bin/rocprofv3" if os.path.exists("/opt/rocm/bin/rocprofv3") else None)
    if exe is None or os.environ.get("EFTS_BENCH_CHILD") or any(k.startswith(("ROCPROF", "ROCP_TOOL")) for k in os.environ):
        return None                                      # no profiler, or this run is itself a profiled one
    tmp = tempfile.mkdtemp(prefix="efts_pmc_", dir="/tmp")
    env = dict(os.environ, TMPDIR="/tmp", EFTS_BENCH_CHILD="1")
    vals, n_disp = {}, {}
    try:
        for ctr in ("FETCH_SIZE", "WRITE_SIZE"):
            out = os.path.join(tmp, ctr)
            cmd = [exe, "--kernel-trace", "--pmc", ctr, "-d", out, "-o", "b", "--", sys.executable, os.path.abspath(__file__),
                   "--steps", "2", "--warmup", "1", "--full", "--no-cpu-baseline", "--parity-mode", "0", "--call-modes", "0", "--train-record", "0",
                   "--measure-traffic", "0", "--train-graph", "0", "--rc-kernel", str(a.rc_kernel), "--precision", precision, "--workload", workload or a.workload]
            subprocess.run(cmd, cwd="/tmp", env=env, timeout=150, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL, check=True)
            dbs = glob.glob(os.path.join(out, "**", "*.db"), recursive=True)
            if not dbs:
                return None
            con = sqlite3.connect(dbs[0])
            # the mel-length launches WITHOUT a text-encoder rider are the most frequent grid of the kernel (6 of 9 per forward; the
            # training step: 9 forward + 6 decoder dgrad launches of one grid)
            rows = con.execute("select grid_size, avg(value), count(*) from counters_collection where kernel_name like '%resconv5_kernel%' "
                               "and counter_name = ? group by grid_size order by 3 desc", (ctr,)).fetchall()
            con.close()
            if not rows:
                return None
            vals[ctr], n_disp[ctr] = float(rows[0][1]), int(rows[0][2])
        traffic = (2.0 * vals["FETCH_SIZE"] + vals["WRITE_SIZE"]) * 1024.0
        return traffic, (f"measured in this run: rocprofv3 --kernel-trace --pmc FETCH_SIZE / --pmc WRITE_SIZE (separate passes over a 2-step child run, "
                         f"{n_disp['FETCH_SIZE']} / {n_disp['WRITE_SIZE']} launches averaged): 2 * FETCH_SIZE + WRITE_SIZE, KiB counters "
                         f"(FETCH_SIZE {vals['FETCH_SIZE']:.0f}, WRITE_SIZE {vals['WRITE_SIZE']:.0f}); FETCH_SIZE doubled per MI355X_MICROARCH.md (HBM), "
                         "WRITE_SIZE uncalibrated, Infinity-Cache hits counted")
    except Exception:                                    # noqa: BLE001 -- profiler missing / timed out / format changed: fall back
        return None
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


def run_infer64(a, world, rank, dev, sub=None):
    """BASELINE config 2, variant (ii) of SURVEY.md: batched FREE-RUNNING inference at B=64 (inference_batch),
    128 phonemes per item, durations forced to 800/128 = 6.25 frames per phoneme after the duration predictor
    has run (so every item yields T2 = 800 and the predictor is still executed and timed)."""
    from efficient_tts_amd import EfficientTTSCNN
    import torch.distributed as dist
    B, T1, T2 = 64, 128, 800
    torch.manual_seed(0)
    model = EfficientTTSCNN(num_symbols=76, dropout_rate=0.0, use_masking=True, sigma=0.01, precision=a.precision).to(dev).eval()
    model.remove_weight_norm()
    g = torch.Generator().manual_seed(1234 + rank)
    text = torch.randint(0, 76, (B, T1), generator=g).to(dev)
    tl = torch.full((B,), T1, dtype=torch.int64, device=dev)
    for _ in range(max(a.warmup, 1)):
        mel, ml, _ = model.inference_batch(text, tl, force_delta=T2 / T1)
    assert int(ml.min()) == T2 and int(ml.max()) == T2 and mel.shape == (B, T2, 80)
    torch.cuda.synchronize()
    if world > 1:
        dist.barrier()
    t0 = time.perf_counter()
    for _ in range(a.steps):
        model.inference_batch(text, tl, force_delta=T2 / T1)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    if world > 1:
        t = torch.tensor([dt], dtype=torch.float64, device=dev)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        dt = float(t.item())
    dt /= a.steps
    # roofline of the dominant kernel: the decoder's six efts_resconv5 launches at 64 x 802 rows, HIP events on the launch stream around
    # each of them over three more calls
    from efficient_tts_amd import ops as Pops
    rows = Pops.Rows(B, T2).rows
    keep_graphs, model.graphs = model.graphs, False      # (the timed calls replay graphs: the launches are issued eagerly here so that they can be bracketed)
    model.inference_batch(text, tl, force_delta=T2 / T1)
    torch.cuda.synchronize()
    Pops.PROFILE, Pops.PROFILE_TAG = [], None
    for _ in range(3):
        model.inference_batch(text, tl, force_delta=T2 / T1)
    torch.cuda.synchronize()
    durs = [s.elapsed_time(e) * 1e-3 for (tag, s, e) in Pops.PROFILE if tag[0] == 5 and tag[2] == 512 and tag[1] >= B * T2]
    Pops.PROFILE, Pops.PROFILE_TAG = None, None
    model.graphs = keep_graphs
    roof, cpu = None, None
    if durs:
        avg = sum(durs) / len(durs)
        flop = 2.0 * B * T2 * 512 * 512 * 5
        alg_bytes = rows * 512 * 8 + 5 * 512 * 512 * (2 if model.split == 1 else 4)
        roof = dict(bound="mfma", kernel=f"resconv5_kernel<split={model.split}>: the decoder's k5 Conv1d 512->512 launches of the free-running pass, {B}x{T2} frames",
                    achieved=flop / avg / 1e12, peak=PEAK_MFMA_BF16_TFLOPS, unit="TFLOP/s", frac=flop / avg / 1e12 / PEAK_MFMA_BF16_TFLOPS, traffic=None,
                    traffic_note="the forward's measurement applies (same kernel, same launch shape): the fwd64 line's roofline.traffic",
                    avg_launch_us=avg * 1e6, launches_measured=len(durs), algorithmic_flop_per_launch=flop, algorithmic_bytes_per_launch=alg_bytes)
    check = None
    if rank == 0 and world == 1 and not a.no_cpu_baseline:
        # the oracle's free-running pass on this box's host cores: a bounded sample (32 items one by one, 8 as a sub-record of the default
        # line -- the reference's inference() is B = 1 by construction, efficient_tts.py:230-285 -- with the same forced durations)
        from oracle import efts_oracle as O          # the cpu_baseline leg: oracle as the thing timed, then as the checker
        Pm = {k: v.detach().cpu().float() for k, v in model.state_dict().items()}
        torch.set_num_threads(sub["threads"] if sub else min(os.cpu_count() or 1, 16))
        fd = torch.full((1, T1), T2 / T1)
        tc = text.cpu()
        nc = 8 if sub else 32
        with torch.no_grad():
            ref0 = O.inference(Pm, tc[:1], forced_delta=fd)["mel_pred"]
            t0 = time.perf_counter()
            for i in range(nc):
                O.inference(Pm, tc[i:i + 1], forced_delta=fd)
            dc = time.perf_counter() - t0
            ref1 = O.inference(Pm, tc[1:2], forced_delta=fd)["mel_pred"]
        cpu = dict(value=nc * T2 / dc, unit="mel-frames/s", cores=torch.get_num_threads(), kind="port",
                   sample=f"oracle inference() fp32, {nc} of the 64 items one by one (B = 1 is the reference's free-running form), durations forced to {T2 / T1} "
                          f"frames per phoneme, after 1 warm-up call ({dc:.2f} s)")
        got = model.inference_batch(text, tl, force_delta=T2 / T1)[0][:2].detach().cpu()
        check = float(max((got[0] - ref0[0]).abs().max(), (got[1] - ref1[0]).abs().max()))
    if rank == 0:
        res = dict(metric="mel-frames/sec (EFTS-CNN batched free-running inference, batch 64/GPU, 80-mel)", value=world * B * T2 / dt,
                   unit="mel-frames/s", n_gpus=world, steps=a.steps, warmup=a.warmup, ms_per_step=dt * 1e3, higher_is_better=True,
                   scaling="weak", vs_baseline=None, dtype=a.precision if a.precision == "bf16" else "bf16x3 (split-bf16 MFMA, fp32-class)",
                   data="synthetic", config={"workload": "EFTS-CNN inference_batch B=64 phon=128, durations forced to 6.25 -> mel=800 (eager, one host sync per call)",
                                              "batch_per_gpu": B, "phoneme_len": T1, "mel_len": T2, "precision": a.precision,
                                              "parallelism": f"replicas x{world}"},
                   rtf=dt / (world * B * T2 * 256 / 22050.0), roofline=roof, cpu_baseline=cpu)
        if check is not None:
            res["hip_vs_oracle_mel_max_abs"] = check
            res["hip_vs_oracle_note"] = f"items 0 and 1 of the batch against the oracle's B = 1 inference() with the same weights and forced durations; precision {a.precision} (1e-3 applies to bf16x3)"
        if a.precision == "bf16" and a.parity_mode and world == 1:
            # the parity-grade mode under the same clock: bf16x3, same weights, same K / W
            mp = EfficientTTSCNN(num_symbols=76, dropout_rate=0.0, use_masking=True, sigma=0.01, precision="bf16x3")
            mp = mp.to(dev).eval()
            mp.remove_weight_norm()
            mp.load_state_dict({k: v.detach() for k, v in model.state_dict().items()})
            for _ in range(max(a.warmup, 1)):
                mp.inference_batch(text, tl, force_delta=T2 / T1)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(a.steps):
                mp.inference_batch(text, tl, force_delta=T2 / T1)
            torch.cuda.synchronize()
            dtp = (time.perf_counter() - t0) / a.steps
            res["parity_mode"] = dict(precision="bf16x3", ms_per_step=dtp * 1e3, value=B * T2 / dtp, tolerance=1e-3)
            if check is not None:
                gotp = mp.inference_batch(text, tl, force_delta=T2 / T1)[0][:2].detach().cpu()
                res["parity_mode"]["hip_vs_oracle_mel_max_abs"] = float(max((gotp[0] - ref0[0]).abs().max(), (gotp[1] - ref1[0]).abs().max()))
            del mp
        if sub is not None:
            return res
        print(json.dumps(res), flush=True)


def run_logmel64(a, world, rank, dev):
    """Row f-3: the on-device log-mel front-end on 64 utterances of 800 frames (204 800 samples each):
    frame_pack -> DFT as an MFMA product (bf16x3) -> magnitude / mel / log.  Inputs resident in HBM."""
    from efficient_tts_amd import ops as P
    from efficient_tts_amd.frontend import LogMelFrontend
    import torch.distributed as dist
    B, T2 = 64, 800
    g = torch.Generator().manual_seed(1234 + rank)
    audio = (torch.rand(B, T2 * 256, generator=g) * 2 - 1).mul_(0.3).to(dev)
    lengths = torch.full((B,), T2 * 256)
    fe = LogMelFrontend(dev, radix=int(os.environ.get("EFTS_LOGMEL_RADIX", "0")))       # (EFTS_LOGMEL_RADIX: A/B: 0 = the fused FFT launch (default), 1 = the dense MFMA product, 2 / 4 / 8 = the split product)
    for _ in range(max(a.warmup, 1)):
        mel, frames = fe(audio, lengths)
    torch.cuda.synchronize()
    if world > 1:
        dist.barrier()
    t0 = time.perf_counter()
    for _ in range(a.steps):
        fe(audio, lengths)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    if world > 1:
        t = torch.tensor([dt], dtype=torch.float64, device=dev)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        dt = float(t.item())
    dt /= a.steps
    # roofline (round 6): the three launches of a call are timed with HIP events on the launch stream (frame pack / the batched DFT product / logmel);
    # the pipeline's algorithmic bytes -- audio in, operand plane written and read, spectrum written and read, mel out -- against HBM, the product's
    # FLOPs against the MFMA peak; `roofline` is the product's line (still the longest launch), `pipeline` the whole call's
    if fe.radix == 0:
        # ONE launch (efts_logmel_fft): HIP events around it on the launch stream; algorithmic bytes = audio in + log-mels out (the step is HBM-bound)
        evs = []
        for _ in range(20):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(); fe(audio, lengths); e1.record()           # (the library launches on torch's current stream: efficient_tts_amd/ops.py `_stream`)
            evs.append((e0, e1))
        torch.cuda.synchronize()
        call = sorted(e0.elapsed_time(e1) for e0, e1 in evs)[len(evs) // 2] * 1e-3
        nbytes = B * T2 * 256 * 4 + B * T2 * 80 * 4
        fft_flop = B * T2 / 2 * (5.0 * 1024 * 10)                  # one complex 1024-point FFT per frame pair, 5 N log2 N
        roof = dict(bound="hbm", kernel="logmel_fft_kernel (audio -> log-mel in one launch: reflect pad, hann window, fp32 FFT in registers / LDS, two real frames per complex "
                                        "1024-point FFT, magnitude, mel filterbank, log)",
                    achieved=nbytes / call / 1e9, peak=PEAK_HBM_GBS, unit="GB/s", frac=nbytes / call / 1e9 / PEAK_HBM_GBS, traffic=None,
                    avg_launch_us=call * 1e6, launches_measured=len(evs), algorithmic_bytes_per_launch=nbytes,
                    valu_fft_gflop=fft_flop / 1e9, valu_tflops=fft_flop / call / 1e12,
                    note="events around the whole call (one kernel + the output allocation); the MFMA pipeline it replaces (EFTS_LOGMEL_RADIX=4) moves 910 MB per call")
    rows = B * (T2 + 2)
    P.PROFILE, P.PROFILE_TAG = [], None
    evs = []
    for _ in range(3):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fe(audio, lengths)
        e1.record()
        evs.append((e0, e1))
    torch.cuda.synchronize()
    durs = [s.elapsed_time(e) * 1e-3 for (tag, s, e) in P.PROFILE if tag[0] == 1 and tag[1] == rows]
    call = sum(e0.elapsed_time(e1) for e0, e1 in evs) / len(evs) * 1e-3
    P.PROFILE, P.PROFILE_TAG = None, None
    avg = sum(durs) / max(len(durs), 1)
    if fe.radix:
      flop = 2.0 * B * T2 * (1024 * 1026 if fe.radix == 1 else fe.radix * fe.sub * fe.sub)
      plane_bytes = rows * 1024 * 4                      # bf16x3 operand plane: hi + lo
      spec_bytes = rows * fe.ld_spec * 4
      gemm_bytes = plane_bytes + spec_bytes
      pipe_bytes = B * T2 * 256 * 4 + 2 * plane_bytes + 2 * spec_bytes + B * T2 * 80 * 4
      roof = dict(bound="mfma", kernel=(f"gemm_kernel<taps=1,split=2>: {fe.radix} real DFTs of {1024 // fe.radix} points per frame as one batched MFMA product (decimation in time, radix {fe.radix})"
                                        if fe.radix > 1 else "gemm_kernel<taps=1,split=2> (real DFT 1024 -> 513 re + 513 im as an MFMA product)"),
                  achieved=flop / avg / 1e12, peak=PEAK_MFMA_BF16_TFLOPS, unit="TFLOP/s", frac=flop / avg / 1e12 / PEAK_MFMA_BF16_TFLOPS,
                  traffic=None, avg_launch_us=avg * 1e6, launches_measured=len(durs), algorithmic_flop_per_launch=flop,
                  mfma_issue_frac=3 * flop / avg / 1e12 / PEAK_MFMA_BF16_TFLOPS,
                  algorithmic_bytes_per_launch=gemm_bytes, hbm_frac_algorithmic=gemm_bytes / avg / 1e9 / PEAK_HBM_GBS,
                  dense_product_flop=2.0 * B * T2 * 1024 * 1026,
                  pipeline=dict(bound="hbm", call_us=call * 1e6, algorithmic_bytes=pipe_bytes, achieved_gbs=pipe_bytes / call / 1e9,
                                frac=pipe_bytes / call / 1e9 / PEAK_HBM_GBS,
                                note="frame pack + product + logmel of one call (events around the call); bytes: audio in, operand plane written + read, spectrum written + read, mel out"))
    if rank == 0:
        res = dict(metric="mel-frames/sec (on-device log-mel front-end, 64 x 800 frames, n_fft 1024 / hop 256 / 80 mel)",
                   value=world * B * T2 / dt, unit="mel-frames/s", n_gpus=world, steps=a.steps, warmup=a.warmup, ms_per_step=dt * 1e3,
                   higher_is_better=True, scaling="weak", vs_baseline=None, dtype="f32 (FFT in registers / LDS)" if fe.radix == 0 else "bf16x3 (split-bf16 MFMA, fp32-class)", data="synthetic",
                   config={"workload": "log-mel front-end B=64 x 204800 samples -> 800 frames x 80 mel", "batch_per_gpu": B, "mel_len": T2,
                           "parallelism": f"replicas x{world}"}, roofline=roof)
        if world == 1 and not a.no_cpu_baseline:
            from oracle import logmel_oracle as LO          # cpu_baseline leg: the oracle as the thing timed
            ya = audio[:8].cpu()
            torch.set_num_threads(min(os.cpu_count() or 1, 16))
            LO.mel_spectrogram(ya)
            ts = []
            for _ in range(5):
                t1 = time.perf_counter(); LO.mel_spectrogram(ya); ts.append(time.perf_counter() - t1)
            med = sorted(ts)[len(ts) // 2]
            res["cpu_baseline"] = dict(value=8 * T2 / med, unit="mel-frames/s", cores=min(os.cpu_count() or 1, 16), kind="port",
                                       sample=f"oracle mel_spectrogram (torch.stft fp32), 8 x 204800 samples, median of 5 ({med*1e3:.1f} ms)")
        print(json.dumps(res), flush=True)


def run_vocoder(a, world, rank, dev):
    """Row f-4: HiFi-GAN V1 generator (nntts/vocoders/hifigan_model.py, HiFiGAN_LJ_V1 config, random-init weights),
    one 800-frame mel -> 204 800 samples (9.3 s of audio) per step; `vocoder8`: a batch of 8 such utterances per step."""
    from efficient_tts_amd.vocoder import HiFiGANGenerator
    import torch.distributed as dist
    cfg = dict(resblock="1", upsample_rates=[8, 8, 2, 2], upsample_kernel_sizes=[16, 16, 4, 4], upsample_initial_channel=512,
               resblock_kernel_sizes=[3, 7, 11], resblock_dilation_sizes=[[1, 3, 5], [1, 3, 5], [1, 3, 5]], num_mels=80)
    T2 = 800
    NB = 8 if a.workload == "vocoder8" else 1
    torch.manual_seed(0)
    model = HiFiGANGenerator(cfg, precision=a.precision).to(dev).eval()
    model.remove_weight_norm()
    model.branch_streams = os.environ.get("EFTS_VOC_BRANCH", "1") == "1"       # (A/B: the residual blocks of a stage side by side / one after the other)
    mel = (torch.randn(NB, 80, T2, generator=torch.Generator().manual_seed(1234 + rank)) * 1.5 - 4.0).to(dev)
    for _ in range(max(a.warmup, 1)):
        y = model(mel)
    assert y.shape == (NB, 1, T2 * 256) and bool(torch.isfinite(y).all())
    torch.cuda.synchronize()
    if world > 1:
        dist.barrier()
    t0 = time.perf_counter()
    for _ in range(a.steps):
        model(mel)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    if world > 1:
        t = torch.tensor([dt], dtype=torch.float64, device=dev)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        dt = float(t.item())
    dt /= a.steps
    # algorithmic FLOPs of the generator per frame (2 * cin * cout * taps per output sample of every layer)
    fl, ch, length = 2 * 80 * 512 * 7, 512, 1
    for u, k in zip(cfg["upsample_rates"], cfg["upsample_kernel_sizes"]):
        fl += 2 * ch * (ch // 2) * k * length                    # transposed conv: k / u taps per output sample, length * u samples
        ch, length = ch // 2, length * u
        fl += sum(2 * ch * ch * kk * 6 for kk in cfg["resblock_kernel_sizes"]) * length
    fl += 2 * ch * 7 * length
    # roofline (round 6): every efts_gemm launch of two eager passes bracketed by HIP events, grouped by (taps, rows, cout): per group the share of
    # the call, TFLOP/s against the bf16 MFMA peak and algorithmic GB/s (operand plane in, fp32 stream + operand plane out, weights) against HBM;
    # `roofline` = the group with the largest share, bound by whichever of its two fractions is the larger
    from efficient_tts_amd import ops as Pops
    keep_g, model.graphs = model.graphs, False
    model(mel)
    torch.cuda.synchronize()
    Pops.PROFILE, Pops.PROFILE_TAG = [], None
    Pops.PROFILE_INFO.clear()
    for _ in range(2):
        model(mel)
    torch.cuda.synchronize()
    groups = {}
    for tag, s0, s1 in Pops.PROFILE:
        groups.setdefault(tag, []).append(s0.elapsed_time(s1) * 1e-3)
    info = dict(Pops.PROFILE_INFO)
    Pops.PROFILE, Pops.PROFILE_TAG = None, None
    model.graphs = keep_g
    sp = model.split
    rows_out = []
    total_gemm = sum(sum(v) for v in groups.values()) / 2
    for (taps, m_, n_), ds in groups.items():
        k_, _, _ = info[(taps, m_, n_)]
        per = sum(ds) / len(ds)
        flop_l = 2.0 * m_ * n_ * k_ * taps
        bytes_l = m_ * k_ * 2 * sp + m_ * n_ * (4 + 2 * sp) + taps * n_ * k_ * 2 * sp
        rows_out.append(dict(taps=taps, rows=m_, cout=n_, cin=k_, launches_per_call=len(ds) // 2, avg_launch_us=per * 1e6, share_of_gemm_time=sum(ds) / 2 / total_gemm,
                             tflops=flop_l / per / 1e12, mfma_frac=(3 if sp == 2 else 1) * flop_l / per / 1e12 / PEAK_MFMA_BF16_TFLOPS,
                             algorithmic_gbs=bytes_l / per / 1e9, hbm_frac=bytes_l / per / 1e9 / PEAK_HBM_GBS))
    rows_out.sort(key=lambda r: -r["share_of_gemm_time"])
    top = rows_out[0] if rows_out else None
    roof = None
    if top is not None:
        mf = top["tflops"] / PEAK_MFMA_BF16_TFLOPS
        bound = "hbm" if top["hbm_frac"] > mf else "mfma"
        roof = dict(bound=bound, kernel=f"gemm_kernel (efts_gemm): the generator's Conv1d launches of {top['taps']} taps, {top['cin']} -> {top['cout']} channels over {top['rows']} rows "
                                       f"({top['launches_per_call']} per call, {100 * top['share_of_gemm_time']:.0f} % of the contraction time)",
                    achieved=top["algorithmic_gbs"] if bound == "hbm" else top["tflops"], peak=PEAK_HBM_GBS if bound == "hbm" else PEAK_MFMA_BF16_TFLOPS,
                    unit="GB/s" if bound == "hbm" else "TFLOP/s", frac=top["hbm_frac"] if bound == "hbm" else mf, traffic=None,
                    avg_launch_us=top["avg_launch_us"], launches_measured=2 * top["launches_per_call"], groups=rows_out[:6],
                    contraction_ms_per_call=total_gemm * 1e3,
                    note="algorithmic bytes per launch = operand plane in + fp32 stream and operand plane out + weights; traffic (PMC) not collected for this row")
    if rank == 0:
        res = dict(metric=f"mel-frames/sec (HiFi-GAN V1 generator, {NB} x 800-frame utterance per step)", value=world * NB * T2 / dt,
                   unit="mel-frames/s", n_gpus=world, steps=a.steps, warmup=a.warmup, ms_per_step=dt * 1e3, higher_is_better=True,
                   scaling="weak", vs_baseline=None, dtype=a.precision if a.precision == "bf16" else "bf16x3 (split-bf16 MFMA, fp32-class)",
                   data="synthetic", config={"workload": f"HiFi-GAN V1 generator, mel [{NB}, 80, 800] -> {NB} x 204800 samples", "mel_len": T2,
                                              "precision": a.precision, "parallelism": f"replicas x{world}"},
                   rtf=dt / (NB * T2 * 256 / 22050.0), tflops=fl * NB * T2 / dt / 1e12, roofline=roof,
                   call_issue="one hipGraph replay per call (the generator's per-shape graph cache decides from its first calls)" if model.graphs else "eager launches")
        pol = [e.policy for e in model._graph_cache.entries.values() if e.policy is not None]
        if pol:
            res["config"]["call_policy"] = dict(chosen=pol[-1][0], host_ms_to_issue=pol[-1][1] * 1e3, device_ms=pol[-1][2] * 1e3)
        if world == 1 and not a.no_cpu_baseline:
            from oracle import hifigan_oracle as HO                  # cpu_baseline leg: the oracle as the thing timed
            P = {k: v.detach().cpu() for k, v in model.state_dict().items()}
            Pw = {}
            for k, v in P.items():                                   # the oracle takes weight_g / weight_v pairs
                if k.endswith(".weight"):
                    Pw[k + "_v"] = v
                    Pw[k + "_g"] = v.flatten(1).norm(dim=1).view(-1, 1, 1)
                else:
                    Pw[k] = v
            torch.set_num_threads(min(os.cpu_count() or 1, 32))
            Tc = 100
            mc = mel[:1, :, :Tc].cpu()
            with torch.no_grad():
                ref = HO.forward(Pw, mc)
                t1 = time.perf_counter(); HO.forward(Pw, mc); tc = time.perf_counter() - t1
                got = model(mel[:1, :, :Tc].contiguous())
            res["cpu_baseline"] = dict(value=Tc / tc, unit="mel-frames/s", cores=min(os.cpu_count() or 1, 32), kind="port",
                                       sample=f"oracle generator fp32, one {Tc}-frame mel ({tc:.2f} s)",
                                       hip_vs_oracle_audio_max_abs=float((got.cpu() - ref).abs().max()))
        print(json.dumps(res), flush=True)


def run_infer_lj(a, world, rank, dev, sub=None):
    """BASELINE config 1 plumbing on the GPU: free-running inference() of the first 10 LJSpeech test
    utterances (what nntts/bin/inference.py:97 iterates), one at a time (B = 1, as the reference), plus
    the same 10 as ONE ragged batch (inference_batch).  RTF = acoustic-model time / audio duration
    (T2 * 256 / 22050 s); the reference's RTF print also includes the vocoder (inference.py:111)."""
    import numpy as np
    from efficient_tts_amd import EfficientTTSCNN
    g = np.load(os.path.join(ROOT, "tests", "golden", "inference_lj.npz"))
    ids = [torch.from_numpy(g[f"ids{n}"]) for n in range(10)]
    torch.manual_seed(0)
    model = EfficientTTSCNN(num_symbols=76, dropout_rate=0.0, use_masking=True, sigma=0.01, precision=a.precision)
    with torch.no_grad():      # random-init weights; bias the duration head to ~6 frames/phoneme so T2 is LJSpeech-like
        model.duration_predictor.linear.bias.fill_(1.9)
    P = {k: v.detach().clone() for k, v in model.state_dict().items()}     # the CPU baseline leg times the same weights
    model = model.to(dev).eval()
    model.remove_weight_norm()
    dids = [x[None].to(dev) for x in ids]
    T1 = max(len(x) for x in ids)
    batch = torch.zeros(10, T1, dtype=torch.int64)
    for n, x in enumerate(ids):
        batch[n, :len(x)] = x
    lens = torch.tensor([len(x) for x in ids])
    batch, lens = batch.to(dev), lens.to(dev)
    for _ in range(max(a.warmup, 1)):
        frames = sum(model.inference(x)[0].shape[1] for x in dids)
        model.inference_batch(batch, lens)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(a.steps):
        for x in dids:
            model.inference(x)
    torch.cuda.synchronize()
    dt1 = (time.perf_counter() - t0) / a.steps
    t0 = time.perf_counter()
    for _ in range(a.steps):
        model.inference_batch(batch, lens)
    torch.cuda.synchronize()
    dtb = (time.perf_counter() - t0) / a.steps
    audio = frames * 256 / 22050.0
    # end to end, as nntts/bin/inference.py:105-111 times it: acoustic model + HiFi-GAN generator per utterance
    from efficient_tts_amd.vocoder import HiFiGANGenerator
    voc = HiFiGANGenerator(dict(resblock="1", upsample_rates=[8, 8, 2, 2], upsample_kernel_sizes=[16, 16, 4, 4], upsample_initial_channel=512,
                                resblock_kernel_sizes=[3, 7, 11], resblock_dilation_sizes=[[1, 3, 5], [1, 3, 5], [1, 3, 5]], num_mels=80),
                           precision=a.precision).to(dev).eval()
    voc.remove_weight_norm()
    for x in dids:
        voc(model.inference(x)[0].transpose(1, 2).contiguous())
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(a.steps):
        for x in dids:
            voc(model.inference(x)[0].transpose(1, 2).contiguous())
    torch.cuda.synchronize()
    dte = (time.perf_counter() - t0) / a.steps

    def batched_e2e():                                   # the same 10 utterances: one ragged acoustic pass + one ragged vocoder pass
        mel_b, mel_lens, _ = model.inference_batch(batch, lens)
        return voc(mel_b.transpose(1, 2).contiguous(), mel_lens)
    batched_e2e()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(a.steps):
        batched_e2e()
    torch.cuda.synchronize()
    dteb = (time.perf_counter() - t0) / a.steps
    res = dict(metric="mel-frames/sec (EFTS-CNN free-running inference, 10 LJSpeech test utterances, B=1 each)", value=frames / dt1,
               unit="mel-frames/s", n_gpus=1, steps=a.steps, warmup=a.warmup, ms_per_step=dt1 * 1e3, higher_is_better=True,
               scaling="weak", vs_baseline=None, dtype=a.precision, data="LJSpeech test phoneme ids (reference filelist), random-init weights with the duration head biased to ~6 frames per phoneme",
               config=dict(workload="inference() x 10 utterances, B=1", frames=frames, precision=a.precision),
               rtf=dt1 / audio, batched=dict(value=frames / dtb, ms=dtb * 1e3, rtf=dtb / audio, note="same 10 utterances as one ragged batch (inference_batch)"),
               end_to_end=dict(ms=dte * 1e3, rtf=dte / audio, note="inference() + HiFi-GAN V1 generator per utterance (random-init vocoder weights): what nntts/bin/inference.py:105-111 calls RTF"),
               end_to_end_batched=dict(ms=dteb * 1e3, rtf=dteb / audio, note="the 10 utterances as one ragged batch through inference_batch() and the batched generator"))
    # roofline of the dominant kernel at one utterance: the decoder's k5 Conv1d 512 -> 512 launches (T2 = 400-800 rows each: the small-M
    # tiling of efts_gemm), HIP events around every such launch of one eager pass over the 10 utterances
    from efficient_tts_amd import ops as Pops
    keep = model.graphs
    model.graphs = False
    for x in dids[:2]:
        model.inference(x)
    torch.cuda.synchronize()
    Pops.PROFILE, Pops.PROFILE_TAG = [], None
    for x in dids:
        model.inference(x)
    torch.cuda.synchronize()
    k5 = [(tag[1], s0.elapsed_time(s1) * 1e-3) for (tag, s0, s1) in Pops.PROFILE if tag[0] == 5 and tag[2] == 512 and tag[1] >= 256]
    Pops.PROFILE, Pops.PROFILE_TAG = None, None
    model.graphs = keep
    if k5:
        flop = sum(2.0 * m * 512 * 512 * 5 for m, _ in k5)
        tsum = sum(t for _, t in k5)
        res["roofline"] = dict(bound="mfma", kernel="the decoder's k5 Conv1d 512 -> 512 launches at ONE utterance (mel-length row spaces of 400-800 rows: "
                               "efts_gemm's small-M tiling, K split across the waves); latency-bound by construction, the figure says how far",
                               achieved=flop / tsum / 1e12, peak=PEAK_MFMA_BF16_TFLOPS, unit="TFLOP/s", frac=flop / tsum / 1e12 / PEAK_MFMA_BF16_TFLOPS,
                               traffic=None, avg_launch_us=tsum / len(k5) * 1e6, launches_measured=len(k5),
                               rows_per_launch=[min(m for m, _ in k5), max(m for m, _ in k5)])
    if not a.no_cpu_baseline:
        from oracle import efts_oracle as O           # cpu_baseline leg: the oracle as the thing timed, and as the checker
        torch.set_num_threads(sub["threads"] if sub else min(os.cpu_count() or 1, 16))
        with torch.no_grad():
            for x in ids[:2]:
                O.inference(P, x[None])
            t0 = time.perf_counter()
            refs = [O.inference(P, x[None])["mel_pred"] for x in ids]
            dc = time.perf_counter() - t0
            gots = [model.inference(x)[0].detach().cpu() for x in dids]
        res["cpu_baseline"] = dict(value=frames / dc, unit="mel-frames/s", cores=torch.get_num_threads(), kind="port", rtf=dc / audio,
                                   sample="oracle inference() fp32 on the same 10 utterances, one pass")
        def against_oracle(gs):
            same = [g.shape == r.shape for g, r in zip(gs, refs)]
            return dict(t2_equal_to_oracle=f"{sum(same)} of {len(same)} utterances",
                        hip_vs_oracle_mel_max_abs=max([float((g - r).abs().max()) for g, r, ok in zip(gs, refs, same) if ok] or [float("nan")]))
        res.update(against_oracle(gots))
        res["hip_vs_oracle_note"] = (f"mel of every utterance whose frame count T2 = round(sum of the predicted durations) equals the oracle's, same weights; precision {a.precision}: "
                                     "a bf16-operand duration predictor moves a sum of ~70 durations across a rounding boundary for some utterances (random-init weights); "
                                     "the 1e-3 grade is parity_mode (bf16x3)")
        if a.precision == "bf16" and a.parity_mode:
            mp = EfficientTTSCNN(num_symbols=76, dropout_rate=0.0, use_masking=True, sigma=0.01, precision="bf16x3")
            mp.load_state_dict(P)
            mp = mp.to(dev).eval()
            mp.remove_weight_norm()
            with torch.no_grad():
                for _ in range(max(a.warmup, 1)):                     # W passes over ALL ten utterances, like the bf16 leg above (two utterances only
                    for x in dids:                                    # left eight shapes' first calls and graph captures inside the timed region:
                        mp.inference(x)                               # 4.4 instead of 3.2 ms per ten with the driver's 5 + 20 steps)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(a.steps):
                    for x in dids:
                        mp.inference(x)
                torch.cuda.synchronize()
                dtp = (time.perf_counter() - t0) / a.steps
                res["parity_mode"] = dict(precision="bf16x3", ms_per_step=dtp * 1e3, value=frames / dtp, tolerance=1e-3,
                                          **against_oracle([mp.inference(x)[0].detach().cpu() for x in dids]))
            del mp
    if sub is not None:
        return res
    print(json.dumps(res), flush=True)


def _self_launch(a) -> int:
    """`python bench.py --gpus N` without a launcher: start the N ranks ourselves -- this same command line under
    torch.distributed.run on 127.0.0.1 -- and pass rank 0's JSON line through.  Fails (non-zero) unless N ranks come up."""
    import socket
    if a.workload != "rendezvous" and os.environ.get("EFTS_BENCH_BACKEND", "nccl") == "nccl":
        have = torch.cuda.device_count()
        if have < a.gpus:
            raise SystemExit(f"--gpus {a.gpus}: only {have} GPU(s) visible on this node; refusing to measure fewer ranks than asked for")
    sock = socket.socket()
    sock.bind(("127.0.0.1", 0))
    port = sock.getsockname()[1]
    sock.close()
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={a.gpus}", "--master-addr", "127.0.0.1",
           "--master-port", str(port), os.path.abspath(__file__)] + sys.argv[1:]
    env = dict(os.environ, EFTS_BENCH_SELF_LAUNCHED="1")
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    env.setdefault("OMP_NUM_THREADS", "8")
    return subprocess.call(cmd, env=env)


def run_rendezvous(a, world, rank):
    """launch check (also the CPU test of the self-launcher): every rank joins the group, one all-reduce counts them"""
    import torch.distributed as dist
    if world > 1:
        t = torch.ones(1, device="cuda" if torch.cuda.is_available() else "cpu")
        dist.all_reduce(t)
        seen = int(t.item())
    else:
        seen = 1
    if rank == 0:
        print(json.dumps(dict(metric="ranks that joined the process group", value=seen, unit="ranks", n_gpus=world, ranks_seen=seen,
                              backend=dist.get_backend() if world > 1 else None, self_launched=bool(os.environ.get("EFTS_BENCH_SELF_LAUNCHED")))), flush=True)
    if world > 1:
        dist.destroy_process_group()
    assert seen == a.gpus, f"--gpus {a.gpus} but {seen} ranks joined"


def main():
    a = parse()
    if a.test_shape:
        tb, t1, t2 = (int(v) for v in a.test_shape.split(","))
        for k in ("fwd64", "train32"):
            WORKLOADS[k].update(B=tb, T1=t1, T2=t2, desc=WORKLOADS[k]["desc"] + f" [TEST SHAPE {tb} x ({t1}, {t2}): a plumbing run, not a measurement]")
    if a.dump_outputs and a.workload not in ("fwd64", "fwd16_long"):
        raise SystemExit(f"--dump-outputs: written by the forward workloads (fwd64, fwd16_long), not by --workload {a.workload}")
    if "WORLD_SIZE" not in os.environ and a.gpus > 1:
        raise SystemExit(_self_launch(a))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    if world != a.gpus:
        raise SystemExit(f"--gpus {a.gpus} but WORLD_SIZE={world}: the launcher must start exactly --gpus ranks")
    on_gpu = torch.cuda.is_available()
    # EFTS_BENCH_BACKEND=gloo (tests only): the ranks share the visible GPUs, so the whole N > 1 code path of this script can be driven
    # on a one-GPU box (RCCL needs a GPU per rank); the data-parallel record then says backend gloo and skips the captured step
    backend = os.environ.get("EFTS_BENCH_BACKEND", "nccl")
    a.allow_gloo = backend != "nccl"
    if a.workload != "rendezvous" or on_gpu:
        dev = torch.device("cuda", local if backend == "nccl" else local % max(torch.cuda.device_count(), 1))
        torch.cuda.set_device(dev)
    if world > 1:
        import torch.distributed as dist
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        if a.workload == "train32" or (a.workload == "fwd64" and a.train_record):
            # RCCL's own account of the topology and of the algorithm / protocol it picks per collective goes to per-rank FILES
            # (never to stdout: the contract is ONE JSON line); efficient_tts_amd/bench_train.py quotes it in the `dp` record
            os.environ.setdefault("NCCL_DEBUG", "INFO")
            os.environ.setdefault("NCCL_DEBUG_SUBSYS", "INIT,TUNING")
            os.environ.setdefault("NCCL_DEBUG_FILE", f"/tmp/efts_rccl_{os.getpid()}_%h_%p.log")
        if on_gpu and backend == "nccl":
            dist.init_process_group("nccl", device_id=dev)
        else:
            dist.init_process_group("gloo")
    if a.workload == "rendezvous":
        return run_rendezvous(a, world, rank)

    from efficient_tts_amd import EfficientTTSCNN, ops as P
    if a.rc_kernel:
        P.RC_KERNEL = a.rc_kernel
    if a.workload == "stock_gpu":
        if rank == 0:
            print(json.dumps(dict(metric="mel-frames/sec (stock torch-ROCm ops: the oracle on the GPU)", unit="mel-frames/s", n_gpus=1,
                                  stock_gpu_baseline=stock_gpu_baseline(dev, find=bool(a.stock_find), budget_s=900.0))), flush=True)
        return None
    if a.workload == "infer_lj":
        return run_infer_lj(a, world, rank, dev)
    if a.workload == "infer64":
        return run_infer64(a, world, rank, dev)
    if a.workload == "logmel64":
        return run_logmel64(a, world, rank, dev)
    if a.workload in ("vocoder", "vocoder8"):
        return run_vocoder(a, world, rank, dev)
    wl = WORKLOADS[a.workload]
    B, T1, T2 = wl["B"], wl["T1"], wl["T2"]
    if a.workload == "train32":
        from efficient_tts_amd.bench_train import run_train      # DP training step (config 3/4)
        return run_train(a, world, rank, dev, wl, cpu_baseline_fn=cpu_train_baseline)

    return run_forward(a, world, rank, dev, wl)


def conv_roofline(P, model, step, B, T2, precision, workload, a=None, traffic_ok=True):
    """The dominant kernel (k5 residual Conv1d 512 -> 512 at mel length): per-launch duration from HIP events recorded
    on the launch stream around every such launch of 3 EAGER steps (graphs off), against the dense bf16 MFMA peak."""
    rows = P.Rows(B, T2).rows
    keep = model.graphs
    model.graphs = False
    step()                                                       # first eager step after graph replays: not measured
    torch.cuda.synchronize()
    P.PROFILE, P.PROFILE_TAG = [], (5, rows, 512)
    for _ in range(3):
        step()
    torch.cuda.synchronize()
    durs = [s.elapsed_time(e) * 1e-3 for (tag, s, e) in P.PROFILE if tag == (5, rows, 512)]
    P.PROFILE, P.PROFILE_TAG = None, None
    model.graphs = keep
    if not durs:                                                 # (--test-shape: no launch of the dominant kernel at all)
        return dict(bound="mfma", kernel="no efts_resconv5 launch at mel length in this shape", achieved=None, peak=PEAK_MFMA_BF16_TFLOPS, unit="TFLOP/s", frac=None, traffic=None)
    avg = sum(durs) / max(len(durs), 1)
    flop = 2.0 * B * T2 * 512 * 512 * 5
    # algorithmic bytes per launch: per element of the [rows, 512] stream 2 B hi + 2 B lo read, 4 B hi + lo
    # written (bf16x3: one 4 B hi|lo chunk read, one written), plus the weight plane once
    alg_bytes = rows * 512 * 8 + 5 * 512 * 512 * (2 if model.split == 1 else 4)
    traffic, src = None, None
    got = measure_traffic(a, precision, workload) if (a is not None and traffic_ok and a.measure_traffic and a.gpus == 1) else None
    # the bare-MFMA-stream ceiling of this box: measured at N = 1 only (at N > 1 every rank would run the whole-chip micro benchmark at once, on
    # top of the other ranks' timed work); the committed round-5 figure is quoted there, and says so
    sust = sustained_mfma_tflops() if (a is None or a.gpus == 1) else (1757.6, "profiles/mfma_ceiling_r05.txt (N > 1: not measured in this run)")
    if got is not None:
        traffic, src = got
    tf = os.path.join(ROOT, "profiles", "traffic.json")
    if traffic is None and os.path.exists(tf):
        try:
            traffic = json.load(open(tf)).get(f"{precision}:{workload}")
            src = "profiles/traffic.json (rocprofv3 PMC passes of this workload: 2 * FETCH_SIZE + WRITE_SIZE per launch; not measured in this run)"
        except Exception:
            traffic = None
    return dict(bound="mfma", kernel=f"resconv5_kernel<split={model.split}> (efts_resconv5: persistent 8-wave workgroups, 256-column tiles, hi/lo bf16 stream): "
                                      f"k5 Conv1d 512->512, {B}x{T2} frames (the decoder's launches; the mel encoder's carry a text-encoder layer each and are not in this average)",
                achieved=flop / avg / 1e12, peak=PEAK_MFMA_BF16_TFLOPS, unit="TFLOP/s", frac=flop / avg / 1e12 / PEAK_MFMA_BF16_TFLOPS,
                traffic=traffic, traffic_source=src, avg_launch_us=avg * 1e6, launches_measured=len(durs),
                algorithmic_flop_per_launch=flop, algorithmic_bytes_per_launch=alg_bytes,
                hbm_frac_algorithmic=alg_bytes / avg / 1e9 / PEAK_HBM_GBS,
                mfma_issue_frac=(3 if model.split == 2 else 1) * flop / avg / 1e12 / PEAK_MFMA_BF16_TFLOPS,
                # extra key: against what this box sustains on a bare MFMA stream with random operands -- `frac` stays vs 2.5 PF
                frac_of_sustained=flop / avg / 1e12 / sust[0],
                mfma_issue_frac_of_sustained=(3 if model.split == 2 else 1) * flop / avg / 1e12 / sust[0],
                sustained_mfma_tflops=sust[0], sustained_source=sust[1])


def _watchdog(seconds, rank, res, key, partial=None, code=3):
    """a timer that, when it fires, prints rank 0's line (with `key` marked as abandoned, or holding what `partial()` returns: the part of
    the record that had been measured) and ends the process; .cancel() disarms it"""
    import threading

    def fire():
        if res is not None and rank == 0:
            note = f"abandoned after {seconds} s without finishing (a rank hung); the rest of the line stands"
            part = partial() if partial is not None else None
            if isinstance(part, dict):
                part.setdefault("config", {})["watchdog"] = note
                res.setdefault(key, part)
            res.setdefault(key, dict(error=note))
            try:
                import copy
                print(json.dumps(copy.deepcopy(res)), flush=True)      # (a snapshot: the main thread may still be writing `res`)
            except Exception:                                          # noqa: BLE001
                pass
        os._exit(code)                                                 # a fired watchdog is a failed run for callers that gate on the code
    t = threading.Timer(seconds, fire)
    t.daemon = True
    t.start()
    return t


def run_forward(a, world, rank, dev, wl, sub=None):
    """BASELINE config 2 (fwd64) / config 5 (fwd16_long): the teacher-forced forward.  The timed step is a PLAIN
    `model(text, tl, mel, sl)` call -- what a drop-in caller of the reference class executes; the model replays a per-shape
    hipGraph internally (efficient_tts_amd/graphs.py).  --graph 1 times a bench-level graph of the eager launches instead.
    `sub` (dict(workload=..., threads=...)): the record is a SUB-RECORD of the default line (config 5 beside config 2): same K / W, both
    precisions, roofline from HIP events, the oracle as checker and as a one-pass CPU leg -- no call modes, no PMC child passes, no training
    record; returned instead of printed."""
    from efficient_tts_amd import EfficientTTSCNN, ops as P
    B, T1, T2 = wl["B"], wl["T1"], wl["T2"]
    wname = sub["workload"] if sub else a.workload
    text, tl, mel, sl = synth(B, T1, T2, 1234 + rank, dev)

    def build(precision, params=None):
        torch.manual_seed(0)
        m = EfficientTTSCNN(num_symbols=76, dropout_rate=0.0, use_masking=True, use_weighted_masking=False, sigma=0.01, precision=precision)
        if params is not None:
            m.load_state_dict(params)
        m = m.to(dev).eval()
        m.side_stream, m.resconv = bool(a.side_stream), bool(a.resconv)
        m.fuse_soft_index = bool(a.fuse_soft_index)
        m.fuse_prenet = bool(a.fuse_prenet)
        if a.resconv_min_rows >= 0:
            m.RESCONV_MIN_ROWS = a.resconv_min_rows
        return m

    def barrier():
        if world > 1:
            import torch.distributed as dist
            dist.barrier()

    def timed(model, steps, warmup, mode):
        """mode: 'call' plain model() calls; 'graph' a bench-level hipGraph of the eager launches; 'eager' graphs off"""
        keep = model.graphs
        model.graphs = mode == "call"

        def step():
            with torch.no_grad():
                return model(text, tl, mel, sl)
        graph = None
        for _ in range(max(warmup, 2)):
            out = step()
        torch.cuda.synchronize()
        if mode == "graph":
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph):
                out = step()
            graph.replay()
            torch.cuda.synchronize()
        barrier()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(steps):
            if graph is not None:
                graph.replay()
            else:
                out = step()
        torch.cuda.synchronize()
        barrier()
        dt = time.perf_counter() - t0
        model.graphs = keep
        if world > 1:
            import torch.distributed as dist
            t = torch.tensor([dt], dtype=torch.float64, device=dev)
            dist.all_reduce(t, op=dist.ReduceOp.MAX)
            dt = float(t.item())
        loss = float(out[0])
        assert loss == loss, "NaN loss"
        return dt, loss, step, out

    model = build(a.precision)
    mode = "graph" if a.graph == 1 else ("call" if a.model_graphs else "eager")
    dt, loss, step, out = timed(model, a.steps, a.warmup, mode)          # ---- THE timed region: exactly K steps
    if a.dump_outputs and rank == 0 and sub is None:
        dump_outputs(a.dump_outputs, forward_outputs(out))              # (before any further step: graph replays write into the same buffers)
    del out
    roof = conv_roofline(P, model, step, B, T2, a.precision, wname, a, traffic_ok=sub is None) if a.full else None

    def line(precision, dt, steps):
        frames = world * B * T2 * steps
        return dict(value=frames / dt, ms_per_step=dt / steps * 1e3, per_gpu=frames / dt / world,
                    rtf=(dt / steps) / (B * T2 * 256 / 22050.0),
                    tflops=FWD_FLOP_PER_ITEM * B * T2 / 800 * world * steps / dt / 1e12 if (T1, T2) == (128, 800) else None)

    res = None
    if rank == 0:
        res = dict(metric=f"mel-frames/sec (EFTS-CNN forward, batch {B}/GPU, 80-mel LJSpeech shape)", unit="mel-frames/s", n_gpus=world,
                   steps=a.steps, warmup=a.warmup, higher_is_better=True, scaling="weak", vs_baseline=None,
                   dtype="bf16" if a.precision == "bf16" else "bf16x3 (split-bf16 MFMA, fp32-class)", data="synthetic",
                   config=dict(workload=wl["desc"], batch_per_gpu=B, phoneme_len=T1, mel_len=T2, precision=a.precision,
                               parallelism=f"replicas x{world}",
                               hipgraph={"graph": "bench-level hipGraph of the eager launches", "call": "plain model() calls (the model decides per shape from its first calls: replay a hipGraph, or stay on eager launches where the host runs far ahead of the device anyway -- see call_policy)",
                                         "eager": "none: every kernel launched from the host"}[mode]),
                   loss=loss, roofline=roof)
        res.update(line(a.precision, dt, a.steps))
        pol = [e.policy for e in model._graph_cache.entries.values() if e.policy is not None]
        if mode == "call" and pol:
            res["config"]["call_policy"] = dict(chosen=pol[-1][0], host_ms_to_issue=pol[-1][1] * 1e3, device_ms=pol[-1][2] * 1e3,
                                                rule=f"eager when host <= {type(model._graph_cache).EAGER_MAX_HOST_SHARE} x device")
    # ---- the parity-grade mode under the same clock: bf16x3 (mel max-abs <= 1e-3 vs the fp32 oracle), same K / W, same inputs
    parity_model = None
    if a.precision == "bf16" and a.parity_mode:
        parity_model = build("bf16x3", {k: v.detach() for k, v in model.state_dict().items()})
        dt2, loss2, step2, _ = timed(parity_model, a.steps, a.warmup, mode)
        roof2 = conv_roofline(P, parity_model, step2, B, T2, "bf16x3", wname, a, traffic_ok=sub is None) if a.full else None
        if rank == 0:
            res["parity_mode"] = dict(precision="bf16x3", dtype="bf16x3 (split-bf16 MFMA operands: hi*hi + hi*lo + lo*hi, fp32 accumulate)",
                                      steps=a.steps, warmup=a.warmup, loss=loss2, roofline=roof2, **line("bf16x3", dt2, a.steps))
    if rank == 0 and world == 1 and a.call_modes and sub is None:
        cm = {}
        for md in ("call", "graph", "eager"):
            d, _, _, _ = timed(model, 10, 2, md)
            cm[md + "_ms"] = d / 10 * 1e3
        res["call_modes"] = dict(cm, note="10 steps each after the timed region: plain model() call (the model's own per-shape choice) / bench-level hipGraph / eager launches")
    if rank == 0 and world == 1 and not a.no_cpu_baseline:
        checks = {}

        def hip_check(Pd, text_c, tl_c, mel_c, sl_c):
            out = None
            for prec in ("bf16", "bf16x3"):
                m2 = build(prec, Pd)
                with torch.no_grad():
                    checks[prec] = m2(text_c.to(dev), tl_c.to(dev), mel_c.to(dev), sl_c.to(dev))[4].detach().cpu()
                if prec == a.precision:
                    out = checks[prec]
            return out
        res["cpu_baseline"] = cpu_baseline(T1, T2, hip_check) if sub is None else cpu_baseline(T1, T2, hip_check, Bc=B, threads=[sub["threads"]], passes=1)
        ref = res["cpu_baseline"].pop("_ref_mel", None)
        if ref is not None and "parity_mode" in res:
            res["parity_mode"]["hip_vs_oracle_mel_max_abs"] = float((checks["bf16x3"] - ref).abs().max())
            res["parity_mode"]["tolerance"] = 1e-3
        if ref is not None:
            res["hip_vs_oracle_mel_max_abs"] = float((checks[a.precision] - ref).abs().max())
            # the headline cannot be read without its error: the bf16 mode is config 2's stated dtype, NOT the 1e-3 parity grade (that is `parity_mode`)
            res["config"]["mel_max_abs_vs_fp32"] = res["hip_vs_oracle_mel_max_abs"]
            res["config"]["mel_max_abs_vs_fp32_note"] = "this precision's mel_pred against the fp32 oracle, same parameters and inputs (2 items); north_star's 1e-3 is met by parity_mode (bf16x3)"
    if sub is not None:
        return res
    if rank == 0 and world == 1 and a.workload == "fwd64" and a.sub_records and not os.environ.get("EFTS_BENCH_CHILD"):
        # ---- the other BASELINE configs under the same invocation: config 5 (B=16 x 1200 frames, both precisions), config
        # 2-ii (batched free-running inference B=64) and config 1 (10 LJSpeech utterances one by one), each with ms_per_step, roofline,
        # the oracle as checker (hip_vs_oracle_mel_max_abs) and ONE bounded CPU pass at the fwd64 leg's thread choice
        nt = (res.get("cpu_baseline") or {}).get("cores") or min(os.cpu_count() or 1, 16)
        for key, fn in (("long16", lambda: run_forward(a, 1, 0, dev, WORKLOADS["fwd16_long"], sub=dict(workload="fwd16_long", threads=nt))),
                        ("infer64", lambda: run_infer64(a, 1, 0, dev, sub=dict(threads=nt))),
                        ("infer_lj", lambda: run_infer_lj(a, 1, 0, dev, sub=dict(threads=nt)))):
            t0 = time.perf_counter()
            try:
                res[key] = fn()
                res[key]["record_wall_s"] = time.perf_counter() - t0
            except Exception as exc:                                   # noqa: BLE001 -- a sub-record must not cost the line
                res[key] = dict(error=f"{type(exc).__name__}: {exc}"[:300])
            torch.cuda.empty_cache()
    if a.workload == "fwd64" and a.train_record and not os.environ.get("EFTS_BENCH_CHILD"):
        # ---- BASELINE configs 3 / 4 under the same invocation, on EVERY rank: the training step at B=32 per GPU (fwd + bwd + clip +
        # Adam-amsgrad; N > 1: the bucketed RCCL gradient all-reduce overlapped with the backward -> its `dp` record), 40 steps; and
        # its parity-grade mode (bf16x3) under the same clock
        from efficient_tts_amd.bench_train import measure_train
        torch.cuda.empty_cache()
        # N > 1: the forward result above must survive whatever the data-parallel record runs into on hardware this code has not seen
        # (a rank that fails alone leaves the others inside a collective).  An exception costs the record, not the line; a hang is
        # cut by a watchdog that prints the line with what there is and ends the process on every rank.
        dog = _watchdog(int(os.environ.get("EFTS_BENCH_DP_TIMEOUT", "240")), rank, res, "train32", partial=lambda: getattr(a, "partial_train", None)) if world > 1 else None
        failed = False
        try:
            tsteps, twarm = (40, 10) if not a.test_shape else (a.steps, a.warmup)
            tr = measure_train(a, world, rank, dev, WORKLOADS["train32"], steps=tsteps, warmup=twarm)      # (None on ranks other than 0)
        except Exception as exc:                                       # noqa: BLE001 -- the line must still be printed
            if world == 1:
                raise
            tr, failed = None, True
            if res is not None:
                res["train32"] = dict(error=f"rank {rank}: {type(exc).__name__}: {exc}"[:400])
        trp = None
        if not failed and a.precision == "bf16" and a.parity_mode and not (rank == 0 and tr and tr["config"].get("device_state")):
            try:
                trp = measure_train(a, world, rank, dev, WORKLOADS["train32"], steps=tsteps, warmup=twarm, precision="bf16x3")
            except Exception as exc:                                   # noqa: BLE001 -- the line must still be printed
                trp = None
                if rank == 0:
                    tr["config"]["parity_mode_note"] = f"not measured: {exc}"[:200]
        if dog is not None:
            dog.cancel()
        if rank == 0 and tr is not None:
            if trp is not None:
                tr["parity_mode"] = {k: trp[k] for k in ("value", "ms_per_step", "eager_ms_per_step", "graph_ms_per_step", "dtype", "loss", "tflops", "roofline", "steps", "warmup")}
                tr["parity_mode"]["note"] = ("bf16x3 operands: the mode the gradient-vs-oracle tests run in (tests/test_gpu_train.py); the bf16 mode's own "
                                             "gradient error is stated by test_bf16_mode_gradients_report_their_own_error")
            if world == 1:
                got = measure_traffic(a, a.precision, "train32") if (a.measure_traffic and a.gpus == 1) else None
                if got is not None:
                    tr["roofline"]["traffic"], tr["roofline"]["traffic_source"] = got
                if trp is not None:
                    gotp = measure_traffic(a, "bf16x3", "train32") if (a.measure_traffic and a.gpus == 1) else None
                    if gotp is not None:
                        tr["parity_mode"]["roofline"]["traffic"], tr["parity_mode"]["roofline"]["traffic_source"] = gotp
                if not a.no_cpu_baseline:
                    tr["cpu_baseline"] = cpu_train_baseline(T1, T2)
            res["train32"] = tr
            if world > 1 and isinstance(tr.get("dp"), dict):
                # what a reader of the N > 1 line wants first: the top-level `value` is the collective-free replica forward; the path WITH
                # the RCCL exchange is the training step, lifted here (whole-job frames/s, ms per step, this run's own scaling efficiency
                # = step without the exchange / step with it, and the part of the exchange the backward did not hide)
                res["dp_value"], res["dp_unit"], res["dp_ms_per_step"] = tr["value"], tr["unit"], tr["ms_per_step"]
                res["dp_efficiency"], res["dp_exposed_ms"] = tr["dp"].get("efficiency"), tr["dp"].get("exposed_ms")
                res["dp_note"] = ("training step B=32/GPU with the bucketed RCCL gradient exchange (train32); dp_efficiency = the same step's time with the "
                                  "exchange switched off / with it, both eager, same run (train32.dp.step_ms_*)")
    if rank == 0 and world == 1 and a.stock_gpu and not a.no_cpu_baseline and not os.environ.get("EFTS_BENCH_CHILD"):
        sg = stock_gpu_baseline(dev, find=bool(a.stock_find))
        res["stock_gpu_baseline"] = sg
        # what the two libraries make of the same configs on the same GPU in the same run (this library's figure / the stock ops' figure)
        if "fwd64_bf16_autocast" in sg:
            res["vs_stock_gpu"] = dict(fwd64_bf16=res["value"] / sg["fwd64_bf16_autocast"]["value"],
                                       fwd64_parity_mode_vs_fp32=(res["parity_mode"]["value"] / sg["fwd64_fp32"]["value"]) if ("parity_mode" in res and "fwd64_fp32" in sg) else None)
            tr = res.get("train32") if isinstance(res.get("train32"), dict) else None
            if tr and "train32_bf16_autocast" in sg and "value" in tr:
                res["vs_stock_gpu"]["train32_bf16"] = tr["value"] / sg["train32_bf16_autocast"]["value"]
            if tr and "train32_fp32" in sg and isinstance(tr.get("parity_mode"), dict):
                res["vs_stock_gpu"]["train32_parity_mode_vs_fp32"] = tr["parity_mode"]["value"] / sg["train32_fp32"]["value"]
    if rank == 0:
        print(json.dumps(res), flush=True)
    if world > 1:
        import torch.distributed as dist
        _watchdog(60, rank, None, None, code=0)                                # the line is out: a tear-down that hangs must not hold the launcher
        try:
            dist.destroy_process_group()
        except Exception:                                              # noqa: BLE001 -- the line is out; nothing left to lose
            pass
        bad = rank == 0 and isinstance(res, dict) and isinstance(res.get("train32"), dict) and "error" in res["train32"]
        os._exit(3 if bad else 0)


if __name__ == "__main__":
    main()
